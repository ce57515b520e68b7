// Host program over csrc/detect_grad_plan.h for tests/test_detect_grad_plan_host.py
// (g++ -std=c++17 -O1 -g -fsanitize=address,undefined; run as a child process, never loaded into python).
//   ranges                       every (in, out) of the sweep and the real pairs: "cases N", a "FAIL ..." line per violation
//   strips H W OUT_H OUT_W       the strips and column groups of one map shape: "strip S nstrips N waves V groups G lds B" (strip 0: refused), "FAIL ..." lines
//   unread IN OUT [IN OUT ...]   per pair one line "IN OUT: i i ...": the source indices whose dg_readers range is empty
#include "../../upliftingtabletennis_amd/csrc/detect_grad_plan.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace ttup;

static long long g_bad;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL " __VA_ARGS__); printf("\n"); ++g_bad; } } while (0)

// one axis: the ranges of dg_first / dg_readers against what dg_src_coord says index by index
static void check_axis(int in, int out) {
    const double scale = (double)in / (double)out;
    std::vector<int> i0(out), i1(out);
    std::vector<int> readers_lo(in, out), readers_hi(in, -1), readers_n(in, 0);
    for (int d = 0; d < out; ++d) {
        double lam, w0, w1;
        int a, b;
        dg_weights(d, scale, in, a, b, lam, w0, w1);
        i0[d] = a;
        i1[d] = b;
        CHECK(a >= 0 && a < in && (b == a + 1 || (b == a && a == in - 1)), "neighbours %d -> %d: dst %d reads %d, %d", in, out, d, a, b);
        CHECK(d == 0 || a >= i0[d - 1], "monotone %d -> %d: dst %d", in, out, d);
        CHECK(lam >= 0.0 && lam < 1.0 && w0 >= 0.0 && w1 >= 0.0 && (w1 == 0.0) == (b == a || lam == 0.0), "weights %d -> %d: dst %d lam %g", in, out, d, lam);
        CHECK(fabs(w0 + w1 - 1.0) <= 2.220446049250313e-16, "weights %d -> %d: dst %d sums to 1 %+g", in, out, d, w0 + w1 - 1.0);
        CHECK(b != a || w0 == (1.0 - lam) + lam, "folded weight %d -> %d: dst %d", in, out, d);
        for (int r : {a, b}) {
            if (d < readers_lo[r]) readers_lo[r] = d;
            if (d > readers_hi[r]) readers_hi[r] = d;
        }
        readers_n[a] += 1;
        if (b != a) readers_n[b] += 1;
    }
    for (int k = -1; k <= in + 1; ++k) {
        int want = 0;
        while (want < out && i0[want] < k) ++want;
        CHECK(dg_first(k, scale, in, out) == want, "first %d -> %d: k %d gives %d, want %d", in, out, k, dg_first(k, scale, in, out), want);
    }
    int plo = 0, phi = 0;
    for (int i = 0; i < in; ++i) {
        int lo, hi;
        dg_readers(i, scale, in, out, lo, hi);
        CHECK(0 <= lo && lo <= hi && hi <= out && lo >= plo && hi >= phi, "range %d -> %d: source %d reads [%d, %d) after [%d, %d)", in, out, i, lo, hi, plo, phi);
        plo = lo;
        phi = hi;
        if (readers_n[i] == 0) {
            CHECK(lo == hi, "unread %d -> %d: source %d has the range [%d, %d)", in, out, i, lo, hi);
        } else {
            // contiguous: as many readers as the range is long, and its ends are the first and the last of them
            CHECK(lo == readers_lo[i] && hi == readers_hi[i] + 1 && hi - lo == readers_n[i], "readers %d -> %d: source %d has [%d, %d), read by %d in [%d, %d]", in, out, i, lo,
                  hi, readers_n[i], readers_lo[i], readers_hi[i]);
        }
    }
    for (int d = 0; d < out; ++d)
        for (int r : {i0[d], i1[d]}) {
            int lo, hi;
            dg_readers(r, scale, in, out, lo, hi);
            CHECK(lo <= d && d < hi, "member %d -> %d: dst %d reads %d whose range is [%d, %d)", in, out, d, r, lo, hi);
        }
}

static int ranges() {
    long long cases = 0;
    for (int in = 1; in <= 40; ++in)
        for (int out = 1; out <= 80; ++out) { ++cases; check_axis(in, out); }
    const int real[][2] = {{704, 1080}, {1280, 1920}, {160, 1080}, {288, 1920}, {1080, 1080}, {2048, 1920}, {64, 7}, {50, 9}};
    for (const auto& p : real) { ++cases; check_axis(p[0], p[1]); }
    printf("cases %lld\nfailures %lld\n", cases, g_bad);
    return 0;
}

static int strips(int h, int w, int out_h, int out_w) {
    const GradPlan p = dg_plan(h, w, out_h, out_w);
    printf("strip %d nstrips %d waves %d groups %d lds %zu\n", p.strip, p.nstrips, p.waves, p.groups, p.lds);
    if (p.strip == 0) {
        CHECK(p.nstrips == 0 && p.lds == 0 && p.waves == 0 && p.groups == 0, "a refused shape has strips");
        printf("failures %lld\n", g_bad);
        return 0;
    }
    CHECK(p.strip == (DG_STRIP < h ? DG_STRIP : h) && p.lds == dg_lds_bytes(p.strip, w, p.waves) && p.lds <= DG_LDS_BYTES, "budget: strip %d lds %zu", p.strip, p.lds);
    // the columns: every source column is owned by one lane 1 .. 63 of one wave of one group, lane 0 of that wave serves the column
    // before, and the group keeps every column its lanes serve, and the right neighbour of each, in LDS
    CHECK(p.waves >= 1 && p.waves <= DG_MAX_WAVES && p.groups >= 1, "waves %d groups %d", p.waves, p.groups);
    CHECK((long long)(p.groups - 1) * p.waves * DG_LANES < w && (long long)p.groups * (p.waves - 1) * DG_LANES < w, "%d groups of %d waves: a group without a column of %d, or a wave too many",
          p.groups, p.waves, w);
    std::vector<int> col_owned(w, 0);
    for (int g = 0; g < p.groups; ++g) {
        int lo, hi;
        dg_group_columns(g, p.waves, w, lo, hi);
        CHECK(0 <= lo && lo < hi && hi <= w && (size_t)(hi - lo) * (p.strip + 2) * sizeof(float) <= p.lds, "group %d keeps the columns [%d, %d)", g, lo, hi);
        for (int v = 0; v < p.waves; ++v)
            for (int lane = 0; lane < 64; ++lane) {
                const int j = dg_column(g, p.waves, v, lane);
                CHECK(lane == 0 || j == dg_column(g, p.waves, v, lane - 1) + 1, "lane %d of wave %d group %d serves column %d", lane, v, g, j);
                CHECK(lane > 0 || (v == 0 && g == 0 ? j == -1 : j == dg_column(v ? g : g - 1, p.waves, v ? v - 1 : p.waves - 1, 63)), "lane 0 of wave %d group %d serves column %d", v, g, j);
                if (j < 0 || j >= w) continue;
                CHECK(lo <= j && (j + 1 < w ? j + 1 : j) < hi, "group %d serves column %d and keeps [%d, %d)", g, j, lo, hi);
                if (lane >= 1) col_owned[j] += 1;
            }
    }
    for (int j = 0; j < w; ++j) CHECK(col_owned[j] == 1, "source column %d belongs to %d lanes", j, col_owned[j]);
    const double scale = (double)h / (double)out_h;
    std::vector<int> owned(h, 0);
    std::vector<double> weight(h, 0.0), seen(h, 0.0);          // per source row: the weights of its readers, and those its strip walked
    for (int y = 0; y < out_h; ++y) {
        int y0, y1;
        double lam, w0, w1;
        dg_weights(y, scale, h, y0, y1, lam, w0, w1);
        weight[y0] += w0;
        if (y1 != y0) weight[y1] += w1;
    }
    for (int s = 0; s < p.nstrips; ++s) {
        const int r0 = s * p.strip, nr = h - r0 < p.strip ? h - r0 : p.strip;
        CHECK(nr >= 1, "strip %d is empty", s);
        for (int r = r0; r < r0 + nr; ++r) owned[r] += 1;
        int lo, hi;
        dg_strip_rows(r0, p.strip, h, lo, hi);
        CHECK(lo >= 0 && hi <= h && hi - lo <= p.strip + 2, "strip %d keeps the rows [%d, %d)", s, lo, hi);
        // the kernel's walk: the output rows whose upper source row is r0 - 1 .. r0 + nr - 1
        const int ybeg = dg_first(r0 - 1, scale, h, out_h), yend = dg_first(r0 + nr, scale, h, out_h);
        for (int y = ybeg; y < yend; ++y) {
            int y0, y1;
            double lam, w0, w1;
            dg_weights(y, scale, h, y0, y1, lam, w0, w1);
            CHECK(y0 >= r0 - 1 && y0 <= r0 + nr - 1 && y0 >= lo && y1 < hi, "strip %d walks output row %d between the source rows %d, %d; it keeps [%d, %d)", s, y, y0, y1, lo, hi);
            if (y0 >= r0) seen[y0] += w0;
            if (y1 != y0 && y1 < r0 + nr) seen[y1] += w1;
        }
    }
    for (int r = 0; r < h; ++r) {
        CHECK(owned[r] == 1, "source row %d belongs to %d strips", r, owned[r]);
        CHECK(seen[r] == weight[r], "source row %d: its strip walked the weight %.17g of %.17g", r, seen[r], weight[r]);
    }
    printf("failures %lld\n", g_bad);
    return 0;
}

int main(int argc, char** argv) {
    const char* cmd = argc > 1 ? argv[1] : "";
    if (!strcmp(cmd, "ranges") && argc == 2) return ranges();
    if (!strcmp(cmd, "unread") && argc >= 4 && argc % 2 == 0) {
        for (int a = 2; a < argc; a += 2) {
            const int in = atoi(argv[a]), out = atoi(argv[a + 1]);
            printf("%d %d:", in, out);
            for (int i = 0; i < in; ++i) {
                int lo, hi;
                dg_readers(i, (double)in / (double)out, in, out, lo, hi);
                if (lo == hi) printf(" %d", i);
            }
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(cmd, "strips") && argc == 6) return strips(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]));
    fprintf(stderr, "usage: %s ranges | unread IN OUT ... | strips H W OUT_H OUT_W\n", argv[0]);
    return 2;
}
