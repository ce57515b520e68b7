// Host program over csrc/detect_loss_plan.h for tests/test_detect_loss_plan_host.py
// (g++ -std=c++17 -O1 -g -fsanitize=address,undefined; run as a child process, never loaded into python).
//   sweep               every (h, out_h) of the sweep and the real pairs at every width: "cases N", "noncontiguous M" (strips in the
//                       per-row-pair layout), a "FAIL ..." line per violation
//   plan H W OUT_H      one shape: "strip S slots L nstrips N lds B noncontiguous K" (strip 0: refused), "FAIL ..." lines
#include "../../upliftingtabletennis_amd/csrc/detect_loss_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace ttup;

static long long g_bad;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL " __VA_ARGS__); printf("\n"); ++g_bad; } } while (0)

// the most source rows a strip of height `strip` lies between, from dg_src_coord row by row: min(span, 2 rows) per strip
static int worst_rows(int h, int out_h, int strip) {
    const double scale = (double)h / (double)out_h;
    int worst = 0;
    for (int r0 = 0; r0 < out_h; r0 += strip) {
        const int nr = out_h - r0 < strip ? out_h - r0 : strip;
        int lo = h, hi = -1;
        for (int i = 0; i < nr; ++i) {
            int i0, i1;
            double lam;
            dg_src_coord(r0 + i, scale, h, i0, i1, lam);
            lo = i0 < lo ? i0 : lo;
            hi = i1 > hi ? i1 : hi;
        }
        const int need = hi - lo + 1 < 2 * nr ? hi - lo + 1 : 2 * nr;
        worst = need > worst ? need : worst;
    }
    return worst;
}

// one shape: the plan against the budget, and per strip the fill rule against the reads.  -> the strips in the non-contiguous layout
static int check_shape(int h, int w, int out_h, LossPlan& p) {
    p = loss_plan(h, w, out_h);
    CHECK((p.strip == 0) == ((size_t)(h < 2 ? h : 2) * w * sizeof(float) > DE_ROW_BYTES), "refusal %d x %d -> %d: strip %d", h, w, out_h, p.strip);
    if (p.strip == 0) {
        CHECK(p.slots == 0 && p.nstrips == 0 && p.lds == 0, "a refused shape has strips");
        return 0;
    }
    CHECK(p.strip >= 1 && p.strip <= DE_STRIP && p.nstrips == (out_h + p.strip - 1) / p.strip, "%d x %d -> %d: strip %d nstrips %d", h, w, out_h, p.strip, p.nstrips);
    for (int s = DE_STRIP; s >= p.strip; --s) {          // the largest height that fits: no taller one does
        const bool fits = (size_t)worst_rows(h, out_h, s) * w * sizeof(float) <= DE_ROW_BYTES;
        CHECK(fits == (s == p.strip), "%d x %d -> %d: strip %d chosen, height %d %s", h, w, out_h, p.strip, s, fits ? "fits" : "does not fit");
    }
    CHECK(p.slots == worst_rows(h, out_h, p.strip), "%d x %d -> %d: %d slots, the worst strip needs %d", h, w, out_h, p.slots, worst_rows(h, out_h, p.strip));
    CHECK(p.lds == (size_t)p.slots * w * sizeof(float) && p.lds <= DE_ROW_BYTES, "%d x %d -> %d: lds %zu for %d slots", h, w, out_h, p.lds, p.slots);
    const double scale = (double)h / (double)out_h;
    int noncontiguous = 0;
    std::vector<int> filled;
    for (int k = 0; k < p.nstrips; ++k) {
        const int r0 = k * p.strip, nr = out_h - r0 < p.strip ? out_h - r0 : p.strip;
        const LossStrip ls = dl_strip(r0, nr, scale, h);
        noncontiguous += !ls.contiguous;
        CHECK(nr >= 1 && ls.slots >= 1 && ls.slots <= p.slots, "%d -> %d strip %d: %d rows, %d slots of %d", h, out_h, k, nr, ls.slots, p.slots);
        filled.assign(ls.slots > 0 ? ls.slots : 0, -1);          // what the kernel's fill loop leaves in LDS
        for (int s = 0; s < ls.slots; ++s) {
            filled[s] = dl_slot_row(ls, r0, s, scale, h);
            CHECK(filled[s] >= 0 && filled[s] < h, "%d -> %d strip %d: slot %d is filled from row %d", h, out_h, k, s, filled[s]);
        }
        for (int i = 0; i < nr; ++i) {
            int i0, i1;
            double lam;
            dg_src_coord(r0 + i, scale, h, i0, i1, lam);
            const int a = dl_slot(ls, i, 0, i0), b = dl_slot(ls, i, 1, i1);
            const bool inside = a >= 0 && a < ls.slots && b >= 0 && b < ls.slots;
            CHECK(inside, "%d -> %d strip %d: row %d reads the slots %d, %d of %d", h, out_h, k, i, a, b, ls.slots);
            if (inside) CHECK(filled[a] == i0 && filled[b] == i1, "%d -> %d strip %d: row %d reads the rows %d, %d and finds %d, %d", h, out_h, k, i, i0, i1, filled[a], filled[b]);
        }
    }
    return noncontiguous;
}

static int sweep() {
    const int widths[] = {1, 1920, 2560, 3840, 7680};          // the budget binds at 8, 7, 5, 3 and 1 rows
    const int real[][2] = {{704, 1080}, {1280, 1920}, {160, 1080}, {288, 1920}, {1080, 1080}, {2048, 1920}, {64, 7}, {50, 9}};
    long long cases = 0, noncontiguous = 0;
    LossPlan p;
    for (int w : widths) {
        for (int h = 1; h <= 40; ++h)
            for (int out_h = 1; out_h <= 80; ++out_h) { ++cases; noncontiguous += check_shape(h, w, out_h, p); }
        for (const auto& r : real) { ++cases; noncontiguous += check_shape(r[0], w, r[1], p); }
    }
    printf("cases %lld\nnoncontiguous %lld\nfailures %lld\n", cases, noncontiguous, g_bad);
    return 0;
}

int main(int argc, char** argv) {
    const char* cmd = argc > 1 ? argv[1] : "";
    if (!strcmp(cmd, "sweep") && argc == 2) return sweep();
    if (!strcmp(cmd, "plan") && argc == 5) {
        LossPlan p;
        const int noncontiguous = check_shape(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), p);
        printf("strip %d slots %d nstrips %d lds %zu noncontiguous %d\nfailures %lld\n", p.strip, p.slots, p.nstrips, p.lds, noncontiguous, g_bad);
        return 0;
    }
    fprintf(stderr, "usage: %s sweep | plan H W OUT_H\n", argv[0]);
    return 2;
}
