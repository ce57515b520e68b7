// Host program over csrc/uplift_grad_plan.h for tests/test_uplift_grad_plan_host.py
// (g++ -std=c++17 -O1 -g -fsanitize=address,undefined; run as a child process, never loaded into python).
//   layout D HD NT POS FIRST SECOND        "tensors N total T hole B L", then one "t n k offset used" line per tensor
//   group BATCH LEN [BATCH LEN ...]        group_size of every pair, one per line
//   workspace D HD NT POS FIRST SECOND     the plan of every batch x len of the sweep: "cases N", a "FAIL ..." line per violation
//   attention                              the geometry of every hd x S x direction: "cases N max_lds B", "FAIL ..." lines
//   served HD NT LEN                       grad_attention_served as 0 / 1
#include "../../upliftingtabletennis_amd/csrc/uplift_grad_plan.h"
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace ttup::upl;

static GradDims dims(char** a) { return {atoi(a[0]), atoi(a[1]), atoi(a[2]), atoi(a[3]), atoi(a[4]), atoi(a[5])}; }

// what stands for a buffer here: where the plan put it and the rows x width it was sized from
struct Buf { long long off, rows, width; long long cap() const { return rows * width; } };

static long long g_bad;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL " __VA_ARGS__); printf("\n"); ++g_bad; } } while (0)

static void check_plan(const GradDims& d, int batch, int len) {
    std::vector<Buf> all;
    PlanT<Buf> p;
    plan_workspace(d, batch, len, &p, [&](long long off, long long rows, long long width) { all.push_back({off, rows, width}); return all.back(); });
    const long long D = d.D, NT = d.n_table, G = p.G;
    CHECK(G == group_size(batch, len) && p.nt == G * len && p.n1 == G * len * (NT + 1) && p.n2 == G * (len + 1) && p.nk == G * NT, "rows B=%d T=%d", batch, len);
    CHECK((long long)all.size() == 5LL * (d.pos_layers + d.first_layers + d.second_layers) + 3 + 25, "buffer count %zu B=%d T=%d", all.size(), batch, len);
    // 16-byte boundaries, no overlap, inside the total
    std::vector<Buf> by_off = all;
    std::sort(by_off.begin(), by_off.end(), [](const Buf& a, const Buf& b) { return a.off < b.off; });
    for (size_t i = 0; i < by_off.size(); ++i) {
        const long long end = i + 1 < by_off.size() ? by_off[i + 1].off : p.total;
        CHECK(by_off[i].off >= 0 && by_off[i].off % 4 == 0, "alignment off=%lld B=%d T=%d", by_off[i].off, batch, len);
        CHECK(by_off[i].cap() > 0 && by_off[i].off + by_off[i].cap() <= end, "overlap off=%lld cap=%lld next=%lld B=%d T=%d", by_off[i].off, by_off[i].cap(), end, batch, len);
    }
    // what a full group uses of every buffer (csrc/uplift_grad.hip: layer_fwd / layer_bwd, head_*, embed_*, group_pass)
    auto use = [&](const char* name, const Buf& b, long long rows, long long width) {
        CHECK(b.cap() >= rows * width, "%s holds %lld, %lld x %lld used, B=%d T=%d", name, b.cap(), rows, width, batch, len);
    };
    const StageT<Buf>* stages[3] = {&p.table, &p.temporal, &p.spin};
    const long long tokens[3] = {p.n1, p.nt, p.n2};
    const int layers[3] = {d.pos_layers, d.first_layers, d.second_layers};
    for (int s = 0; s < 3; ++s) {
        CHECK((int)stages[s]->L.size() == layers[s] && stages[s]->tokens == tokens[s] && (long long)stages[s]->n_seq * stages[s]->S == tokens[s], "stage %d B=%d T=%d", s, batch, len);
        for (const auto& L : stages[s]->L) {
            use("x", L.x, tokens[s], D); use("qkv", L.qkv, tokens[s], 3 * D); use("att", L.att, tokens[s], D); use("x2", L.x2, tokens[s], D); use("hp", L.hp, tokens[s], D);
        }
        use("out", stages[s]->out, tokens[s], D);
        // the layers' scratch: LayerNorm outputs and d att (tA), ReLU output / d hp / LayerNorm-1 output (tB), d x2 (tC), dy xhat (tE), dqkv (tQ)
        use("tA", p.tA, tokens[s], D); use("tB", p.tB, tokens[s], D); use("tC", p.tC, tokens[s], D); use("tE", p.tE, tokens[s], D); use("tQ", p.tQ, tokens[s], 3 * D);
    }
    use("dX", p.dX, p.n2, D); use("dX", p.dX, p.n1, D); use("dY", p.dY, p.nt, D);
    // head_bwd(rotation head: G rows; position head: nt rows): t1 = tB, t2 = tC, dx = tA or dY
    use("tB", p.tB, p.nt, D / 2); use("tC", p.tC, p.nt, D / 4); use("tA", p.tA, G, D);
    // assemble_bwd: d ball_tok -> tA, d table_tok -> tB;  embed_bwd: tmp = tC
    use("tA", p.tA, p.nt, D); use("tB", p.tB, p.nk, D); use("tC", p.tC, p.nt, D); use("tC", p.tC, p.nk, D);
    use("ball_h", p.ball_h, p.nt, D); use("ball_tok", p.ball_tok, p.nt, D); use("tab_h", p.tab_h, p.nk, D); use("tab_tok", p.tab_tok, p.nk, D);
    use("pos_h1", p.pos_h1, p.nt, D / 2); use("pos_h2", p.pos_h2, p.nt, D / 4); use("rot_h1", p.rot_h1, G, D / 2); use("rot_h2", p.rot_h2, G, D / 4);
    use("m1", p.m1, p.nt, 1); use("m2", p.m2, p.n2, 1); use("tmask", p.tmask, G, NT + 1); use("txy", p.txy, p.nk, 2);
    use("rope", p.rope, p.nt * (d.hd / 2), 2); use("rot_t", p.rot_t, G, 3); use("d_rot", p.d_rot, G, 3); use("d_pos", p.d_pos, p.nt, 3); use("mask_sum", p.mask_sum, 1, 1);
    // the sliced reductions: dW = dY^T X (n x k partial products per slice of KSLICE rows) and the column sums behind every vector
    const GradLayout lay = grad_layout(d);
    for (const GradTensor& t : lay.t) {
        if (!t.used) continue;
        const long long M = p.rows(t.rows);
        CHECK(M > 0, "tensor at %lld: no rows", t.offset);
        CHECK(p.partial.cap() >= (M + 511) / 512 * t.count(), "partial holds %lld, tensor at %lld needs %lld slices x %lld, B=%d T=%d", p.partial.cap(), t.offset,
              (M + 511) / 512, t.count(), batch, len);
    }
}

static int workspace(const GradDims& d) {
    long long cases = 0;
    for (int batch : {1, 2, 3, 5, 64, 80})
        for (int len : {1, 2, 15, 16, 17, 64, 128, 171, 250, 255}) { ++cases; check_plan(d, batch, len); }
    printf("cases %lld\nfailures %lld\n", cases, g_bad);
    return 0;
}

static int attention() {
    long long cases = 0;
    size_t max_lds = 0;
    for (int hd : {8, 16, 24, 32})
        for (int S = 1; S <= 257; ++S)
            for (int bwd = 0; bwd < 2; ++bwd) {
                ++cases;
                const AttnGeom g = attn_geom(S, hd, bwd != 0);
                if (S == 257) { CHECK(!g.ok, "S=257 hd=%d bwd=%d is served", hd, bwd); continue; }
                int P = 16;
                while (P < S) P *= 2;
                const int seqs = P < 64 ? 64 / P : 1;
                const size_t lds = (size_t)seqs * ((bwd ? 4 : 2) * S * hd + (bwd ? 3 * S : 0) + S) * 4;
                CHECK(g.ok && g.P == P && g.seqs == seqs && g.threads == seqs * P && g.threads <= 256 && g.threads >= 64 && g.lds == lds && g.lds <= 160 * 1024,
                      "S=%d hd=%d bwd=%d: ok=%d P=%d seqs=%d threads=%d lds=%zu", S, hd, bwd, (int)g.ok, g.P, g.seqs, g.threads, g.lds);
                if (g.lds > max_lds) max_lds = g.lds;
            }
    for (int hd : {0, 4, 12, 40, 64}) { ++cases; CHECK(!attn_geom(16, hd, false).ok, "hd=%d is served", hd); }
    printf("cases %lld max_lds %zu\nfailures %lld\n", cases, max_lds, g_bad);
    return 0;
}

int main(int argc, char** argv) {
    const char* cmd = argc > 1 ? argv[1] : "";
    if (!strcmp(cmd, "layout") && argc == 8) {
        const GradLayout L = grad_layout(dims(argv + 2));
        printf("tensors %zu total %lld hole %lld %lld\n", L.t.size(), L.total, L.hole_begin, L.hole_len);
        for (const GradTensor& t : L.t) printf("t %d %d %lld %d\n", t.n, t.k, t.offset, (int)t.used);
        return 0;
    }
    if (!strcmp(cmd, "group") && argc >= 4 && argc % 2 == 0) {
        for (int i = 2; i < argc; i += 2) printf("%d\n", group_size(atoi(argv[i]), atoi(argv[i + 1])));
        return 0;
    }
    if (!strcmp(cmd, "workspace") && argc == 8) return workspace(dims(argv + 2));
    if (!strcmp(cmd, "attention") && argc == 2) return attention();
    if (!strcmp(cmd, "served") && argc == 5) {
        printf("%d\n", (int)grad_attention_served(GradDims{0, atoi(argv[2]), atoi(argv[3]), 0, 0, 0}, atoi(argv[4])));
        return 0;
    }
    fprintf(stderr, "usage: %s layout|workspace D HD NT POS FIRST SECOND | group BATCH LEN ... | attention | served HD NT LEN\n", argv[0]);
    return 2;
}
