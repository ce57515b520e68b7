// Host program over csrc/vitpose_grad_plan.h for tests/test_vitpose_grad_plan_host.py
// (g++ -std=c++17 -O1 -g -fsanitize=address,undefined; run as a child process, never loaded into python).
//   table IN_CH NTOK          "key ndim d0 d1 d2 d3 offset count" per tensor, then "total N"; offsets checked for overlap
//   workspace                 the plan over max_rows x in_ch: alignment, overlap, sizing, bytes a token
//   slices TOKENS [...]       "tokens slices last" per argument; then "slice_tokens N"
//   attn NTOK BATCH [...]     "ntok batch gx gy gz walk dx dy" per pair; then "lds BYTES"
//   refusals                  check_create / check_forward / check_backward on a table
// Every checking command prints a "FAIL ..." line per violation, "cases N" and "failures N".
#include "../../upliftingtabletennis_amd/csrc/vitpose_grad_plan.h"
#include <algorithm>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace ttup::vgrad;

static long long g_bad, g_cases;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL " __VA_ARGS__); printf("\n"); ++g_bad; } } while (0)

static int table(int in_ch, int ntok) {
    const GradTable g = grad_table(in_ch, ntok);
    size_t end = 0;
    for (const GradTensor& t : g.t) {
        size_t n = 1;
        for (int i = 0; i < t.ndim; ++i) n *= (size_t)t.shape[i];
        if (t.offset != end || n != t.count || t.count % 4) { printf("FAIL %s offset %zu count %zu\n", t.key.c_str(), t.offset, t.count); return 0; }
        end = t.offset + t.count;
        printf("%s %d %lld %lld %lld %lld %zu %zu\n", t.key.c_str(), t.ndim, t.shape[0], t.shape[1], t.shape[2], t.shape[3], t.offset, t.count);
    }
    if (end != g.total || (int)g.t.size() != TENSORS) { printf("FAIL total %zu end %zu tensors %zu\n", g.total, end, g.t.size()); return 0; }
    // the enum's positions are the table's
    const char* at[][2] = {{"pos_embed", nullptr}, {"patch_embed.proj.weight", nullptr}, {"patch_embed.proj.bias", nullptr}};
    for (int i = 0; i < 3; ++i)
        if (g.t[i].key != at[i][0]) printf("FAIL position %d is %s\n", i, g.t[i].key.c_str());
    if (g.t[block_tensor(3, T_QKVW)].key != "blocks.3.attn.qkv.weight" || g.t[block_tensor(11, T_FC2B)].key != "blocks.11.mlp.fc2.bias" ||
        g.t[T_LNW].key != "last_norm.weight" || g.t[T_LNB].key != "last_norm.bias" || g.t[block_tensor(0, T_N1W)].key != "blocks.0.norm1.weight")
        printf("FAIL enum positions\n");
    printf("total %zu\n", g.total);
    return 0;
}

static void workspace() {
    const char* names[B_COUNT] = {"x", "xmid", "st1", "st2", "stl", "qkv", "lse", "att", "pre", "col", "hid", "dhid", "br", "ln", "g", "dln", "dqkv", "delta",
                                  "sums", "partial", "scale"};
    for (long long T : {1LL, 2LL, 63LL, 64LL, 65LL, 511LL, 512LL, 513LL, 1024LL, 1025LL, 23040LL, (long long)MAX_ROWS})
        for (int C : {1, 3, 9, 16}) {
            const int mb = T >= 8 ? 8 : (int)T;
            const Workspace w = plan_workspace(T, C, mb);
            std::vector<int> order(B_COUNT);
            for (int i = 0; i < B_COUNT; ++i) order[i] = i;
            std::sort(order.begin(), order.end(), [&](int a, int b) { return w.off[a] < w.off[b]; });
            for (int i = 0; i < B_COUNT; ++i) {
                const int b = order[i];
                const size_t end = i + 1 < B_COUNT ? w.off[order[i + 1]] : w.total;
                CHECK(w.off[b] % SMALL_ALIGN == 0 && (w.bytes[b] < LARGE_ALIGN || w.off[b] % LARGE_ALIGN == 0), "%s not aligned T=%lld", names[b], T);
                CHECK(w.bytes[b] > 0 && w.off[b] + w.bytes[b] <= end, "%s overlaps its neighbour T=%lld", names[b], T);
            }
            // what a forward + backward at T tokens puts into every buffer (csrc/vitpose_grad.hip)
            const size_t t = (size_t)T, S = (size_t)slices(T);
            const size_t use[B_COUNT] = {13 * t * DIM * 4, 12 * t * DIM * 4, 12 * t * 8, 12 * t * 8, t * 8, 12 * t * 3 * DIM * 4, 12 * t * HEADS * 4, 12 * t * DIM * 4,
                                         12 * t * MLP * 4, t * C * 256 * 4, t * MLP * 4, t * MLP * 4, t * DIM * 4, t * DIM * 4, t * DIM * 4, t * DIM * 4,
                                         t * 3 * DIM * 4, t * HEADS * 4, S * 2 * MLP * 8, S * DIM * (size_t)std::max(MLP, 256 * C) * 4, (size_t)24 * mb * 4};
            size_t kept = 0, scratch = 0;
            for (int b = 0; b < B_COUNT; ++b) {
                CHECK(w.bytes[b] >= use[b], "%s holds %zu, %zu used, T=%lld C=%d", names[b], w.bytes[b], use[b], T, C);
                if (b <= B_COL) kept += w.bytes[b];
                else if (b <= B_DELTA) scratch += w.bytes[b];
            }
            CHECK(kept == kept_floats_per_token(C) * 4 * t && scratch == scratch_floats_per_token() * 4 * t, "bytes a token T=%lld C=%d: %zu %zu", T, C, kept, scratch);
            CHECK(kept_floats_per_token(C) * 4 == 186632 + 1024 * (size_t)C && scratch_floats_per_token() * 4 == 23088, "the documented bytes a token");
            ++g_cases;
        }
}

static void refusals() {
    auto bad = [](const Refusal& r) { return r.rc == TTUP_EINVAL && r.msg[0]; };
    auto ok = [](const Refusal& r) { return r.rc == TTUP_OK; };
    CHECK(bad(check_create(0, 2, 2, 1)) && bad(check_create(17, 2, 2, 1)) && bad(check_create(-3, 2, 2, 1)) && ok(check_create(1, 2, 2, 1)) && ok(check_create(16, 2, 2, 1)), "in_ch");
    CHECK(bad(check_create(3, 0, 2, 1)) && bad(check_create(3, 2, -1, 1)) && bad(check_create(3, 2, 2, 0)) && ok(check_create(3, 1, 1, 1)), "non-positive");
    CHECK(ok(check_create(3, 2048, 2048, 1)) && bad(check_create(3, 2048, 2049, 1)) && bad(check_create(3, 2048, 2048, 2)) && bad(check_create(3, 1 << 16, 1 << 16, 1 << 16)),
          "tokens beyond 2^22, and a product that overflows int");
    CHECK(bad(check_forward(4, 0, 0)) && bad(check_forward(4, -1, 0)) && bad(check_forward(4, 5, 0)) && ok(check_forward(4, 4, 0)) && ok(check_forward(4, 1, 0)), "batch");
    CHECK(ok(check_forward(4, 3, 72)) && bad(check_forward(4, 3, 71)) && bad(check_forward(4, 3, 96)) && bad(check_forward(4, 3, 24)) && bad(check_forward(4, 3, -72)), "drop_scale length");
    CHECK(bad(check_backward(0, 1)) && ok(check_backward(2, 2)) && bad(check_backward(2, 1)) && bad(check_backward(2, 3)), "backward");
    g_cases += 6;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "table") && argc == 4) return table(atoi(argv[2]), atoi(argv[3]));
    if (!strcmp(argv[1], "slices")) {
        for (int i = 2; i < argc; ++i) {
            const long long t = atoll(argv[i]);
            printf("%lld %d %lld\n", t, slices(t), ttup::vhead::last_slice_rows(t, 0));
        }
        printf("slice_tokens %d\n", SLICE_TOKENS);
        return 0;
    }
    if (!strcmp(argv[1], "attn")) {
        for (int i = 2; i + 1 < argc; i += 2) {
            const int n = atoi(argv[i]), b = atoi(argv[i + 1]);
            const AttnGrid g = attn_bwd_grid(n, b), d = attn_delta_grid((long long)n * b);
            printf("%d %d %u %u %u %d %u %u\n", n, b, g.x, g.y, g.z, g.walk, d.x, d.y);
        }
        printf("lds %zu\n", ATTN_BWD_LDS);
        return 0;
    }
    if (!strcmp(argv[1], "workspace")) workspace();
    else if (!strcmp(argv[1], "refusals")) refusals();
    else return 2;
    printf("cases %lld\nfailures %lld\n", g_cases, g_bad);
    return 0;
}
