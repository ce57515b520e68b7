// Host program over csrc/vitpose_head_plan.h (and gemm_modes.h's dgrad_index) for tests/test_vitpose_head_plan_host.py
// (g++ -std=c++17 -O1 -g -fsanitize=address,undefined; run as a child process, never loaded into python).
//   taps                     the tap <-> (phase, 2x2 tap) bijection and the three weight layouts as permutations of each other
//   gather                   dgrad_index against a brute-force scatter of the transposed convolution, grids 1x1 .. 6x6, batch 1 and 2
//   slices TOKENS [...]      "tokens slices last0 last1 last2" per argument; then the constants "slice_tokens N dwf_sub N"
//   workspace                the plan over max_rows x out_ch: alignment, overlap, sizing
//   refusals                 check_create / check_forward / check_backward on a table
// Every command prints a "FAIL ..." line per violation, "cases N" and "failures N".
#include "../../upliftingtabletennis_amd/csrc/vitpose_head_plan.h"
#include <algorithm>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace ttup::vhead;

static long long g_bad, g_cases;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL " __VA_ARGS__); printf("\n"); ++g_bad; } } while (0)

static void taps() {
    bool seen[4][4] = {};
    for (int ky = 0; ky < 4; ++ky)
        for (int kx = 0; kx < 4; ++kx) {
            const PhaseTap p = phase_of_tap(ky, kx);
            CHECK(p.phase >= 0 && p.phase < 4 && p.tap >= 0 && p.tap < 4 && !seen[p.phase][p.tap], "tap (%d,%d) -> (%d,%d)", ky, kx, p.phase, p.tap);
            seen[p.phase][p.tap] = true;
            const KernelTap k = tap_of_phase(p.phase, p.tap);
            CHECK(k.ky == ky && k.kx == kx, "inverse of (%d,%d) is (%d,%d)", ky, kx, k.ky, k.kx);
            // weights.vitpose_fold_head's rule: phase 2 py + px, tap 2 dy + dx <-> (3 - py - 2 dy, 3 - px - 2 dx)
            const int py = p.phase >> 1, px = p.phase & 1, dy = p.tap >> 1, dx = p.tap & 1;
            CHECK(ky == 3 - py - 2 * dy && kx == 3 - px - 2 * dx, "fold rule at (%d,%d)", ky, kx);
            // the geometry: output row 2y + py takes input row y + py + dy - 1 through tap ky means 2 (y + py + dy - 1) - 1 + ky = 2y + py
            CHECK(2 * (py + dy - 1) - 1 + ky == py && 2 * (px + dx - 1) - 1 + kx == px, "geometry at (%d,%d)", ky, kx);
            ++g_cases;
        }
    // pack (reference -> phase matrices, reference -> backward matrix) and un-pack (backward matrix -> reference) as permutations
    const int shapes[][2] = {{DIM, DEC}, {DEC, DEC}, {3, 5}, {1, 1}};
    for (const auto& s : shapes) {
        const int cin = s[0], cout = s[1];
        const size_t n = (size_t)cin * cout * 16;
        std::vector<char> ph(n, 0), pm(n, 0);
        for (int ci = 0; ci < cin; ++ci)
            for (int co = 0; co < cout; ++co)
                for (int ky = 0; ky < 4; ++ky)
                    for (int kx = 0; kx < 4; ++kx) {
                        const size_t r = ref_index(cin, cout, ci, co, ky, kx), a = phase_index(cin, cout, ci, co, ky, kx), b = perm_index(cin, cout, ci, co, ky, kx);
                        CHECK(r < n && a < n && b < n, "index out of range cin=%d cout=%d", cin, cout);
                        if (r >= n || a >= n || b >= n) continue;
                        CHECK(!ph[a] && !pm[b], "two weights in one slot cin=%d cout=%d", cin, cout);
                        ph[a] = pm[b] = 1;
                        CHECK(ref_of_perm(cin, cout, b) == r, "un-pack of pack at (%d,%d,%d,%d)", ci, co, ky, kx);
                        // the phase matrix's slot read back by the fold's formula
                        const PhaseTap p = phase_of_tap(ky, kx);
                        CHECK(a == (((size_t)p.phase * cout + co) * 4 + p.tap) * cin + ci, "phase slot at (%d,%d,%d,%d)", ci, co, ky, kx);
                    }
        ++g_cases;
    }
}

// dz -> da by scattering: every output pixel (oy, ox) = (2y - 1 + ky, 2x - 1 + kx) of the transposed convolution of input pixel (y, x)
static void gather() {
    const int C = 3;
    for (int batch = 1; batch <= 2; ++batch)
        for (int ih = 1; ih <= 6; ++ih)
            for (int iw = 1; iw <= 6; ++iw) {
                const long long rows = (long long)batch * ih * iw, nout = rows * 4 * C;
                // want[m][k]: the element the scatter pairs with (row m, column k), -1 where the tap leaves the map
                std::vector<long long> want((size_t)rows * 16 * C, -1);
                for (int b = 0; b < batch; ++b)
                    for (int y = 0; y < ih; ++y)
                        for (int x = 0; x < iw; ++x)
                            for (int ky = 0; ky < 4; ++ky)
                                for (int kx = 0; kx < 4; ++kx) {
                                    const int oy = 2 * y - 1 + ky, ox = 2 * x - 1 + kx;
                                    if (oy < 0 || oy >= 2 * ih || ox < 0 || ox >= 2 * iw) continue;
                                    for (int co = 0; co < C; ++co)
                                        want[(((size_t)b * ih + y) * iw + x) * 16 * C + (4 * ky + kx) * C + co] = (((long long)b * 2 * ih + oy) * 2 * iw + ox) * C + co;
                                }
                std::vector<int> uses((size_t)nout, 0);
                for (long long m = 0; m < rows; ++m)
                    for (int k = 0; k < 16 * C; ++k) {
                        const long long e = ttup::gemm::dgrad_index(m, k, ih, iw, C);
                        CHECK(e == want[(size_t)m * 16 * C + k], "gather B=%d %dx%d m=%lld k=%d: %lld, scatter %lld", batch, ih, iw, m, k, e, want[(size_t)m * 16 * C + k]);
                        CHECK(e < nout, "gather out of the map B=%d %dx%d", batch, ih, iw);
                        if (e >= 0 && e < nout) ++uses[(size_t)e];
                    }
                // every output pixel is reached by exactly four (input pixel, tap) pairs: 2 x 2 per axis... except at the border rows
                // and columns, which two input rows / columns would reach and one lies outside
                for (int oy = 0; oy < 2 * ih; ++oy)
                    for (int ox = 0; ox < 2 * iw; ++ox) {
                        const int ny = (oy == 0 || oy == 2 * ih - 1) ? 1 : 2, nx = (ox == 0 || ox == 2 * iw - 1) ? 1 : 2;
                        CHECK(uses[((size_t)oy * 2 * iw + ox) * C] == ny * nx, "uses of (%d,%d) in %dx%d: %d", oy, ox, ih, iw, uses[((size_t)oy * 2 * iw + ox) * C]);
                    }
                ++g_cases;
            }
}

static void workspace() {
    const char* names[B_COUNT] = {"feat", "z1", "a1", "z2", "a2", "d1", "d2", "wph1", "wph2", "wperm1", "wperm2", "small", "sums", "dwf", "partial"};
    for (long long T : {1LL, 2LL, 35LL, 64LL, 65LL, 511LL, 512LL, 513LL, 1024LL, 1025LL, 23040LL, (long long)MAX_ROWS})
        for (int C : {1, 13, 16}) {
            const Workspace w = plan_workspace(T, C);
            CHECK(ttup::vhead::check_create(C, T).rc == TTUP_OK, "create refuses T=%lld C=%d", T, C);
            std::vector<int> order(B_COUNT);
            for (int i = 0; i < B_COUNT; ++i) order[i] = i;
            std::sort(order.begin(), order.end(), [&](int a, int b) { return w.off[a] < w.off[b]; });
            for (int i = 0; i < B_COUNT; ++i) {
                const int b = order[i];
                const size_t end = i + 1 < B_COUNT ? w.off[order[i + 1]] : w.total;
                CHECK(w.off[b] % WS_ALIGN == 0, "%s not aligned T=%lld", names[b], T);
                CHECK(w.bytes[b] > 0 && w.off[b] + w.bytes[b] <= end, "%s overlaps its neighbour T=%lld", names[b], T);
            }
            // what a forward + backward at T tokens puts into every buffer (csrc/vitpose_head_grad.hip)
            const size_t t = (size_t)T, S = (size_t)slices(T);
            const size_t use[B_COUNT] = {t * DIM * 4, t * 4 * DEC * 4, t * 4 * DEC * 4, t * 16 * DEC * 4, t * 16 * DEC * 4, t * 4 * DEC * 4, t * 16 * DEC * 4,
                                         (size_t)4 * DEC * 4 * DIM * 4, (size_t)4 * DEC * 4 * DEC * 4, (size_t)DIM * 16 * DEC * 4, (size_t)DEC * 16 * DEC * 4,
                                         (size_t)SmallOff::COUNT * 4, S * 2 * DEC * 8, S * DWF_SUB * ((size_t)C * DEC + C) * 8, S * DIM * 16 * DEC * 4};
            for (int b = 0; b < B_COUNT; ++b) CHECK(w.bytes[b] >= use[b], "%s holds %zu, %zu used, T=%lld C=%d", names[b], w.bytes[b], use[b], T, C);
            CHECK(SmallOff::ZERO + DIM <= SmallOff::G1 && SmallOff::G1 + DEC <= SmallOff::G2 && SmallOff::G2 + DEC <= SmallOff::WF && SmallOff::WF + C * DEC <= SmallOff::BN1
                  && SmallOff::BN1 + 5 * DEC <= SmallOff::BN2 && SmallOff::BN2 + 5 * DEC == SmallOff::COUNT, "small offsets C=%d", C);
            CHECK(slice_rows(2) % DWF_SUB == 0, "a slice's pixels are not a whole number of dWf parts");
            ++g_cases;
        }
}

static void refusals() {
    auto bad = [](const Refusal& r) { return r.rc == TTUP_EINVAL && r.msg[0]; };
    auto ok = [](const Refusal& r) { return r.rc == TTUP_OK; };
    CHECK(bad(check_create(0, 8)) && bad(check_create(17, 8)) && bad(check_create(-1, 8)) && ok(check_create(1, 8)) && ok(check_create(16, 8)), "out_ch");
    CHECK(bad(check_create(1, 0)) && bad(check_create(1, -5)) && bad(check_create(1, MAX_ROWS + 1)) && ok(check_create(1, MAX_ROWS)) && ok(check_create(1, 1)), "max_rows");
    CHECK(bad(check_forward(8, 0, 2, 2)) && bad(check_forward(8, -1, 2, 2)) && bad(check_forward(8, 1, 0, 2)) && bad(check_forward(8, 1, 2, -3)), "non-positive");
    CHECK(ok(check_forward(8, 2, 2, 2)) && bad(check_forward(8, 3, 2, 2)) && bad(check_forward(8, 1, 3, 3)) && ok(check_forward(8, 1, 2, 4)), "rows");
    CHECK(bad(check_forward(8, 1 << 16, 1 << 16, 1 << 16)), "a product that overflows int");
    CHECK(bad(check_backward(0, 0, 0, 1, 2, 2)) && ok(check_backward(1, 2, 2, 1, 2, 2)) && bad(check_backward(1, 2, 2, 2, 2, 2)) && bad(check_backward(1, 2, 2, 1, 2, 3))
          && bad(check_backward(1, 2, 3, 1, 3, 2)), "backward");
    g_cases += 6;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "taps")) taps();
    else if (!strcmp(argv[1], "gather")) gather();
    else if (!strcmp(argv[1], "workspace")) workspace();
    else if (!strcmp(argv[1], "refusals")) refusals();
    else if (!strcmp(argv[1], "slices")) {
        for (int i = 2; i < argc; ++i) {
            const long long t = atoll(argv[i]);
            printf("%lld %d %lld %lld %lld\n", t, slices(t), last_slice_rows(t, 0), last_slice_rows(t, 1), last_slice_rows(t, 2));
        }
        printf("slice_tokens %d dwf_sub %d rows %lld %lld %lld\n", SLICE_TOKENS, DWF_SUB, slice_rows(0), slice_rows(1), slice_rows(2));
        return 0;
    } else return 2;
    printf("cases %lld\nfailures %lld\n", g_cases, g_bad);
    return 0;
}
