// The ViTPose head's training pass without a device (csrc/vitpose_head_grad.hip): the tap <-> (phase, 2x2 tap) bijection of
// ConvTranspose2d(k4, s2, p1) and the three weight layouts built on it, the slices of every fixed-order reduction, the checks an
// argument list has to pass and the one workspace the handle owns -- functions of plain integers.  Standard headers,
// include/ttup.h and gemm_modes.h only: the same source compiles for gfx950 (hipcc) and for the host (g++:
// tests/helpers/host_vitpose_head_plan.cpp).
#pragma once
#include "../../include/ttup.h"
#include "gemm_modes.h"
#include <stddef.h>
#include <stdio.h>

namespace ttup {
namespace vhead {

using namespace ttup::gemm;

constexpr int DIM = 384, DEC = 256, MAX_OUT = 16;          // last_norm's width, the deconvolutions' width, the most heatmaps
constexpr double BN_EPS = 1e-5, BN_MOMENTUM = 0.1;
constexpr long long MAX_ROWS = 1 << 22;                    // tokens a handle may be sized for: its 16 pixels a token stay far below 2^31 GEMM rows

// ------------------------------------------------------------------ the transposed convolution's taps
// Output pixel (2y + py, 2x + px) of phase p = 2 py + px reads input pixel (y + py + dy - 1, x + px + dx - 1), t = 2 dy + dx, through
// the reference kernel's tap (ky, kx) = (3 - py - 2 dy, 3 - px - 2 dx) (weights.vitpose_fold_head): every one of the sixteen taps
// belongs to exactly one (phase, 2x2 tap).
struct PhaseTap { int phase, tap; };
constexpr PhaseTap phase_of_tap(int ky, int kx) {
    return {2 * ((3 - ky) & 1) + ((3 - kx) & 1), 2 * ((3 - ky) >> 1) + ((3 - kx) >> 1)};
}
struct KernelTap { int ky, kx; };
constexpr KernelTap tap_of_phase(int phase, int tap) {
    return {3 - (phase >> 1) - 2 * (tap >> 1), 3 - (phase & 1) - 2 * (tap & 1)};
}
// The weight of (ci, co, ky, kx) in the reference's layout (cin, cout, 4, 4), in the forward's four phase matrices
// (4, cout, 4 cin) -- row co of phase p, reduction index t cin + ci -- and in the backward's matrix (cin, 16 cout) -- row ci,
// column (4 ky + kx) cout + co, the order gemm_modes.h's dgrad_index gathers in
constexpr size_t ref_index(int cin, int cout, int ci, int co, int ky, int kx) { return (((size_t)ci * cout + co) * 4 + ky) * 4 + kx; }
constexpr size_t phase_index(int cin, int cout, int ci, int co, int ky, int kx) {
    const PhaseTap p = phase_of_tap(ky, kx);
    return ((size_t)p.phase * cout + co) * 4 * cin + (size_t)p.tap * cin + ci;
}
constexpr size_t perm_index(int cin, int cout, int ci, int co, int ky, int kx) { return (size_t)ci * 16 * cout + (size_t)(4 * ky + kx) * cout + co; }
// ... and back: element e of the backward's matrix is which element of the reference's
constexpr size_t ref_of_perm(int cin, int cout, size_t e) {
    const int ci = (int)(e / ((size_t)16 * cout)), r = (int)(e - (size_t)ci * 16 * cout), t16 = r / cout, co = r - t16 * cout;
    return ref_index(cin, cout, ci, co, t16 >> 2, t16 & 3);
}

// ------------------------------------------------------------------ slices
// Every sum over rows -- the BN statistics, d gamma / d beta, dWf / dbf, and the k range of the dW products -- is cut at the same
// token boundaries: SLICE_TOKENS tokens a slice, i.e. SLICE_TOKENS << 2l rows at level l (0 the tokens, 1 deconvolution 1's
// pixels, 2 deconvolution 2's).  Slices are summed in slice order.
constexpr int SLICE_TOKENS = 512;
static_assert(SLICE_TOKENS % BK == 0, "a k-slice of the dW product is a whole number of GEMM k-tiles");
constexpr int slices(long long tokens) { return (int)((tokens + SLICE_TOKENS - 1) / SLICE_TOKENS); }
constexpr long long slice_rows(int level) { return (long long)SLICE_TOKENS << (2 * level); }
constexpr long long last_slice_rows(long long tokens, int level) { return ((tokens - 1) % SLICE_TOKENS + 1) << (2 * level); }
constexpr int DWF_SUB = 16;                                // dWf / dbf: a slice's pixels in sixteen consecutive parts, one workgroup each

// ------------------------------------------------------------------ refusals
struct Refusal {
    int rc = TTUP_OK;
    char msg[200] = "";
};
#define VH_PLAN_REQUIRE(cond, ...) do { if (!(cond)) { r.rc = TTUP_EINVAL; snprintf(r.msg, sizeof r.msg, __VA_ARGS__); return r; } } while (0)
inline Refusal check_create(int out_ch, long long max_rows) {
    Refusal r;
    VH_PLAN_REQUIRE(out_ch >= 1 && out_ch <= MAX_OUT, "ttup_vitpose_head_create: out_ch %d outside 1..%d", out_ch, MAX_OUT);
    VH_PLAN_REQUIRE(max_rows >= 1 && max_rows <= MAX_ROWS, "ttup_vitpose_head_create: max_rows %lld outside 1..%lld", max_rows, MAX_ROWS);
    return r;
}
inline Refusal check_forward(long long max_rows, int batch, int hp, int wp) {
    Refusal r;
    VH_PLAN_REQUIRE(batch >= 1 && hp >= 1 && wp >= 1, "ttup_vitpose_head_forward: batch %d and grid %dx%d must be positive", batch, hp, wp);
    VH_PLAN_REQUIRE((long long)batch * hp * wp <= max_rows && (long long)hp * wp <= max_rows, "ttup_vitpose_head_forward: %d x %dx%d rows, the handle was sized for %lld",
                    batch, hp, wp, max_rows);
    return r;
}
// kept: what the last forward ran on (batch 0: none)
inline Refusal check_backward(int kept_batch, int kept_hp, int kept_wp, int batch, int hp, int wp) {
    Refusal r;
    VH_PLAN_REQUIRE(kept_batch > 0, "ttup_vitpose_head_backward: no forward has run on this handle");
    VH_PLAN_REQUIRE(batch == kept_batch && hp == kept_hp && wp == kept_wp, "ttup_vitpose_head_backward: batch %d grid %dx%d, the forward ran batch %d grid %dx%d",
                    batch, hp, wp, kept_batch, kept_hp, kept_wp);
    return r;
}
#undef VH_PLAN_REQUIRE

// ------------------------------------------------------------------ the workspace
// One allocation per handle, for max_rows tokens (T): the kept activations (feat, z1, a1, z2, a2: 384 + 2 (4 + 16) 256 floats a
// token), the two gradient streams that become dz in place (d1, d2), the packed weights, the fp32 statistics and the partial sums.
enum Buf {
    B_FEAT, B_Z1, B_A1, B_Z2, B_A2, B_D1, B_D2,          // T x 384; 4T x 256 (z1, a1, d1); 16T x 256 (z2, a2, d2)
    B_WPH1, B_WPH2, B_WPERM1, B_WPERM2,                  // (4, 256, 4 cin) and (cin, 4096) of each deconvolution
    B_SMALL,                                             // a zero bias (DIM), gamma1, gamma2, wf and, per BN, mean / var / rstd / c1 / c2 (floats: SmallOff)
    B_SUMS,                                              // fp64: slices x 2 x 256 partial sums of one BN pass (forward or backward)
    B_DWF,                                               // fp64: slices x DWF_SUB x (out_ch x 256 + out_ch)
    B_PARTIAL,                                           // slices x 384 x 4096: the k-slices of a dW product
    B_COUNT
};
// float offsets inside B_SMALL
struct SmallOff { enum { ZERO = 0, G1 = 512, G2 = G1 + DEC, WF = G2 + DEC, BN1 = WF + MAX_OUT * DEC, BN2 = BN1 + 5 * DEC, COUNT = BN2 + 5 * DEC }; };
static_assert(SmallOff::G1 >= DIM && SmallOff::G1 % 4 == 0, "the zero bias serves every GEMM of the pass: N up to DIM");
enum { S_MEAN = 0, S_VAR = 1, S_RSTD = 2, S_C1 = 3, S_C2 = 4 };          // rows of 256 inside BN1 / BN2

struct Workspace {
    size_t off[B_COUNT] = {}, bytes[B_COUNT] = {};
    size_t total = 0;
};
constexpr size_t WS_ALIGN = 256;
inline Workspace plan_workspace(long long max_rows, int out_ch) {
    const size_t T = (size_t)max_rows, S = (size_t)slices(max_rows);
    Workspace w;
    auto take = [&](int b, size_t bytes) {
        w.bytes[b] = bytes;
        w.off[b] = (w.total + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN;
        w.total = w.off[b] + bytes;
    };
    take(B_FEAT, T * DIM * 4);
    take(B_Z1, T * 4 * DEC * 4); take(B_A1, T * 4 * DEC * 4);
    take(B_Z2, T * 16 * DEC * 4); take(B_A2, T * 16 * DEC * 4);
    take(B_D1, T * 4 * DEC * 4); take(B_D2, T * 16 * DEC * 4);
    take(B_WPH1, (size_t)16 * DEC * DIM * 4); take(B_WPH2, (size_t)16 * DEC * DEC * 4);
    take(B_WPERM1, (size_t)16 * DEC * DIM * 4); take(B_WPERM2, (size_t)16 * DEC * DEC * 4);
    take(B_SMALL, (size_t)SmallOff::COUNT * 4);
    take(B_SUMS, S * 2 * DEC * 8);
    take(B_DWF, S * DWF_SUB * ((size_t)out_ch * DEC + out_ch) * 8);
    take(B_PARTIAL, S * DIM * 16 * DEC * 4);
    return w;
}

}  // namespace vhead
}  // namespace ttup
