// What a host plan needs to know of the matrix-pipe GEMMs (csrc/gemm_f32.h, csrc/gemm_bf16.h): tile sizes, A modes and epilogue
// flags.  No includes: the same text compiles for gfx950 and in a host program (csrc/vitpose_plan.h).
#pragma once

namespace ttup {
namespace gemm {

constexpr int BM = 64, BN = 64, BK = 32;          // gemm_kernel / gemm_guard_kernel: fp32 operands

enum { A_DENSE = 0, A_LN = 1, A_PATCH = 2, A_DECONV = 3, A_PATCH_FRAMES = 4, A_DGRAD = 5 };
enum { E_GELU = 1, E_RESID = 2, E_POS = 4, E_RELU = 8, E_GATE = 16 };

// A_DGRAD (and the guarded form's O_DGRAD): the one gather operand of both backward products of ConvTranspose2d(k4, s2, p1)
// (csrc/vitpose_head_grad.hip).  Row m is pixel (b, y, x) of the ih x iw input grid, column k = (4 ky + kx) * c + co reads
// dz[b, 2y - 1 + ky, 2x - 1 + kx, co] of the NHWC (2ih, 2iw, c) gradient: that element's index, -1 outside the map.
constexpr long long dgrad_index(long long m, int k, int ih, int iw, int c) {
    const long long per = (long long)ih * iw, b = m / per, t = m - b * per;
    const int y = (int)(t / iw), x = (int)(t - (long long)y * iw), tap = k / c, co = k - tap * c;
    const int oy = 2 * y - 1 + (tap >> 2), ox = 2 * x - 1 + (tap & 3);
    if (oy < 0 || oy >= 2 * ih || ox < 0 || ox >= 2 * iw) return -1;
    return ((b * 2 * ih + oy) * (2 * iw) + ox) * c + co;
}

}  // namespace gemm
namespace gemm16 {

constexpr int TM = 128, TN = 128, TK = 32;        // gemm_bf16_kernel

}  // namespace gemm16
}  // namespace ttup
