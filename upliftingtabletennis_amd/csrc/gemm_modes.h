// What a host plan needs to know of the matrix-pipe GEMMs (csrc/gemm_f32.h, csrc/gemm_bf16.h): tile sizes, A modes and epilogue
// flags.  No includes: the same text compiles for gfx950 and in a host program (csrc/vitpose_plan.h).
#pragma once

namespace ttup {
namespace gemm {

constexpr int BM = 64, BN = 64, BK = 32;          // gemm_kernel / gemm_guard_kernel: fp32 operands

enum { A_DENSE = 0, A_LN = 1, A_PATCH = 2, A_DECONV = 3, A_PATCH_FRAMES = 4 };
enum { E_GELU = 1, E_RESID = 2, E_POS = 4, E_RELU = 8, E_GATE = 16 };

}  // namespace gemm
namespace gemm16 {

constexpr int TM = 128, TN = 128, TK = 32;        // gemm_bf16_kernel

}  // namespace gemm16
}  // namespace ttup
