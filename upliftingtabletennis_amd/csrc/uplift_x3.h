// Building blocks of the uplift transformer's split-bf16 kernels (csrc/uplift_linear.h, uplift_blocks.h, uplift_stage.h), K = 128 features per token.
// The arithmetic (that of csrc/conv_x3.hip): every fp32 weight and every (LayerNorm'd) activation is split exactly into three bf16
// parts, a product is the sum of six exact partial products (smallest first) accumulated in fp32 -- accurate to below one fp32 fma
// rounding, at 2.7x the peak rate of v_mfma_f32_16x16x4_f32.
// LDS image of a token tile: three planes [rows][128] bf16 (256-byte rows), the 16-byte chunk index XOR-swizzled with the row's low
// four bits: the 16 lanes of a ds_read_b128 group (8 tokens of one k chunk, 8 of the next) fall on 16 different chunks.
// Everything here is forced inline.
#pragma once
#include "common.h"

namespace ttup {
namespace upl {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int X3_K = 128;          // features per token row: the pitch of every tile below
namespace x3 {
// (weight part, activation part) of the six partial products, smallest first
constexpr int PA[6] = {0, 1, 2, 0, 1, 0}, PB[6] = {2, 1, 0, 1, 0, 0};
}  // namespace x3

// sum over the 16 lanes of a DPP row (every lane gets it): rotations by 8, 4, 2, 1 -- the same pairings, hence bit for bit the same
// value, as the xor butterfly of __shfl_xor, without its four trips through the LDS crossbar
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));
    return v;
}
// workgroup barrier that orders LDS traffic only: global loads issued before it stay in flight (a __syncthreads() drains vmcnt too)
__device__ __forceinline__ void stage_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ unsigned ux3_pack2(float a, float b) { return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2)); }
__device__ __forceinline__ f32x4 relu4(f32x4 v) { return f32x4{v[0] > 0.f ? v[0] : 0.f, v[1] > 0.f ? v[1] : 0.f, v[2] > 0.f ? v[2] : 0.f, v[3] > 0.f ? v[3] : 0.f}; }

// features 8 chunk .. 8 chunk + 7 of token row r (lo, hi) -> their three bf16 parts, into the three planes (PLANE elements apart)
template <int PLANE>
__device__ __forceinline__ void x3_split_store(uint16_t* planes, int r, int chunk, const f32x4& lo, const f32x4& hi) {
    u32x4 p0, p1, p2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float x0 = j < 2 ? lo[2 * j] : hi[2 * (j - 2)], x1 = j < 2 ? lo[2 * j + 1] : hi[2 * (j - 2) + 1];
        const unsigned q0 = ux3_pack2(x0, x1);
        const float r0 = x0 - __uint_as_float(q0 << 16), r1 = x1 - __uint_as_float(q0 & 0xffff0000u);
        const unsigned q1 = ux3_pack2(r0, r1);
        const float s0 = r0 - __uint_as_float(q1 << 16), s1 = r1 - __uint_as_float(q1 & 0xffff0000u);
        p0[j] = q0; p1[j] = q1; p2[j] = ux3_pack2(s0, s1);
    }
    uint16_t* d = planes + r * X3_K + ((chunk ^ (r & 15)) << 3);
    *(u32x4*)d = p0; *(u32x4*)(d + PLANE) = p1; *(u32x4*)(d + 2 * PLANE) = p2;
}
// feature n of row r in an fp32 staging tile [rows][128]: 16-byte chunks XOR-swizzled with the row's low four bits (512-byte rows
// alias on the banks: the swizzle spreads the 8 rows of a ds_write_b128 lane group over 8 chunks)
__device__ __forceinline__ float* x3_f32(float* b, int r, int n) { return b + r * X3_K + ((((n >> 2) ^ (r & 15))) << 2) + (n & 3); }

// the weight tile requested one GEMM ahead (wnext) becomes the current one (wc): KS k-steps x 3 parts, 16 bytes per lane each
template <int KS>
__device__ __forceinline__ void x3_take(bf16x8 (&wc)[3][KS], const bf16x8 (&wnext)[3][KS]) {
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int p = 0; p < 3; ++p) wc[p][s] = wnext[p][s];
}

// acc[mt] += W_tile . planes  (64 tokens x 16 outputs x 128 inputs, six partial products smallest first): rows 16 mt .. 16 mt + 15
// of the planes against the wave's weight tile; lane (q, c) = (lane >> 4, lane & 15) ends with outputs 4q .. 4q + 3 of row 16 mt + c
template <int PLANE, int KS>
__device__ __forceinline__ void x3_gemm64(const uint16_t* planes, int c, int q, const bf16x8 (&w)[3][KS], f32x4 (&acc)[4]) {
    const uint16_t* xw = planes + c * X3_K;          // (row & 15) == c: the swizzle term is the lane's own c
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        bf16x8 xb[3][4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int p = 0; p < 3; ++p) xb[p][mt] = *(const bf16x8*)(xw + p * PLANE + mt * 16 * X3_K + (((4 * s + q) ^ c) << 3));
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[x3::PA[j]][s], xb[x3::PB[j]][mt], acc[mt], 0, 0, 0);
    }
}

}  // namespace upl
}  // namespace ttup
