// The bf16 GEMM of the ViTPose detector's bf16 path (csrc/vitpose.hip) on v_mfma_f32_16x16x32_bf16: bf16 operands, fp32
// accumulation.  C[m][n] = epilogue(sum_k A[m][k] W[n][k]) with the A modes and epilogues of gemm_f32.h (whose GemmArgs it takes):
//   A_PATCH / A_PATCH_FRAMES          read fp32 (gemm::load_a4) and round to bf16 (RNE) on the way into LDS: the GEMM prologue;
//   A_LN                              the same through LayerNorm evaluated in fp64 (row mean / rstd as doubles from ln_stats_kernel<double>),
//                                     rounded to fp32 and then to bf16: the operand is stored nowhere, so it has to be THE bf16
//                                     neighbour of the exact value -- an fp32 LayerNorm lands on the other side of a rounding tie
//                                     once in a few thousand operands, which moves a whole output row by ulp(operand) |W|
//                                     (measured: up to 23 bf16 ulps of qkv);
//   A_DENSE / A_DECONV                read stored bf16 activations (a16);
//   W                                 bf16, rounded once at handle creation (w16);
//   output                            fp32 (g.out) or rounded to bf16 (out16), after bias and the epilogue.
// Tile (gemm_modes.h): TM x TN = 128 x 128 per workgroup, TK = 32 per step, 4 waves of 64 x 64 (4 x 4 MFMA tiles).  The product is computed
// transposed (W rows in the MFMA's A slot, activation rows in its B slot), so a lane ends with four consecutive n of one row m: one
// 8- or 16-byte store, one 16-byte bias / residual / pos_embed load.  An output element's sum runs over k in steps of 32 in the
// MFMA's own order, whatever M is: batch composition is bit-neutral.
// LDS image: a tile row is 32 bf16 = four 16-byte chunks; chunk c of row r lies at 16-byte unit 4r + (c ^ ((-(r >> 2)) & 3)).
// ds_read_b128 serves a wave in four groups of 16 lanes ({0-3, 12-15, 20-27}, ...: MI355X_MICROARCH §LDS): a group takes rows
// {0-3, 12-15} at chunk c and rows {4-11} at chunk c ^ 1, and with this XOR the sixteen units are distinct mod 16 -- the operand
// reads are conflict-free without padding.  Two LDS buffers: step k + 1 is fetched into registers during step k's MFMAs and
// stored into the other buffer, one barrier per step.
#pragma once
#include "gemm_f32.h"

namespace ttup {
namespace gemm16 {

using namespace ttup::gemm;

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

struct Gemm16Args {
    GemmArgs g;              // shapes, fp32 operands and epilogue terms as in gemm_f32.h; g.w is not read
    const bf16_t* a16;       // A_DENSE: (M, K) row-major; A_DECONV: NHWC input
    const bf16_t* w16;       // (N, K)
    bf16_t* out16;           // when set the result is rounded to bf16 and goes here; otherwise fp32 to g.out
    const double* stats64;   // A_LN: (M, 2) mean, rstd in fp64 (g.stats is not read)
};

// two fp32 -> one dword of two bf16 (RNE; the first in the low half, i.e. at the lower address)
__device__ __forceinline__ unsigned pack2(float a, float b) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
__device__ __forceinline__ u32x4 pack8(f32x4 lo, f32x4 hi) {
    return u32x4{pack2(lo.x, lo.y), pack2(lo.z, lo.w), pack2(hi.x, hi.y), pack2(hi.z, hi.w)};
}
// 16-byte unit of chunk c of tile row r
__device__ __forceinline__ int lds_unit(int r, int c) { return 4 * r + (c ^ ((-(r >> 2)) & 3)); }

// Four consecutive k of row m through LayerNorm in fp64, rounded to fp32
__device__ __forceinline__ f32x4 load_ln4(const GemmArgs& g, const double* __restrict__ stats64, int m, int k) {
    const f32x4 v = *(const f32x4*)(g.a + (size_t)m * g.K + k), w = *(const f32x4*)(g.ln_g + k), b = *(const f32x4*)(g.ln_b + k);
    const double mu = stats64[2 * m], rs = stats64[2 * m + 1];
    f32x4 o;
    o.x = (float)(((double)v.x - mu) * rs * (double)w.x + (double)b.x);
    o.y = (float)(((double)v.y - mu) * rs * (double)w.y + (double)b.y);
    o.z = (float)(((double)v.z - mu) * rs * (double)w.z + (double)b.z);
    o.w = (float)(((double)v.w - mu) * rs * (double)w.w + (double)b.w);
    return o;
}

// Eight consecutive k of row m of A as bf16 (k multiple of 8)
template <int AM>
__device__ __forceinline__ u32x4 load_a8(const Gemm16Args& p, int m, int k) {
    const GemmArgs& g = p.g;
    const u32x4 z = {0u, 0u, 0u, 0u};
    if (AM == A_DENSE) {
        if (m >= g.M) return z;
        return *(const u32x4*)(p.a16 + (size_t)m * g.K + k);
    } else if (AM == A_DECONV) {
        size_t e;
        return m < g.M && deconv_in(g, m, k, &e) ? *(const u32x4*)(p.a16 + e) : z;
    } else if (AM == A_LN) {
        if (m >= g.M) return z;
        return pack8(load_ln4(g, p.stats64, m, k), load_ln4(g, p.stats64, m, k + 4));
    } else {
        return pack8(load_a4<AM>(g, m, k), load_a4<AM>(g, m, k + 4));
    }
}

template <int AM>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(Gemm16Args p) {
    __shared__ u32x4 sa[2][TM * 4];
    __shared__ u32x4 sw[2][TN * 4];
    const GemmArgs& g = p.g;
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const int m0 = ttup_bid_x() * TM, n0 = ttup_bid_y() * TN;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int lr = lane & 15, lg = lane >> 4;
    f32x4 acc[4][4];                                    // [n tile j][m tile i]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // tile loads: 128 rows x 4 chunks per operand, two passes of 64 rows (rows r and r + 64 share their XOR term)
    const int lrow = tid >> 2, lc = tid & 3;
    const int lu = lds_unit(lrow, lc);
    u32x4 ra[2], rw[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            ra[h] = load_a8<AM>(p, m0 + lrow + 64 * h, k0 + 8 * lc);
            rw[h] = *(const u32x4*)(p.w16 + (size_t)(n0 + lrow + 64 * h) * g.K + k0 + 8 * lc);
        }
    };
    auto stash = [&](int b) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            sa[b][lu + 256 * h] = ra[h];
            sw[b][lu + 256 * h] = rw[h];
        }
    };
    fetch(0);
    stash(0);
    __syncthreads();
    const int fu = lds_unit(lr, lg);                    // the lane's operand chunk in a 16-row block (blocks start at multiples of 16)
    int b = 0;
    for (int k0 = 0; k0 < g.K; k0 += TK, b ^= 1) {
        const bool more = k0 + TK < g.K;
        if (more) fetch(k0 + TK);                       // next tile in flight during this tile's MFMAs
        bf16x8 av[4], wv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) av[i] = __builtin_bit_cast(bf16x8, sa[b][(wm + 16 * i) * 4 + fu]);
#pragma unroll
        for (int j = 0; j < 4; ++j) wv[j] = __builtin_bit_cast(bf16x8, sw[b][(wn + 16 * j) * 4 + fu]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[j], av[i], acc[j][i], 0, 0, 0);
        if (more) stash(b ^ 1);                         // the buffer every wave finished reading before the last barrier
        __syncthreads();
    }
    // epilogue: lane holds C[m0 + wm + 16i + lr][n0 + wn + 16j + 4lg + (0..3)]
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + wm + 16 * i + lr;
        if (m >= g.M) continue;
        const size_t orow = (AM == A_DECONV ? deconv_out_pixel(m, g.ih, g.iw, g.py, g.px) : (size_t)m) * g.N;
        const int tok = (g.flags & E_POS) ? m % g.ntok : 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn + 16 * j + 4 * lg;
            f32x4 v = acc[j][i] + *(const f32x4*)(g.bias + n);
            if (g.flags & E_POS) v = v + *(const f32x4*)(g.pos + (size_t)(1 + tok) * g.N + n) + *(const f32x4*)(g.pos + n);
            if (g.flags & E_GELU) { v.x = gelu(v.x); v.y = gelu(v.y); v.z = gelu(v.z); v.w = gelu(v.w); }
            if (g.flags & E_RESID) v = *(const f32x4*)(g.res + (size_t)m * g.N + n) + v;
            if (g.flags & E_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            if (p.out16) *(u32x2*)(p.out16 + orow + n) = u32x2{pack2(v.x, v.y), pack2(v.z, v.w)};
            else *(f32x4*)(g.out + orow + n) = v;
        }
    }
}

}  // namespace gemm16
}  // namespace ttup
