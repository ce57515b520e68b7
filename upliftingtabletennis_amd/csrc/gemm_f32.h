// The fp32 GEMM on the matrix pipe (v_mfma_f32_16x16x4_f32: fp32 operands, fp32 accumulation) shared by the ViTPose detector
// (csrc/vitpose.hip, which describes the tile and its A modes), the uplift transformer's training pass (csrc/uplift_grad.hip) and the
// ViTPose head's (csrc/vitpose_head_grad.hip: the A_DGRAD / O_DGRAD gather of a transposed convolution's backward, gemm_modes.h).
#pragma once
#include "common.h"
#include "gemm_modes.h"

namespace ttup {
namespace gemm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LDS_STRIDE = BK + 4;          // BM, BN, BK, the A modes and the epilogue flags: gemm_modes.h

// GUARD form (the uplift transformer's training pass, uplift_grad.hip): any M, N, K; either operand read by rows (k contiguous) or by
// columns (the row index contiguous: a transposed operand), leading dimensions of their own; the k range cut into slices of `kslice`
// (grid z), slice z writing its own partial product at out + z * M * ldo -- summed afterwards in slice order, so a reduction over
// tens of thousands of rows has a fixed tree and needs no atomics.
enum { O_ROWS = 0, O_COLS = 1, O_DGRAD = 2 };          // O_DGRAD (w only): the gather of gemm_modes.h's dgrad_index, read by columns

struct GemmArgs {
    const float* a;          // A_DENSE / A_LN: (M, K) row-major; A_PATCH: NCHW input; A_DECONV: NHWC input; A_PATCH_FRAMES: (n, 3, H, W);
                             // A_DGRAD: the NHWC (2ih, 2iw, cin) gradient the rows gather from
    const float* w;          // (N, K)
    const float* bias;       // (N)
    const float* ln_g;       // A_LN: (K) gain, bias
    const float* ln_b;
    const float* stats;      // A_LN: (M, 2) mean, rstd
    const float* res;        // E_RESID: (M, N), may alias out
    const float* pos;        // E_POS: (N_tok + 1, N)
    float* out;
    int M, N, K;
    int cin, ih, iw;         // A_PATCH: input channels and size; A_DECONV: input channels and (phase) grid h x w; A_DGRAD / O_DGRAD:
                             // channels of the gathered gradient and the grid h x w of the rows
    int ntok;                // tokens per sample (E_POS)
    int py, px;              // A_DECONV: output phase
    int flags;
    // GUARD form only
    int lda, ldw, ldo, ldr;  // leading dimensions of a, w, out, res
    const float* gate;       // E_GATE: (M, N) with leading dimension ldg; the result is kept where gate > 0, else 0 (ReLU backward)
    int ldg;
    int kslice;              // k range of one grid-z slice (multiple of BK)
};

__device__ __forceinline__ float gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// Row m of a deconvolution phase's GEMM is one pixel of the ih x iw input grid: sample b, row y, column x
struct Pixel { int b, y, x; };
__device__ __forceinline__ Pixel deconv_pixel(int m, int ih, int iw) {
    const int per = ih * iw, b = m / per, t = m - b * per, y = t / iw;
    return {b, y, t - y * iw};
}
// ... and phase (py, px) puts it at pixel (2y + py, 2x + px) of the 2ih x 2iw output: that pixel's index in the NHWC output
__device__ __forceinline__ size_t deconv_out_pixel(int m, int ih, int iw, int py, int px) {
    const Pixel q = deconv_pixel(m, ih, iw);
    return ((size_t)q.b * 2 * ih + 2 * q.y + py) * (2 * iw) + 2 * q.x + px;
}
// ... reading, at reduction index k = tap * cin + c, input pixel (y + py + tap / 2 - 1, x + px + tap % 2 - 1): that element's index in
// the NHWC input; false outside the grid
__device__ __forceinline__ bool deconv_in(const GemmArgs& p, int m, int k, size_t* e) {
    const Pixel q = deconv_pixel(m, p.ih, p.iw);
    const int tap = k / p.cin, c = k - tap * p.cin;
    const int iy = q.y + p.py + (tap >> 1) - 1, ix = q.x + p.px + (tap & 1) - 1;
    if (iy < 0 || iy >= p.ih || ix < 0 || ix >= p.iw) return false;
    *e = (((size_t)q.b * p.ih + iy) * p.iw + ix) * p.cin + c;
    return true;
}

// Four consecutive k of row m of A (k multiple of 4).
template <int AM>
__device__ __forceinline__ f32x4 load_a4(const GemmArgs& p, int m, int k) {
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (m >= p.M) return z;
    if (AM == A_DENSE || AM == A_LN) {
        f32x4 v = *(const f32x4*)(p.a + (size_t)m * p.K + k);
        if (AM == A_LN) {
            const float mu = p.stats[2 * m], rs = p.stats[2 * m + 1];
            const f32x4 g = *(const f32x4*)(p.ln_g + k), b = *(const f32x4*)(p.ln_b + k);
            v.x = (v.x - mu) * rs * g.x + b.x;
            v.y = (v.y - mu) * rs * g.y + b.y;
            v.z = (v.z - mu) * rs * g.z + b.z;
            v.w = (v.w - mu) * rs * g.w + b.w;
        }
        return v;
    } else if (AM == A_PATCH || AM == A_PATCH_FRAMES) {
        const int hp = p.ih >> 4, wp = p.iw >> 4, per = hp * wp;
        const int b = m / per, t = m - b * per, ty = t / wp, tx = t - ty * wp;
        const int c = k >> 8, ky = (k >> 4) & 15, kx = k & 15;
        // padding 2 (vit.py:222: 4 + 2 * (ratio // 2 - 1), ratio 1): a quad starts at x = 2 mod 4, so it is read as two float2,
        // each wholly on one side of a border (x even, W even)
        const int y = 16 * ty - 2 + ky, x = 16 * tx - 2 + kx;
        if (y < 0 || y >= p.ih) return z;
        const size_t plane = AM == A_PATCH ? (size_t)b * p.cin + c : (size_t)(b + c / 3) * 3 + c % 3;
        const float* r = p.a + (plane * p.ih + y) * p.iw;
        if (x >= 0 && x < p.iw) { const float2 u = *(const float2*)(r + x); z.x = u.x; z.y = u.y; }
        if (x + 2 >= 0 && x + 2 < p.iw) { const float2 u = *(const float2*)(r + x + 2); z.z = u.x; z.w = u.y; }
        return z;
    } else if (AM == A_DECONV) {
        size_t e;
        return deconv_in(p, m, k, &e) ? *(const f32x4*)(p.a + e) : z;
    } else {
        const long long e = dgrad_index(m, k, p.ih, p.iw, p.cin);          // a quad stays inside one tap's run of cin (cin multiple of 4)
        return e >= 0 ? *(const f32x4*)(p.a + e) : z;
    }
}

// GUARD form, operand read by rows: four consecutive k of row i, zero outside [0, rows) x [0, kend) (one 16-byte load when the
// quad lies inside and is aligned)
__device__ __forceinline__ f32x4 load_g4(const float* __restrict__ a, int ld, int i, int rows, int k, int kend) {
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (i >= rows || k >= kend) return z;
    const float* r = a + (size_t)i * ld + k;
    if (k + 3 < kend && ((size_t)r & 15) == 0) return *(const f32x4*)r;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k + e < kend) z[e] = r[e];
    return z;
}

// GUARD form, operand read by columns: rows i .. i+3 at one k (consecutive in memory: one 16-byte load when the row is aligned)
__device__ __forceinline__ f32x4 load_c4(const float* __restrict__ a, int ld, int i, int rows, int k, int kend) {
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (k >= kend || i >= rows) return z;
    const float* r = a + (size_t)k * ld + i;
    if (i + 3 < rows && ((size_t)r & 15) == 0) return *(const f32x4*)r;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (i + e < rows) z[e] = r[e];
    return z;
}

// GUARD form, w = the O_DGRAD gather read by columns: columns n .. n+3 (one tap, four consecutive channels: N and cin multiples of 4)
// of row k
__device__ __forceinline__ f32x4 load_d4(const GemmArgs& p, int n, int k, int kend) {
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (k >= kend || n >= p.N) return z;
    const long long e = dgrad_index(k, n, p.ih, p.iw, p.cin);
    return e >= 0 ? *(const f32x4*)(p.w + e) : z;
}

template <int AM, bool GUARD = false, int WM = O_ROWS>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs p) {
    __shared__ float sa[BM * LDS_STRIDE];
    __shared__ float sw[BN * LDS_STRIDE];
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const int m0 = ttup_bid_x() * BM, n0 = ttup_bid_y() * BN;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int lr = lane & 15, lg = lane >> 4;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // tile loads: 64 rows x 8 quads per operand, two passes of 32 rows
    const int lrow = tid >> 3, lq = (tid & 7) * 4;
    const int crow = (tid & 15) * 4, ck = tid >> 4;          // an operand read by columns: four consecutive rows at one k, two passes of 16 k
    f32x4 ra[2], rw[2];
    const int kbeg = GUARD ? ttup_bid_z() * p.kslice : 0;
    const int kend = GUARD ? (kbeg + p.kslice < p.K ? kbeg + p.kslice : p.K) : p.K;
    auto fetch = [&](int k0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (GUARD) {
                ra[h] = AM == O_ROWS ? load_g4(p.a, p.lda, m0 + lrow + 32 * h, p.M, k0 + lq, kend) : load_c4(p.a, p.lda, m0 + crow, p.M, k0 + ck + 16 * h, kend);
                rw[h] = WM == O_ROWS ? load_g4(p.w, p.ldw, n0 + lrow + 32 * h, p.N, k0 + lq, kend)
                      : WM == O_COLS ? load_c4(p.w, p.ldw, n0 + crow, p.N, k0 + ck + 16 * h, kend) : load_d4(p, n0 + crow, k0 + ck + 16 * h, kend);
            } else {
                ra[h] = load_a4<AM>(p, m0 + lrow + 32 * h, k0 + lq);
                rw[h] = *(const f32x4*)(p.w + (size_t)(n0 + lrow + 32 * h) * p.K + k0 + lq);
            }
        }
    };
    fetch(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (GUARD && AM == O_COLS) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sa[(crow + e) * LDS_STRIDE + ck + 16 * h] = ra[h][e];
            } else *(f32x4*)(sa + (lrow + 32 * h) * LDS_STRIDE + lq) = ra[h];
            if (GUARD && WM != O_ROWS) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sw[(crow + e) * LDS_STRIDE + ck + 16 * h] = rw[h][e];
            } else *(f32x4*)(sw + (lrow + 32 * h) * LDS_STRIDE + lq) = rw[h];
        }
        __syncthreads();
        if (k0 + BK < kend) fetch(k0 + BK);            // next tile in flight during this tile's MFMAs
#pragma unroll
        for (int s = 0; s < BK / 4; ++s) {
            float av[2], wv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = sa[(wm + 16 * i + lr) * LDS_STRIDE + 4 * s + lg];
#pragma unroll
            for (int j = 0; j < 2; ++j) wv[j] = sw[(wn + 16 * j + lr) * LDS_STRIDE + 4 * s + lg];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], wv[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // epilogue: lane holds C[wm + 16i + 4*lg + r][wn + 16j + lr]
    if (GUARD) {
        float* out = p.out + (size_t)ttup_bid_z() * p.M * p.ldo;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn + 16 * j + lr;
            if (n >= p.N) continue;
            const float bn = p.bias ? p.bias[n] : 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + wm + 16 * i + 4 * lg + r;
                    if (m >= p.M) continue;
                    float v = acc[i][j][r] + bn;
                    if (p.flags & E_RESID) v = p.res[(size_t)m * p.ldr + n] + v;
                    if (p.flags & E_RELU) v = fmaxf(v, 0.f);
                    if (p.flags & E_GATE) v = p.gate[(size_t)m * p.ldg + n] > 0.f ? v : 0.f;
                    out[(size_t)m * p.ldo + n] = v;
                }
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int n = n0 + wn + 16 * j + lr;
        const float bn = p.bias[n];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * i + 4 * lg + r;
                if (m >= p.M) continue;
                float v = acc[i][j][r] + bn;
                if (p.flags & E_POS) {
                    const int tok = m % p.ntok;
                    v = v + p.pos[(size_t)(1 + tok) * p.N + n] + p.pos[n];
                }
                if (p.flags & E_GELU) v = gelu(v);
                if (p.flags & E_RESID) v = p.res[(size_t)m * p.N + n] + v;
                if (p.flags & E_RELU) v = fmaxf(v, 0.f);
                const size_t orow = AM == A_DECONV ? deconv_out_pixel(m, p.ih, p.iw, p.py, p.px) : (size_t)m;
                p.out[orow * p.N + n] = v;
            }
        }
    }
}

}  // namespace gemm
}  // namespace ttup
