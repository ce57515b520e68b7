// The kernels of the ViTPose backbone's training pass beside the GEMMs (csrc/vitpose_grad.hip).  Everything is
// fp32; every sum over tokens is an fp64 partial per slice added in slice order; no atomics: every sum has one owner.
//   ln_stats_kernel          vitpose_kernels.h's statistics (the same arithmetic, so the same bits), kept per block.
//   ln_apply_kernel          an LN output materialised: last_norm in the forward, norm1 / norm2 recomputed in the backward.
//   attention_lse_kernel     vitpose_kernels.h's attention_kernel (the same arithmetic, so the same bits) that also writes
//                            lse = m + log(l) per (row, head).  A kernel of its own: the inference kernel keeps its device code.
//   attn_delta_kernel        D[row, head] = sum_d dO O, as the diagonal of dO O^T on the matrix pipe: the same chain of products
//                            as dP = dO V^T below, so that a row whose softmax has one entry (O = V) gives dP - D = 0 exactly.
//   attn_bwd_dkv_kernel      one workgroup per (key tile of 64, head, sample), 16 keys a wave, walking the query tiles in
//                            ascending order through LDS.  Scores are computed as S = Q K^T, so a lane holds 4 queries of ONE key:
//                            P = exp(S - lse) and dS = P (dP - D) in that layout are directly the B operands of
//                            dV^T += dO^T P and dK^T += (scale Q)^T dS (the k-order of the products is permuted, the sums are
//                            the same).  Accumulators in registers.
//   attn_bwd_dq_kernel       one workgroup per (query tile of 64, head, sample), 16 queries a wave, walking the key tiles in
//                            ascending order; scores transposed (S^T = K Q^T, the forward's layout): dQ^T += K^T dS^T.
//   scale_rows / scale_add   s[b] g and x + s[b] y with the sample's branch scale (stochastic depth).
//   gelu / gelu_bwd          exact-erf GELU of the kept pre-activation and its derivative.
//   ln_bwd_kernel            g (+)= rstd (gd - mean(gd) - xhat mean(gd xhat)), gd = gamma dy, one wave a row.
//   col_sums_kernel<LN>      per column and slice, in fp64: sum dy (bias gradients, dpos[0]) or, LN, (sum dy, sum dy xhat).
//   sums_finalize, dw_reduce, dpos_rows, im2col: the rest.
#pragma once
#include "common.h"
#include "gemm_f32.h"
#include "vitpose_grad_plan.h"
#include <math.h>

namespace ttup {
namespace vgrad {

using gemm::f32x4;
using gemm::GemmArgs;

// one wave per row of DIM floats -> (mean, 1/sqrt(var + 1e-6)), two-pass in registers
__global__ __launch_bounds__(256) void ln_stats_kernel(const float* __restrict__ x, int M, float* __restrict__ stats) {
    const int row = ttup_bid_x() * 4 + (ttup_tid_x() >> 6), lane = ttup_tid_x() & 63;
    if (row >= M) return;
    const float* r = x + (size_t)row * DIM;
    float v[DIM / 64];
    float s = 0;
#pragma unroll
    for (int i = 0; i < DIM / 64; ++i) { v[i] = r[lane + 64 * i]; s += v[i]; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    const float mu = s * (1.0f / DIM);
    float q = 0;
#pragma unroll
    for (int i = 0; i < DIM / 64; ++i) { const float d = v[i] - mu; q += d * d; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
    if (lane == 0) {
        stats[2 * row] = mu;
        stats[2 * row + 1] = 1.0f / sqrt(q * (1.0f / DIM) + 1e-6f);
    }
}

// out[m][k] = (x[m][k] - mean) * rstd * g[k] + b[k], one quad per thread (p.K = DIM)
__global__ __launch_bounds__(256) void ln_apply_kernel(GemmArgs p) {
    const long long e = (long long)ttup_bid_x() * 256 + ttup_tid_x();
    if (e >= (long long)p.M * (DIM / 4)) return;
    const int m = (int)(e / (DIM / 4)), k = (int)(e - (long long)m * (DIM / 4)) * 4;
    *(f32x4*)(p.out + (size_t)m * DIM + k) = gemm::load_a4<gemm::A_LN>(p, m, k);
}

// col[m][k] = the im2col of the patch embedding (p.a the NCHW images, p.cin, p.ih, p.iw, p.M, p.K = cin * 256), one quad per thread
__global__ __launch_bounds__(256) void im2col_kernel(GemmArgs p) {
    const long long e = (long long)ttup_bid_x() * 256 + ttup_tid_x();
    const int q = p.K / 4;
    if (e >= (long long)p.M * q) return;
    const int m = (int)(e / q), k = (int)(e - (long long)m * q) * 4;
    *(f32x4*)(p.out + (size_t)m * p.K + k) = gemm::load_a4<gemm::A_PATCH>(p, m, k);
}

// qkv: (B*N, 3*DIM) rows [q | k | v], each [head][32]; out: (B*N, DIM) [head][32]; lse: (B*N, HEADS).  grid (ceil(N/64), HEADS, B)
__global__ __launch_bounds__(256) void attention_lse_kernel(const float* __restrict__ qkv, int N, float scale, float* __restrict__ out,
                                                            float* __restrict__ lse) {
    __shared__ float sk[AKV * ASTR];
    __shared__ float sv[AKV * ASTR];
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const int head = ttup_bid_y(), b = ttup_bid_z();
    const int lr = lane & 15, lg = lane >> 4;
    const size_t row0 = (size_t)b * N;
    const int qi = ttup_bid_x() * AQ + wave * 16 + lr;            // this lane's query
    float q[HD / 4];
    {
        const bool ok = qi < N;
        const float* qr = qkv + (row0 + (ok ? qi : 0)) * (3 * DIM) + head * HD;
#pragma unroll
        for (int s = 0; s < HD / 4; ++s) q[s] = ok ? qr[4 * s + lg] * scale : 0.f;
    }
    f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float m_run = -INFINITY, l_run = 0.f;
    const int lrow = tid >> 3, lq = (tid & 7) * 4;
    for (int kv0 = 0; kv0 < N; kv0 += AKV) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int key = kv0 + lrow + 32 * h;
            f32x4 kk = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (key < N) {
                const float* kr = qkv + (row0 + key) * (3 * DIM) + DIM + head * HD + lq;
                kk = *(const f32x4*)kr;
                vv = *(const f32x4*)(kr + DIM);
            }
            *(f32x4*)(sk + (lrow + 32 * h) * ASTR + lq) = kk;
            *(f32x4*)(sv + (lrow + 32 * h) * ASTR + lq) = vv;
        }
        __syncthreads();
        f32x4 st[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            st[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < HD / 4; ++s)
                st[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(sk[(16 * t + lr) * ASTR + 4 * s + lg], q[s], st[t], 0, 0, 0);
        }
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (kv0 + 16 * t + 4 * lg + r >= N) st[t][r] = -INFINITY;
                mx = fmaxf(mx, st[t][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = expf(m_run - m_new);
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                st[t][r] = expf(st[t][r] - m_new);
                sum += st[t][r];
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        l_run = l_run * alpha + sum;
        m_run = m_new;
#pragma unroll
        for (int u = 0; u < 2; ++u) o[u] *= alpha;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    o[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(sv[(16 * t + 4 * lg + r) * ASTR + 16 * u + lr], st[t][r], o[u], 0, 0, 0);
        __syncthreads();
    }
    if (qi < N) {
        const float inv = 1.0f / l_run;
        float* orow = out + (row0 + qi) * DIM + head * HD;
#pragma unroll
        for (int u = 0; u < 2; ++u) *(f32x4*)(orow + 16 * u + 4 * lg) = o[u] * inv;
        if (lg == 0) lse[(row0 + qi) * HEADS + head] = m_run + logf(l_run);
    }
}

// D[row][head] = sum_d dO[row][head][d] O[row][head][d]: a wave takes 16 rows of one head, A = dO[row lr][d], B = O^T[d][row lr]; the
// diagonal of the 16 x 16 product (row i: lane lr = i, lg = i / 4, register i % 4).  grid (ceil(rows / 64), HEADS), 256 threads.
__global__ __launch_bounds__(256) void attn_delta_kernel(const float* __restrict__ dout, const float* __restrict__ out, long long rows,
                                                         float* __restrict__ delta) {
    const int lane = ttup_tid_x() & 63, wave = ttup_tid_x() >> 6, head = ttup_bid_y();
    const int lr = lane & 15, lg = lane >> 4;
    const long long row = (long long)ttup_bid_x() * 64 + wave * 16 + lr;
    const bool ok = row < rows;
    const size_t e = (size_t)(ok ? row : 0) * DIM + head * HD;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < HD / 4; ++s) {
        const float a = ok ? dout[e + 4 * s + lg] : 0.f, o = ok ? out[e + 4 * s + lg] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, o, acc, 0, 0, 0);
    }
    if (ok && (lr >> 2) == lg) delta[(size_t)row * HEADS + head] = acc[lr & 3];
}

// A query (key) tile of 64 rows x 32 of one head into LDS, row stride ASTR, rows >= N as zeros: column block `col` of the
// `ld`-float rows of src starting at sample row row0; scaled by `scale`.  256 threads: 64 rows x 8 quads, two passes of 32 rows.
__device__ __forceinline__ void load_tile(float* __restrict__ dst, const float* __restrict__ src, size_t row0, int r0, int N, int ld, int col, float scale,
                                          int tid) {
    const int lrow = tid >> 3, lq = (tid & 7) * 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int r = r0 + lrow + 32 * h;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (r < N) v = *(const f32x4*)(src + (row0 + r) * ld + col + lq) * scale;
        *(f32x4*)(dst + (lrow + 32 * h) * ASTR + lq) = v;
    }
}

// dK, dV of one key tile: qkv, dqkv (B*N, 3*DIM); dout (B*N, DIM): d att; lse, delta (B*N, HEADS).  grid (ceil(N/64), HEADS, B).
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
                                                           const float* __restrict__ delta, int N, float scale, float* __restrict__ dqkv) {
    __shared__ float sq[AQ * ASTR];          // scale * Q of the query tile
    __shared__ float sdo[AQ * ASTR];         // dO of the query tile
    __shared__ float sl[AQ], sd[AQ];         // its lse and D
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const int head = ttup_bid_y(), b = ttup_bid_z();
    const int lr = lane & 15, lg = lane >> 4;
    const size_t row0 = (size_t)b * N;
    const int ki = ttup_bid_x() * AKV + wave * 16 + lr;           // this lane's key
    // K^T and V^T as B operands: step s needs K[key lr][d = 4s + lg]
    float k[HD / 4], v[HD / 4];
    {
        const bool ok = ki < N;
        const float* kr = qkv + (row0 + (ok ? ki : 0)) * (3 * DIM) + DIM + head * HD;
#pragma unroll
        for (int s = 0; s < HD / 4; ++s) { k[s] = ok ? kr[4 * s + lg] : 0.f; v[s] = ok ? kr[DIM + 4 * s + lg] : 0.f; }
    }
    f32x4 dk[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, dv[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int q0 = 0; q0 < N; q0 += AQ) {
        load_tile(sq, qkv, row0, q0, N, 3 * DIM, head * HD, scale, tid);
        load_tile(sdo, dout, row0, q0, N, DIM, head * HD, 1.0f, tid);
        if (tid < AQ) {
            const bool ok = q0 + tid < N;
            sl[tid] = ok ? lse[(row0 + q0 + tid) * HEADS + head] : 0.f;
            sd[tid] = ok ? delta[(row0 + q0 + tid) * HEADS + head] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            // lane holds S[query q0 + 16t + 4lg + r][key lr] and dP likewise
            f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < HD / 4; ++s) {
                sc = __builtin_amdgcn_mfma_f32_16x16x4f32(sq[(16 * t + lr) * ASTR + 4 * s + lg], k[s], sc, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(sdo[(16 * t + lr) * ASTR + 4 * s + lg], v[s], dp, 0, 0, 0);
            }
            f32x4 p, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ql = 16 * t + 4 * lg + r;
                p[r] = (q0 + ql < N && ki < N) ? expf(sc[r] - sl[ql]) : 0.f;
                ds[r] = p[r] * (dp[r] - sd[ql]);
            }
            // dV^T[d = 16u + 4lg + r'][key lr] += sum_query dO^T[d][query] P[query][key]; k-step r takes query 16t + 4 * (lane / 16) + r
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    dv[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(sdo[(16 * t + 4 * lg + r) * ASTR + 16 * u + lr], p[r], dv[u], 0, 0, 0);
                    dk[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(sq[(16 * t + 4 * lg + r) * ASTR + 16 * u + lr], ds[r], dk[u], 0, 0, 0);
                }
        }
        __syncthreads();
    }
    if (ki < N) {
        float* kr = dqkv + (row0 + ki) * (3 * DIM) + DIM + head * HD;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            *(f32x4*)(kr + 16 * u + 4 * lg) = dk[u];
            *(f32x4*)(kr + DIM + 16 * u + 4 * lg) = dv[u];
        }
    }
}

// dQ of one query tile.  grid (ceil(N/64), HEADS, B), 256 threads.
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
                                                          const float* __restrict__ delta, int N, float scale, float* __restrict__ dqkv) {
    __shared__ float sk[AKV * ASTR];
    __shared__ float sv[AKV * ASTR];
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const int head = ttup_bid_y(), b = ttup_bid_z();
    const int lr = lane & 15, lg = lane >> 4;
    const size_t row0 = (size_t)b * N;
    const int qi = ttup_bid_x() * AQ + wave * 16 + lr;            // this lane's query
    const bool qok = qi < N;
    // (scale Q)^T and dO^T as B operands, the query's lse and D: zeros for a query past the end, never garbage
    float q[HD / 4], dO[HD / 4];
    {
        const float* qr = qkv + (row0 + (qok ? qi : 0)) * (3 * DIM) + head * HD;
        const float* dr = dout + (row0 + (qok ? qi : 0)) * DIM + head * HD;
#pragma unroll
        for (int s = 0; s < HD / 4; ++s) { q[s] = qok ? qr[4 * s + lg] * scale : 0.f; dO[s] = qok ? dr[4 * s + lg] : 0.f; }
    }
    const float l = qok ? lse[(row0 + qi) * HEADS + head] : 0.f, dl = qok ? delta[(row0 + qi) * HEADS + head] : 0.f;
    f32x4 dq[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int kv0 = 0; kv0 < N; kv0 += AKV) {
        load_tile(sk, qkv, row0, kv0, N, 3 * DIM, DIM + head * HD, 1.0f, tid);
        load_tile(sv, qkv, row0, kv0, N, 3 * DIM, 2 * DIM + head * HD, 1.0f, tid);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            // lane holds S^T[key kv0 + 16t + 4lg + r][query lr] (the forward's chain of products) and dP^T likewise
            f32x4 sc = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < HD / 4; ++s) {
                sc = __builtin_amdgcn_mfma_f32_16x16x4f32(sk[(16 * t + lr) * ASTR + 4 * s + lg], q[s], sc, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_16x16x4f32(sv[(16 * t + lr) * ASTR + 4 * s + lg], dO[s], dp, 0, 0, 0);
            }
            f32x4 ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = (qok && kv0 + 16 * t + 4 * lg + r < N) ? expf(sc[r] - l) : 0.f;
                ds[r] = p * (dp[r] - dl);
            }
            // dQ^T[d = 16u + 4lg + r'][query lr] += sum_key K^T[d][key] dS^T[key][query]; k-step r takes key 16t + 4 * (lane / 16) + r
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    dq[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(sk[(16 * t + 4 * lg + r) * ASTR + 16 * u + lr], ds[r], dq[u], 0, 0, 0);
        }
        __syncthreads();
    }
    if (qok) {
        float* qr = dqkv + (row0 + qi) * (3 * DIM) + head * HD;
#pragma unroll
        for (int u = 0; u < 2; ++u) *(f32x4*)(qr + 16 * u + 4 * lg) = dq[u] * scale;
    }
}

// ------------------------------------------------------------------ elementwise, one quad per thread
// s: the branch's scales (B), null: 1.  out = x + s[b] y (x non-null) or s[b] y; rows of DIM, sample b = row / ntok
__global__ void scale_add_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ s, int ntok, long long quads,
                                 float* __restrict__ out) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= quads) return;
    const float sc = s ? s[(i / (DIM / 4)) / ntok] : 1.0f;
    f32x4 v = *(const f32x4*)(y + i * 4);
    if (x) {
        const f32x4 r = *(const f32x4*)(x + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = r[e] + sc * v[e];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = sc * v[e];
    }
    *(f32x4*)(out + i * 4) = v;
}
__global__ void gelu_kernel(const float* __restrict__ pre, long long quads, float* __restrict__ out) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= quads) return;
    f32x4 v = *(const f32x4*)(pre + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = gemm::gelu(v[e]);
    *(f32x4*)(out + i * 4) = v;
}
// d *= gelu'(pre) = Phi(pre) + pre phi(pre)
__global__ void gelu_bwd_kernel(const float* __restrict__ pre, long long quads, float* __restrict__ d) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= quads) return;
    const f32x4 v = *(const f32x4*)(pre + i * 4);
    f32x4 g = *(const f32x4*)(d + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        g[e] *= 0.5f * (1.0f + erff(v[e] * 0.70710678118654752f)) + v[e] * 0.39894228040143268f * expf(-0.5f * v[e] * v[e]);
    *(f32x4*)(d + i * 4) = g;
}
__global__ void fill_kernel(float* __restrict__ p, int n, float v) {
    const int i = ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i < n) p[i] = v;
}

// ------------------------------------------------------------------ LayerNorm backward
// one wave per row: g[row] = (acc ? g[row] : 0) + rstd (gd - mean(gd) - xhat mean(gd xhat)), gd = gamma dy
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ stats, const float* __restrict__ dy,
                                                     const float* __restrict__ gamma, int M, int acc, float* __restrict__ g) {
    const int row = ttup_bid_x() * 4 + (ttup_tid_x() >> 6), lane = ttup_tid_x() & 63;
    if (row >= M) return;
    const size_t r0 = (size_t)row * DIM;
    const float mu = stats[2 * row], rs = stats[2 * row + 1];
    float xh[DIM / 64], gd[DIM / 64];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < DIM / 64; ++i) {
        const int c = lane + 64 * i;
        xh[i] = (x[r0 + c] - mu) * rs;
        gd[i] = gamma[c] * dy[r0 + c];
        s1 += gd[i]; s2 += gd[i] * xh[i];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { s1 += __shfl_xor(s1, off, 64); s2 += __shfl_xor(s2, off, 64); }
    const float m1 = s1 * (1.0f / DIM), m2 = s2 * (1.0f / DIM);
#pragma unroll
    for (int i = 0; i < DIM / 64; ++i) {
        const int c = lane + 64 * i;
        const float dx = rs * (gd[i] - m1 - xh[i] * m2);
        g[r0 + c] = acc ? g[r0 + c] + dx : dx;
    }
}

// ------------------------------------------------------------------ per-column sums over rows
// partial[slice][c] = the slice's sum of d[m][c] in fp64, or, LN, partial[slice][0][c], [1][c] = the sums of (dy, dy xhat) with
// xhat = (x - mean[m]) rstd[m].  Fixed order: wave w takes rows w, w + 16, ...; the sixteen waves are added 0..15.
// Grid (ncols / 64, slices), 1024 threads.
template <bool LN>
__global__ __launch_bounds__(1024) void col_sums_kernel(const float* __restrict__ d, const float* __restrict__ x, const float* __restrict__ stats, int ncols,
                                                        long long rows, long long per_slice, double* __restrict__ partial) {
    __shared__ double sm[2][16][64];
    const int lane = ttup_tid_x() & 63, wave = ttup_tid_x() >> 6;
    const int c = ttup_bid_x() * 64 + lane;
    const long long m0 = (long long)ttup_bid_y() * per_slice;
    const long long m1 = m0 + per_slice < rows ? m0 + per_slice : rows;
    double s0 = 0.0, s1 = 0.0;
    for (long long m = m0 + wave; m < m1; m += 16) {
        const size_t e = (size_t)m * ncols + c;
        const float dy = d[e];
        s0 += (double)dy;
        if (LN) s1 += (double)dy * (double)((x[e] - stats[2 * m]) * stats[2 * m + 1]);
    }
    sm[0][wave][lane] = s0; sm[1][wave][lane] = s1;
    __syncthreads();
    if (wave < (LN ? 2 : 1)) {
        double s = sm[wave][0][lane];
#pragma unroll
        for (int w = 1; w < 16; ++w) s += sm[wave][w][lane];
        partial[((size_t)ttup_bid_y() * (LN ? 2 : 1) + wave) * ncols + c] = s;
    }
}
// out0[c] (and, with out1, out1[c] from the second row of sums) = the slices added in order
__global__ void sums_finalize_kernel(const double* __restrict__ partial, int nslices, int ncols, float* __restrict__ out0, float* __restrict__ out1) {
    const int c = ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (c >= ncols) return;
    const int per = out1 ? 2 : 1;
    double s = 0.0, q = 0.0;
    for (int i = 0; i < nslices; ++i) {
        s += partial[((size_t)i * per) * ncols + c];
        if (out1) q += partial[((size_t)i * per + 1) * ncols + c];
    }
    out0[c] = (float)s;
    if (out1) out1[c] = (float)q;
}
// dw[e] = the k-slices of a dW product added in slice order
__global__ void dw_reduce_kernel(const float* __restrict__ partial, int nslices, long long n, float* __restrict__ dw) {
    const long long e = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (e >= n) return;
    float acc = partial[e];
    for (int s = 1; s < nslices; ++s) acc += partial[(size_t)s * n + e];
    dw[e] = acc;
}
// dpos[1 + t][c] = sum over samples, in order, of dx0[b][t][c]
__global__ void dpos_rows_kernel(const float* __restrict__ dx0, int batch, int ntok, float* __restrict__ dpos) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    const long long per = (long long)ntok * DIM;
    if (i >= per) return;
    float acc = dx0[i];
    for (int b = 1; b < batch; ++b) acc += dx0[(size_t)b * per + i];
    dpos[DIM + i] = acc;
}

}  // namespace vgrad
}  // namespace ttup
