// Kernels of the ViTPose detector beside the GEMMs (csrc/gemm_f32.h, csrc/gemm_bf16.h), for both of its paths; included by
// vitpose.hip.  The bf16 path's arithmetic contract is DESIGN.md §24.
//   ln_stats_kernel<T>      one wave per token: mean and 1/sqrt(var + 1e-6) of 384 values (two-pass, in registers), in fp32 for the fp32
//                           path and in fp64 for the bf16 path's LN prologues.
//   attention_kernel        flash-style, 32-dim heads, 64 queries per workgroup (16 per wave), K/V tiles of 64 keys through LDS,
//                           online softmax; scores are computed transposed (S^T = K Q^T) so that a lane holds 16 keys of ONE query:
//                           the row max / sum is 15 in-lane ops + 2 cross-lane steps, and P^T in that layout is directly the B
//                           operand of O^T += V^T P^T (the k-order of the product is permuted, the sum is the same).  No N x N matrix.
//   attention_bf16_kernel   flash-style like attention_kernel: 64 queries per workgroup (16 per wave), K/V tiles of 64 keys through
//                           LDS, fp32 online softmax, transposed scores.  Head dim 32 is one v_mfma_f32_16x16x32_bf16 per 16 x 16
//                           score tile: S^T = K Q^T with K rows from the GEMM's LDS image (ds_read_b128) and the query's row chunk
//                           in registers; scores are scaled by 1/sqrt(32) in fp32 afterwards.  P^T is directly the B operand of
//                           O^T += V^T P^T: an MFMA k-step of 32 keys takes, from lane group g, the keys 4g..4g+3 of its two score
//                           tiles (a permutation of k applied to both operands), and V lies transposed in LDS ([d][key], row stride
//                           72 bf16: the two ds_read_b64 per operand are conflict-free).  p enters as TWO bf16 operands, its bf16
//                           rounding and the rounded remainder (16 significant bits; two MFMAs on the same V fragment): with one,
//                           p's rounding (up to 2^-8 of each p, bf16's unit round-off) and the output's own storage together
//                           exceed 2^-9 (sum_j p_j |v_j| / l + |att|) on short rows.  The row sum l is accumulated from the
//                           unrounded p.
//   ln_apply_kernel         last_norm applied once, fp32.
//   ln_apply_bf16_kernel    the same in fp64 (as the prologues), rounded to bf16.
//   conv1x1_kernel<TIn>     the final 1x1 conv (256 -> C_out, + bias) from NHWC to the NCHW heatmap, 64 pixels per workgroup staged in
//                           LDS.  It is not fused into deconv 2: a deconv tile holds 64 of the 256 channels the 1x1 reduces over.
//                           TIn: the stored deconv output, fp32 or bf16; the arithmetic is fp32 on either.
#pragma once
#include "gemm_bf16.h"
#include "vitpose_plan.h"

namespace ttup {
namespace vit {

using namespace ttup::gemm16;

// one wave per row of DIM floats -> (mean, 1/sqrt(var + eps)) in T, eps 1e-6 (vit.py:274)
template <class T>
__global__ __launch_bounds__(256) void ln_stats_kernel(const float* __restrict__ x, int M, T* __restrict__ stats) {
    const int row = ttup_bid_x() * 4 + (ttup_tid_x() >> 6), lane = ttup_tid_x() & 63;
    if (row >= M) return;
    const float* r = x + (size_t)row * DIM;
    T v[DIM / 64];
    T s = 0;
#pragma unroll
    for (int i = 0; i < DIM / 64; ++i) { v[i] = (T)r[lane + 64 * i]; s += v[i]; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    const T mu = s * (T(1) / DIM);
    T q = 0;
#pragma unroll
    for (int i = 0; i < DIM / 64; ++i) { const T d = v[i] - mu; q += d * d; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
    if (lane == 0) {
        stats[2 * row] = mu;
        stats[2 * row + 1] = T(1) / sqrt(q * (T(1) / DIM) + T(1e-6));
    }
}

constexpr int AQ = 64, AKV = 64, ASTR = HD + 4;

// qkv: (B*N, 3*DIM) rows [q | k | v], each [head][32]; out: (B*N, DIM) [head][32].  grid (ceil(N/64), HEADS, B), 256 threads.
__global__ __launch_bounds__(256) void attention_kernel(const float* __restrict__ qkv, int N, float scale, float* __restrict__ out) {
    __shared__ float sk[AKV * ASTR];
    __shared__ float sv[AKV * ASTR];
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const int head = ttup_bid_y(), b = ttup_bid_z();
    const int lr = lane & 15, lg = lane >> 4;
    const size_t row0 = (size_t)b * N;
    const int qi = ttup_bid_x() * AQ + wave * 16 + lr;            // this lane's query
    // Q^T as the B operand of S^T = K Q^T: step s needs Q[query lr][d = 4s + lg]
    float q[HD / 4];
    {
        const bool ok = qi < N;
        const float* qr = qkv + (row0 + (ok ? qi : 0)) * (3 * DIM) + head * HD;
#pragma unroll
        for (int s = 0; s < HD / 4; ++s) q[s] = ok ? qr[4 * s + lg] * scale : 0.f;
    }
    f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float m_run = -INFINITY, l_run = 0.f;
    const int lrow = tid >> 3, lq = (tid & 7) * 4;                // K/V tile load: 64 keys x 8 quads, two passes of 32 keys
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
        // S^T tile t: lane holds S^T[key kv0 + 16t + 4lg + r][query lr]
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
        const float m_new = fmaxf(m_run, mx);                 // finite: every tile holds at least one key < N
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
        // O^T[d = 16u + 4lg + r][query lr] += sum_key V^T[d][key] P^T[key][query]; k-step (t, r) takes key 16t + 4*(lane/16) + r
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
    }
}

constexpr int VSTR = 72;

// qkv: (B*N, 3*DIM) bf16 rows [q | k | v], each [head][32]; out: (B*N, DIM) bf16 [head][32].  grid (ceil(N/64), HEADS, B), 256 threads.
__global__ __launch_bounds__(256) void attention_bf16_kernel(const bf16_t* __restrict__ qkv, int N, float scale, bf16_t* __restrict__ out) {
    __shared__ u32x4 sk[64 * 4];
    __shared__ __attribute__((aligned(16))) bf16_t svt[HD * VSTR];
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const int head = ttup_bid_y(), b = ttup_bid_z();
    const int lr = lane & 15, lg = lane >> 4;
    const size_t row0 = (size_t)b * N;
    const int qi = ttup_bid_x() * 64 + wave * 16 + lr;            // this lane's query
    // Q^T as the B operand of S^T = K Q^T: Q[query lr][d = 8lg + j]
    u32x4 qf = {0u, 0u, 0u, 0u};
    if (qi < N) qf = *(const u32x4*)(qkv + (row0 + qi) * (3 * DIM) + head * HD + 8 * lg);
    f32x4 o[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float m_run = -INFINITY, l_run = 0.f;
    const int lrow = tid >> 2, lc = tid & 3;                      // K/V tile load: 64 keys x 4 chunks of 8
    const int fu = lds_unit(lr, lg);
    for (int kv0 = 0; kv0 < N; kv0 += 64) {
        {
            const int key = kv0 + lrow;
            u32x4 kk = {0u, 0u, 0u, 0u}, vv = {0u, 0u, 0u, 0u};
            if (key < N) {
                const bf16_t* kr = qkv + (row0 + key) * (3 * DIM) + DIM + head * HD + 8 * lc;
                kk = *(const u32x4*)kr;
                vv = *(const u32x4*)(kr + DIM);
            }
            sk[lds_unit(lrow, lc)] = kk;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                svt[(8 * lc + 2 * e) * VSTR + lrow] = (bf16_t)(vv[e] & 0xffffu);
                svt[(8 * lc + 2 * e + 1) * VSTR + lrow] = (bf16_t)(vv[e] >> 16);
            }
        }
        __syncthreads();
        // S^T tile t: lane holds S^T[key kv0 + 16t + 4lg + r][query lr]
        f32x4 st[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
            st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, sk[16 * t * 4 + fu]), __builtin_bit_cast(bf16x8, qf),
                                                            (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                st[t][r] = kv0 + 16 * t + 4 * lg + r >= N ? -INFINITY : st[t][r] * scale;
                mx = fmaxf(mx, st[t][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);                 // finite: every tile holds at least one key < N
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
        // O^T[d = 16u + 4lg + r][query lr] += sum_key V^T[d][key] P^T[key][query]; k-slot (lane group g, j) of step s is key
        // 32s + 4g + j (j < 4) or 32s + 16 + 4g + j - 4: the keys whose p this lane holds in score tiles 2s and 2s + 1
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const u32x4 pb = pack8(st[2 * s], st[2 * s + 1]);
            f32x4 rem[2];                       // p - bf16(p): exact in fp32
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned w = pb[2 * h + (r >> 1)];
                    rem[h][r] = st[2 * s + h][r] - bf16_to_f32((bf16_t)((r & 1) ? w >> 16 : w & 0xffffu));
                }
            const u32x4 pl = pack8(rem[0], rem[1]);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const bf16_t* vr = svt + (16 * u + lr) * VSTR + 32 * s + 4 * lg;
                const u32x2 lo = *(const u32x2*)vr, hi = *(const u32x2*)(vr + 16);
                const bf16x8 vf = __builtin_bit_cast(bf16x8, (u32x4){lo.x, lo.y, hi.x, hi.y});
                o[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, __builtin_bit_cast(bf16x8, pb), o[u], 0, 0, 0);
                o[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, __builtin_bit_cast(bf16x8, pl), o[u], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (qi < N) {
        const float inv = 1.0f / l_run;
        bf16_t* orow = out + (row0 + qi) * DIM + head * HD;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f32x4 v = o[u] * inv;
            *(u32x2*)(orow + 16 * u + 4 * lg) = u32x2{pack2(v.x, v.y), pack2(v.z, v.w)};
        }
    }
}

// last_norm applied once: out[m][k] = (x[m][k] - mean) * rstd * g[k] + b[k], one quad per thread
__global__ __launch_bounds__(256) void ln_apply_kernel(GemmArgs p) {
    const long long e = (long long)ttup_bid_x() * 256 + ttup_tid_x();
    if (e >= (long long)p.M * (DIM / 4)) return;
    const int m = (int)(e / (DIM / 4)), k = (int)(e - (long long)m * (DIM / 4)) * 4;
    *(f32x4*)(p.out + (size_t)m * DIM + k) = load_a4<A_LN>(p, m, k);
}

// last_norm applied once: out16[m][k] = bf16((x[m][k] - mean) * rstd * g[k] + b[k]) evaluated in fp64, eight values per thread
__global__ __launch_bounds__(256) void ln_apply_bf16_kernel(GemmArgs p, const double* __restrict__ stats64, bf16_t* __restrict__ out16) {
    const long long e = (long long)ttup_bid_x() * 256 + ttup_tid_x();
    if (e >= (long long)p.M * (DIM / 8)) return;
    const int m = (int)(e / (DIM / 8)), k = (int)(e - (long long)m * (DIM / 8)) * 8;
    *(u32x4*)(out16 + (size_t)m * DIM + k) = pack8(load_ln4(p, stats64, m, k), load_ln4(p, stats64, m, k + 4));
}

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(bf16_t v) { return bf16_to_f32(v); }

// x: NHWC (B, H, W, DEC) fp32 or bf16 -> heat (B, cout, H, W) fp32 = w (cout, DEC) x + bias in fp32 arithmetic; 64 pixels per workgroup
template <class TIn>
__global__ __launch_bounds__(256) void conv1x1_kernel(const TIn* __restrict__ x, long long npix, int hw, const float* __restrict__ w,
                                                      const float* __restrict__ bias, int cout, float* __restrict__ heat) {
    __shared__ float sx[64 * (64 + 1)];
    const int tid = ttup_tid_x();
    const long long p0 = (long long)ttup_bid_x() * 64;
    const int pl = tid & 63, cg = tid >> 6;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};          // output channels cg, cg+4, cg+8, cg+12
    for (int c0 = 0; c0 < DEC; c0 += 64) {
        for (int e = tid; e < 64 * 64; e += 256) {
            const int pp = e >> 6, c = e & 63;
            sx[pp * 65 + c] = p0 + pp < npix ? to_f32(x[(size_t)(p0 + pp) * DEC + c0 + c]) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = cg + 4 * j;
            if (co < cout)
                for (int c = 0; c < 64; ++c) acc[j] += sx[pl * 65 + c] * w[co * DEC + c0 + c];
        }
        __syncthreads();
    }
    const long long pix = p0 + pl;
    if (pix >= npix) return;
    const long long b = pix / hw, t = pix - b * hw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int co = cg + 4 * j;
        if (co < cout) heat[((size_t)b * cout + co) * hw + t] = acc[j] + bias[co];
    }
}

}  // namespace vit
}  // namespace ttup
