// The small kernels of the uplift gradient pass (csrc/uplift_grad.hip): the sliced reductions behind dW / db, LayerNorm forward and
// backward, ReLU, the transposes of the token plumbing (csrc/uplift_tokens.h), the mask sum and the loss.
#pragma once
#include "common.h"
#include "uplift_grad_plan.h"
#include <math.h>

namespace {

using namespace ttup;
using namespace ttup::upl;

// ------------------------------------------------------------------ sliced reductions (KSLICE rows per partial sum)
// out[i] += sum over slices, in slice order, of partial[s][i]
__global__ void reduce_kernel(const float* __restrict__ partial, int slices, long long n, float* __restrict__ out) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= n) return;
    float acc = partial[i];
    for (int s = 1; s < slices; ++s) acc += partial[(size_t)s * n + i];
    out[i] += acc;
}
// partial[slice][n] = sum over the slice's rows (fixed order: wave w takes rows w, w+16, ...; the sixteen waves are added 0..15) of z[m][n]
__global__ __launch_bounds__(1024) void colsum_kernel(const float* __restrict__ z, long long ldz, long long M, int N, float* __restrict__ partial) {
    __shared__ float sm[16][64];
    const int lane = ttup_tid_x() & 63, wave = ttup_tid_x() >> 6;
    const int n = ttup_bid_x() * 64 + lane;
    const long long m0 = (long long)ttup_bid_y() * KSLICE;
    const long long m1 = m0 + KSLICE < M ? m0 + KSLICE : M;
    float acc = 0.f;
    if (n < N)
        for (long long m = m0 + wave; m < m1; m += 16) acc += z[m * ldz + n];
    sm[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && n < N) {
        float s = sm[0][lane];
#pragma unroll
        for (int w = 1; w < 16; ++w) s += sm[w][lane];
        partial[(size_t)ttup_bid_y() * N + n] = s;
    }
}

// ------------------------------------------------------------------ LayerNorm (eps 1e-5, biased variance), one wave per row, D <= 256
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                     float* __restrict__ y, long long M, int D) {
    const long long row = (long long)ttup_bid_x() * 4 + (ttup_tid_x() >> 6);
    const int lane = ttup_tid_x() & 63;
    if (row >= M) return;
    const float* r = x + row * D;
    float v[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int k = lane + 64 * i; v[i] = k < D ? r[k] : 0.f; s += v[i]; }
    const float mu = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int k = lane + 64 * i; const float d = k < D ? v[i] - mu : 0.f; q += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int k = lane + 64 * i; if (k < D) y[row * D + k] = (v[i] - mu) * rstd * g[k] + b[k]; }
}
// dx = rstd (g dy - mean(g dy) - xhat mean(g dy xhat)) [+ res];  dyx = dy xhat (its column sums are d gamma)
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ dy,
                                                     const float* __restrict__ res, float* __restrict__ dx, float* __restrict__ dyx, long long M, int D) {
    const long long row = (long long)ttup_bid_x() * 4 + (ttup_tid_x() >> 6);
    const int lane = ttup_tid_x() & 63;
    if (row >= M) return;
    const float* r = x + row * D;
    float v[4], gd[4], xh[4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int k = lane + 64 * i; v[i] = k < D ? r[k] : 0.f; s += v[i]; }
    const float mu = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int k = lane + 64 * i; const float d = k < D ? v[i] - mu : 0.f; q += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = lane + 64 * i;
        xh[i] = 0.f; gd[i] = 0.f;
        if (k < D) {
            const float d = dy[row * D + k];
            xh[i] = (v[i] - mu) * rstd;
            gd[i] = d * g[k];
            dyx[row * D + k] = d * xh[i];
        }
        c1 += gd[i]; c2 += gd[i] * xh[i];
    }
    c1 = wave_sum(c1) / (float)D; c2 = wave_sum(c2) / (float)D;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = lane + 64 * i;
        if (k < D) {
            const float o = rstd * (gd[i] - c1 - xh[i] * c2);
            dx[row * D + k] = res ? o + res[row * D + k] : o;
        }
    }
}
__global__ void relu_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i < n) y[i] = fmaxf(x[i], 0.f);
}

// ------------------------------------------------------------------ token plumbing (the rest: uplift_tokens.h), loss
// the transpose of assemble_table_kernel (uplift_tokens.h): d ball_tok[b,t] = dx[(b,t), 0];  d table_tok[b,n] = sum over t (in order) of dx[(b,t), 1+n]
__global__ void assemble_bwd_kernel(const float* dx, float* d_ball, float* d_table, int B, int T, int NT, int D) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    const long long nb = (long long)B * T * D, ntab = (long long)B * NT * D;
    if (i < nb) {
        d_ball[i] = dx[(i / D) * (NT + 1) * D + i % D];
    } else if (i < nb + ntab) {
        const long long j = i - nb;
        const int d = (int)(j % D);
        const long long bn = j / D;
        const long long b = bn / NT; const int n = (int)(bn % NT);
        float acc = 0.f;
        for (int t = 0; t < T; ++t) acc += dx[(((b * T + t) * (NT + 1)) + 1 + n) * D + d];
        d_table[j] = acc;
    }
}
// the transpose of gather_rows_kernel: y[r * seq_tokens] = x[r], every other row 0
__global__ void expand_rows_kernel(const float* x, float* y, int D, int seq_tokens, long long total) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= total) return;
    const long long r = i / D;
    y[i] = r % seq_tokens == 0 ? x[(r / seq_tokens) * D + i % D] : 0.f;
}
// one workgroup, fixed tree: thread t sums elements t, t+1024, ...; then the halving tree over the 1024 partial sums
__device__ __forceinline__ float block_sum_1024(float v, float* sm) {
    const int tid = ttup_tid_x();
    sm[tid] = v;
    __syncthreads();
    for (int off = 512; off >= 1; off >>= 1) {
        if (tid < off) sm[tid] += sm[tid + off];
        __syncthreads();
    }
    const float r = sm[0];
    __syncthreads();
    return r;
}
__global__ __launch_bounds__(1024) void mask_sum_kernel(const float* mask, long long n, float* out) {
    __shared__ float sm[1024];
    float acc = 0.f;
    for (long long i = ttup_tid_x(); i < n; i += 1024) acc += mask[i];
    const float s = block_sum_1024(acc, sm);
    if (ttup_tid_x() == 0) out[0] = s;
}
// the loss terms of one group of trajectories and their gradients at rot / pos (train.py:107, :125-127); loss[0..1] += the terms
__global__ __launch_bounds__(1024) void loss_kernel(const float* rot, const float* pos, const float* rot_t, const float* r_world, const float* mask,
                                                    const float* mask_sum, int B, int T, float* d_rot, float* d_pos, float* loss) {
    __shared__ float sm[1024];
    const int tid = ttup_tid_x();
    const float msum = mask_sum[0];
    float lr = 0.f, lp = 0.f;
    for (int b = tid; b < B; b += 1024) {
        const float dx = rot[b * 3] - rot_t[b * 3], dy = rot[b * 3 + 1] - rot_t[b * 3 + 1], dz = rot[b * 3 + 2] - rot_t[b * 3 + 2];
        const float n = sqrtf(dx * dx + dy * dy + dz * dz);
        lr += n;
        const float inv = n > 0.f ? 1.f / n : 0.f;
        d_rot[b * 3] = dx * inv; d_rot[b * 3 + 1] = dy * inv; d_rot[b * 3 + 2] = dz * inv;
    }
    const long long n3 = (long long)B * T * 3;
    for (long long i = tid; i < n3; i += 1024) {
        const float m = mask[i / 3];
        float e = 0.f, g = 0.f;
        if (m != 0.f) {          // a padded slot is inert whatever it holds
            const float d = pos[i] - r_world[i];
            e = d * d * m;
            g = 2.f * d * m / msum;
        }
        lp += e;
        d_pos[i] = g;
    }
    const float sr = block_sum_1024(lr, sm);
    const float sp = block_sum_1024(lp, sm);
    if (tid == 0) { loss[0] += sr; loss[1] += sp / msum; }
}

}  // namespace
