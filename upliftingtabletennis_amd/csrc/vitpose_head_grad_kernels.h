// The small kernels of the ViTPose head's training pass (csrc/vitpose_head_grad.hip): the weight pack, batch-statistics BatchNorm
// forward and backward over fixed-order fp64 partial sums, the 1x1 conv's backward, and the reduction that turns the k-slices of a
// dW product into the reference's layout.  The matrix products themselves are gemm_kernel (csrc/gemm_f32.h).
// Every activation is NHWC with DEC channels, so element i belongs to channel i % DEC.  No atomics: every sum has one owner.
#pragma once
#include "common.h"
#include "vitpose_head_plan.h"
#include <math.h>

namespace ttup {
namespace vhead {

typedef float f4 __attribute__((ext_vector_type(4)));

// w (cin, cout, 4, 4), the reference's -> wph (4, cout, 4 cin) and wperm (cin, 16 cout) (vitpose_head_plan.h)
__global__ void pack_kernel(const float* __restrict__ w, int cin, int cout, float* __restrict__ wph, float* __restrict__ wperm) {
    const int i = ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= cin * cout * 16) return;
    const int kx = i & 3, ky = (i >> 2) & 3, co = (i >> 4) % cout, ci = (i >> 4) / cout;
    const float v = w[i];
    wph[phase_index(cin, cout, ci, co, ky, kx)] = v;
    wperm[perm_index(cin, cout, ci, co, ky, kx)] = v;
}
// what the backward reads of the small parameters, kept with the pack: gamma1, gamma2, wf; and the zero bias of the forward's GEMMs
__global__ void keep_small_kernel(const float* __restrict__ g1, const float* __restrict__ g2, const float* __restrict__ wf, int out_ch, float* __restrict__ small) {
    const int i = ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i < DIM) small[SmallOff::ZERO + i] = 0.f;
    if (i < DEC) { small[SmallOff::G1 + i] = g1[i]; small[SmallOff::G2 + i] = g2[i]; }
    if (i < out_ch * DEC) small[SmallOff::WF + i] = wf[i];
}

// ------------------------------------------------------------------ per-channel sums over rows
// partial[slice][0][c], [1][c] = the slice's sums, in fp64, of (z, z^2) -- the forward's statistics -- or, BWD, of (dy, dy xhat) with
// dy = d where gate > 0 (gate null: d as it stands) and xhat = (z - mean) rstd.  Fixed order: wave w takes rows w, w + 16, ...; the
// sixteen waves are added 0..15.  Grid (DEC / 64, slices), 1024 threads.
template <bool BWD>
__global__ __launch_bounds__(1024) void bn_sums_kernel(const float* __restrict__ z, const float* __restrict__ d, const float* __restrict__ gate,
                                                       const float* __restrict__ bn, long long rows, long long per_slice, double* __restrict__ partial) {
    __shared__ double sm[2][16][64];
    const int lane = ttup_tid_x() & 63, wave = ttup_tid_x() >> 6;
    const int c = ttup_bid_x() * 64 + lane;
    const long long m0 = (long long)ttup_bid_y() * per_slice;
    const long long m1 = m0 + per_slice < rows ? m0 + per_slice : rows;
    const float mean = BWD ? bn[S_MEAN * DEC + c] : 0.f, rstd = BWD ? bn[S_RSTD * DEC + c] : 0.f;
    double s0 = 0.0, s1 = 0.0;
    for (long long m = m0 + wave; m < m1; m += 16) {
        const size_t e = (size_t)m * DEC + c;
        if (BWD) {
            const float dy = !gate || gate[e] > 0.f ? d[e] : 0.f;
            const float xh = (z[e] - mean) * rstd;
            s0 += (double)dy; s1 += (double)dy * (double)xh;
        } else {
            const double v = (double)z[e];
            s0 += v; s1 += v * v;
        }
    }
    sm[0][wave][lane] = s0; sm[1][wave][lane] = s1;
    __syncthreads();
    if (wave < 2) {
        double s = sm[wave][0][lane];
#pragma unroll
        for (int w = 1; w < 16; ++w) s += sm[wave][w][lane];
        partial[((size_t)ttup_bid_y() * 2 + wave) * DEC + c] = s;
    }
}

// Forward statistics of one BN, 256 threads.  train: mean and biased variance from the partial sums (slice order), and the
// running statistics' update (momentum 0.1, the unbiased variance; *tracked += 1).  eval: the running statistics as they stand.
__global__ void bn_finalize_kernel(const double* __restrict__ partial, int nslices, long long n, int train, float* __restrict__ run_mean,
                                   float* __restrict__ run_var, long long* __restrict__ tracked, float* __restrict__ bn) {
    const int c = ttup_tid_x();
    double mean, var;
    if (train) {
        double s = 0.0, q = 0.0;
        for (int i = 0; i < nslices; ++i) { s += partial[((size_t)i * 2) * DEC + c]; q += partial[((size_t)i * 2 + 1) * DEC + c]; }
        mean = s / (double)n;
        var = q / (double)n - mean * mean;
        if (var < 0.0) var = 0.0;
        run_mean[c] = (float)((1.0 - BN_MOMENTUM) * (double)run_mean[c] + BN_MOMENTUM * mean);
        run_var[c] = (float)((1.0 - BN_MOMENTUM) * (double)run_var[c] + BN_MOMENTUM * var * ((double)n / (double)(n - 1)));
        if (c == 0) *tracked += 1;
    } else {
        mean = (double)run_mean[c]; var = (double)run_var[c];
    }
    bn[S_MEAN * DEC + c] = (float)mean;
    bn[S_VAR * DEC + c] = (float)var;
    bn[S_RSTD * DEC + c] = (float)(1.0 / sqrt((double)(float)var + BN_EPS));
}

// a = relu((z - mean) rstd gamma + beta), four channels a thread
__global__ void bn_relu_kernel(const float* __restrict__ z, const float* __restrict__ bn, const float* __restrict__ gamma, const float* __restrict__ beta,
                               float* __restrict__ a, long long quads) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= quads) return;
    const int c = (int)(i % (DEC / 4)) * 4;
    const f4 v = *(const f4*)(z + i * 4), mu = *(const f4*)(bn + S_MEAN * DEC + c), rs = *(const f4*)(bn + S_RSTD * DEC + c);
    const f4 g = *(const f4*)(gamma + c), b = *(const f4*)(beta + c);
    f4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = fmaxf((v[e] - mu[e]) * rs[e] * g[e] + b[e], 0.f);
    *(f4*)(a + i * 4) = o;
}

// d gamma = sum dy xhat, d beta = sum dy (both modes), and the two means the train-mode dz subtracts (eval: 0)
__global__ void bn_bwd_finalize_kernel(const double* __restrict__ partial, int nslices, long long n, int train, float* __restrict__ dgamma,
                                       float* __restrict__ dbeta, float* __restrict__ bn) {
    const int c = ttup_tid_x();
    double s = 0.0, q = 0.0;
    for (int i = 0; i < nslices; ++i) { s += partial[((size_t)i * 2) * DEC + c]; q += partial[((size_t)i * 2 + 1) * DEC + c]; }
    dbeta[c] = (float)s; dgamma[c] = (float)q;
    bn[S_C1 * DEC + c] = train ? (float)(s / (double)n) : 0.f;
    bn[S_C2 * DEC + c] = train ? (float)(q / (double)n) : 0.f;
}

// d (in place) -> dz = gamma rstd (dy - mean(dy) - xhat mean(dy xhat)), dy = d where gate > 0 (gate null: d as it stands); in eval mode
// the two means are zero and this is dy gamma rstd
__global__ void bn_dz_kernel(float* __restrict__ d, const float* __restrict__ z, const float* __restrict__ gate, const float* __restrict__ bn,
                             const float* __restrict__ gamma, long long quads) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= quads) return;
    const int c = (int)(i % (DEC / 4)) * 4;
    f4 dy = *(const f4*)(d + i * 4);
    const f4 v = *(const f4*)(z + i * 4);
    if (gate) {
        const f4 a = *(const f4*)(gate + i * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) dy[e] = a[e] > 0.f ? dy[e] : 0.f;
    }
    const f4 mu = *(const f4*)(bn + S_MEAN * DEC + c), rs = *(const f4*)(bn + S_RSTD * DEC + c), c1 = *(const f4*)(bn + S_C1 * DEC + c),
             c2 = *(const f4*)(bn + S_C2 * DEC + c), g = *(const f4*)(gamma + c);
    f4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = g[e] * rs[e] * (dy[e] - c1[e] - (v[e] - mu[e]) * rs[e] * c2[e]);
    *(f4*)(d + i * 4) = o;
}

// ------------------------------------------------------------------ the 1x1 conv, forward and backward
// heat (B, cout, H, W) = wf (cout, DEC) a2 + bias from NHWC a2: 64 pixels a workgroup staged through LDS 64 channels at a time, thread
// (pixel, channel group) -- the scheme of the inference head's conv1x1_kernel (csrc/vitpose_kernels.h)
__global__ __launch_bounds__(256) void conv1x1_fwd_kernel(const float* __restrict__ a2, long long npix, int hw, const float* __restrict__ wf,
                                                          const float* __restrict__ bias, int cout, float* __restrict__ heat) {
    __shared__ float sx[64 * (64 + 1)];
    const int tid = ttup_tid_x();
    const long long p0 = (long long)ttup_bid_x() * 64;
    const int pl = tid & 63, cg = tid >> 6;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};          // output channels cg, cg + 4, cg + 8, cg + 12
    for (int c0 = 0; c0 < DEC; c0 += 64) {
        for (int e = tid; e < 64 * 64; e += 256) {
            const int pp = e >> 6, c = e & 63;
            sx[pp * 65 + c] = p0 + pp < npix ? a2[(size_t)(p0 + pp) * DEC + c0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = cg + 4 * j;
            if (co < cout)
                for (int c = 0; c < 64; ++c) acc[j] += sx[pl * 65 + c] * wf[co * DEC + c0 + c];
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
// dy2[pix][k] = sum_c wf[c][k] dheat[b][c][t] where a2[pix][k] > 0, else 0 (the second ReLU's gate); four channels a thread
__global__ void conv1x1_bwd_kernel(const float* __restrict__ dheat, const float* __restrict__ a2, const float* __restrict__ wf, long long npix, int hw,
                                   int cout, float* __restrict__ dy) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= npix * (DEC / 4)) return;
    const long long pix = i / (DEC / 4), b = pix / hw, t = pix - b * hw;
    const int k = (int)(i - pix * (DEC / 4)) * 4;
    f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < cout; ++c) {
        const float g = dheat[((size_t)b * cout + c) * hw + t];
        const f4 w = *(const f4*)(wf + c * DEC + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += w[e] * g;
    }
    const f4 a = *(const f4*)(a2 + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = a[e] > 0.f ? acc[e] : 0.f;
    *(f4*)(dy + i * 4) = acc;
}
// part[j][c][k] = sum over part j's pixels (in order) of dheat[c, pix] a2[pix][k], and behind them part[j][cout * DEC + c] = sum of
// dheat[c, pix], in fp64; part j = DWF_SUB * slice + sub covers per_part pixels of that slice.  Thread k; grid (slices * DWF_SUB).
__global__ __launch_bounds__(DEC) void dwf_partial_kernel(const float* __restrict__ dheat, const float* __restrict__ a2, long long npix, int hw, int cout,
                                                          long long per_slice, double* __restrict__ part) {
    const int k = ttup_tid_x(), j = ttup_bid_x();
    const long long per_part = per_slice / DWF_SUB;
    const long long p0 = (long long)(j / DWF_SUB) * per_slice + (long long)(j % DWF_SUB) * per_part;
    const long long slice_end = (long long)(j / DWF_SUB + 1) * per_slice < npix ? (long long)(j / DWF_SUB + 1) * per_slice : npix;
    const long long p1 = p0 + per_part < slice_end ? p0 + per_part : slice_end;
    double acc[MAX_OUT], sb[MAX_OUT];
#pragma unroll
    for (int c = 0; c < MAX_OUT; ++c) { acc[c] = 0.0; sb[c] = 0.0; }
    for (long long pix = p0; pix < p1; ++pix) {
        const long long b = pix / hw, t = pix - b * hw;
        const double a = (double)a2[(size_t)pix * DEC + k];
#pragma unroll
        for (int c = 0; c < MAX_OUT; ++c)
            if (c < cout) {
                const double g = (double)dheat[((size_t)b * cout + c) * hw + t];
                acc[c] += g * a; sb[c] += g;
            }
    }
    double* o = part + (size_t)j * ((size_t)cout * DEC + cout);
#pragma unroll
    for (int c = 0; c < MAX_OUT; ++c)
        if (c < cout) {
            o[(size_t)c * DEC + k] = acc[c];
            if (k == 0) o[(size_t)cout * DEC + c] = sb[c];
        }
}
// dwf (cout, DEC) and dbf (cout) = the parts added in order
__global__ void dwf_finalize_kernel(const double* __restrict__ part, int parts, int cout, float* __restrict__ dwf, float* __restrict__ dbf) {
    const int i = ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    const int n = cout * DEC + cout;
    if (i >= n) return;
    double s = 0.0;
    for (int j = 0; j < parts; ++j) s += part[(size_t)j * n + i];
    if (i < cout * DEC) dwf[i] = (float)s; else dbf[i - cout * DEC] = (float)s;
}

// ------------------------------------------------------------------ dW: the k-slices of A^T G -> the reference's layout
// dw (cin, cout, 4, 4)[ref_of_perm(e)] = sum over slices, in slice order, of partial[s][e], e over (cin, 16 cout)
__global__ void dw_reduce_kernel(const float* __restrict__ partial, int nslices, int cin, int cout, float* __restrict__ dw) {
    const long long n = (long long)cin * 16 * cout;
    const long long e = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (e >= n) return;
    float acc = partial[e];
    for (int s = 1; s < nslices; ++s) acc += partial[(size_t)s * n + e];
    dw[ref_of_perm(cin, cout, (size_t)e)] = acc;
}

}  // namespace vhead
}  // namespace ttup
