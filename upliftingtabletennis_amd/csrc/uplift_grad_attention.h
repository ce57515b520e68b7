// The attention kernel of the uplift gradient pass (csrc/uplift_grad.hip), forward and backward, and its launcher.  The launch
// geometry is attn_geom (csrc/uplift_grad_plan.h).
#pragma once
#include "common.h"
#include "uplift_net.h"
#include <math.h>

namespace {

using namespace ttup;
using namespace ttup::upl;

// ------------------------------------------------------------------ attention (model.py:186-229), forward and backward
// P >= S threads per (sequence, head), thread i owns query row i (and, in the second half of the backward pass, key row i).  The
// rotated q / k, v and (backward) dO of the sequence live in LDS.  Additive {0, -inf} row + column mask: a masked key is skipped, a
// masked query row yields zeros (torch SDPA) and gets a zero gradient.
struct AttnArgs {
    const float* qkv;   // [n_seq*S][3D], q and k before RoPE
    float* out;         // forward: attention output [n_seq*S][D]
    const float* o;     // backward: the forward's output
    const float* d_o;   // backward: its gradient
    float* dqkv;        // backward: [n_seq*S][3D]
    int n_seq, D, P;
    SeqView sv;
};

template <int HD, bool BWD>
__global__ __launch_bounds__(256) void attention_grad_kernel(AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int S = a.sv.S, P = a.P, G = ttup_bdim_x() / P;
    const int NARR = BWD ? 4 : 2;                     // k~, v, (q~, dO)
    const int SEQ = NARR * S * HD + (BWD ? 3 * S : 0) + S;          // floats per sequence: the arrays, (mx, 1/den, rowsum(dO o O)), mask
    const int h = ttup_bid_y(), tid = ttup_tid_x();
    const int D3 = 3 * a.D;
    // ---- stage: pairs (2e, 2e+1) of token j, rotated by the token's (cos, sin) row
    for (int u = tid; u < G * S * (HD / 2); u += ttup_bdim_x()) {
        const int g = u / (S * (HD / 2)), rem = u - g * (S * (HD / 2)), j = rem / (HD / 2), e = rem - j * (HD / 2);
        const int seq = ttup_bid_x() * G + g;
        if (seq >= a.n_seq) continue;
        float* base = sm + (size_t)g * SEQ;
        const float* qp = a.qkv + ((size_t)seq * S + j) * D3 + h * HD + 2 * e;
        float2 q = *(const float2*)qp, k = *(const float2*)(qp + a.D);
        const float2 v = *(const float2*)(qp + 2 * a.D);
        if (j >= a.sv.num_cls) {
            const float2 cs = a.sv.rope[((size_t)(seq / a.sv.times_div) * a.sv.times_stride + (j - a.sv.num_cls)) * (HD / 2) + e];
            k = make_float2(k.x * cs.x - k.y * cs.y, k.x * cs.y + k.y * cs.x);
            q = make_float2(q.x * cs.x - q.y * cs.y, q.x * cs.y + q.y * cs.x);
        }
        base[j * HD + 2 * e] = k.x; base[j * HD + 2 * e + 1] = k.y;
        base[S * HD + j * HD + 2 * e] = v.x; base[S * HD + j * HD + 2 * e + 1] = v.y;
        if (BWD) {
            base[2 * S * HD + j * HD + 2 * e] = q.x; base[2 * S * HD + j * HD + 2 * e + 1] = q.y;
            const float2 d = *(const float2*)(a.d_o + ((size_t)seq * S + j) * a.D + h * HD + 2 * e);
            base[3 * S * HD + j * HD + 2 * e] = d.x; base[3 * S * HD + j * HD + 2 * e + 1] = d.y;
        }
    }
    for (int u = tid; u < G * S; u += ttup_bdim_x()) {
        const int g = u / S, j = u - g * S;
        const int seq = ttup_bid_x() * G + g;
        sm[(size_t)g * SEQ + NARR * S * HD + (BWD ? 3 * S : 0) + j] = seq < a.n_seq ? a.sv.mask[(size_t)(seq / a.sv.mask_div) * S + j] : -INFINITY;
    }
    __syncthreads();
    const int g = tid / P, i = tid - g * P;
    const int seq = ttup_bid_x() * G + g;
    const bool live = seq < a.n_seq && i < S;
    float* base = sm + (size_t)g * SEQ;
    const float* ks = base;
    const float* vs = base + S * HD;
    const float* qs = base + 2 * S * HD;
    const float* ds = base + 3 * S * HD;
    float* stats = base + NARR * S * HD;
    const float* mg = base + NARR * S * HD + (BWD ? 3 * S : 0);
    const bool row_on = live && mg[i] == 0.f;
    float q[HD];
    float mx = -INFINITY, den = 0.f;
    if (row_on) {
        if (BWD) {
#pragma unroll
            for (int d = 0; d < HD; ++d) q[d] = qs[i * HD + d];
        } else {
            const float* qp = a.qkv + ((size_t)seq * S + i) * D3 + h * HD;
#pragma unroll
            for (int d = 0; d < HD; ++d) q[d] = qp[d];
            if (i >= a.sv.num_cls) {
                const float2* rp = a.sv.rope + ((size_t)(seq / a.sv.times_div) * a.sv.times_stride + (i - a.sv.num_cls)) * (HD / 2);
#pragma unroll
                for (int e = 0; e < HD / 2; ++e) {
                    const float2 cs = rp[e];
                    const float x0 = q[2 * e], x1 = q[2 * e + 1];
                    q[2 * e] = x0 * cs.x - x1 * cs.y; q[2 * e + 1] = x0 * cs.y + x1 * cs.x;
                }
            }
        }
        for (int j = 0; j < S; ++j) {
            if (mg[j] != 0.f) continue;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) s = fmaf(q[d], ks[j * HD + d], s);
            s *= a.sv.scale;
            mx = s > mx ? s : mx;
        }
        for (int j = 0; j < S; ++j) {
            if (mg[j] != 0.f) continue;
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) s = fmaf(q[d], ks[j * HD + d], s);
            den += expf(s * a.sv.scale - mx);
        }
    }
    const float inv = den > 0.f ? 1.f / den : 0.f;
    if (!BWD) {
        if (!live) return;
        float o[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) o[d] = 0.f;
        if (row_on)
            for (int j = 0; j < S; ++j) {
                if (mg[j] != 0.f) continue;
                float s = 0.f;
#pragma unroll
                for (int d = 0; d < HD; ++d) s = fmaf(q[d], ks[j * HD + d], s);
                const float p = expf(s * a.sv.scale - mx) * inv;
#pragma unroll
                for (int d = 0; d < HD; ++d) o[d] = fmaf(p, vs[j * HD + d], o[d]);
            }
        float* op = a.out + ((size_t)seq * S + i) * a.D + h * HD;
#pragma unroll
        for (int d = 0; d < HD; ++d) op[d] = o[d];
        return;
    }
    // ---- backward, first half: dq of query row i;  (mx, 1/den, rowsum(dO o O)) go to LDS for the second half
    float acc[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] = 0.f;
    float dsum = 0.f;
    if (row_on) {
        const float* op = a.o + ((size_t)seq * S + i) * a.D + h * HD;
#pragma unroll
        for (int d = 0; d < HD; ++d) dsum = fmaf(ds[i * HD + d], op[d], dsum);
        for (int j = 0; j < S; ++j) {
            if (mg[j] != 0.f) continue;
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { s = fmaf(q[d], ks[j * HD + d], s); dp = fmaf(ds[i * HD + d], vs[j * HD + d], dp); }
            const float p = expf(s * a.sv.scale - mx) * inv;
            const float t = p * (dp - dsum) * a.sv.scale;
#pragma unroll
            for (int d = 0; d < HD; ++d) acc[d] = fmaf(t, ks[j * HD + d], acc[d]);
        }
    }
    if (live) {
        stats[3 * i] = row_on ? mx : 0.f; stats[3 * i + 1] = row_on ? inv : 0.f; stats[3 * i + 2] = dsum;
        float* gp = a.dqkv + ((size_t)seq * S + i) * D3 + h * HD;
        if (i >= a.sv.num_cls) {          // back through the rotation: its transpose
            const float2* rp = a.sv.rope + ((size_t)(seq / a.sv.times_div) * a.sv.times_stride + (i - a.sv.num_cls)) * (HD / 2);
#pragma unroll
            for (int e = 0; e < HD / 2; ++e) {
                const float2 cs = rp[e];
                const float x0 = acc[2 * e], x1 = acc[2 * e + 1];
                gp[2 * e] = x0 * cs.x + x1 * cs.y; gp[2 * e + 1] = x1 * cs.x - x0 * cs.y;
            }
        } else {
#pragma unroll
            for (int d = 0; d < HD; ++d) gp[d] = acc[d];
        }
    }
    __syncthreads();
    // ---- second half: thread i owns KEY row i: dk_i = sum_r dS[r][i] q_r,  dv_i = sum_r P[r][i] dO_r  (r in row order)
    if (!live) return;
    float dk[HD], dv[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
    if (mg[i] == 0.f) {
        float kk[HD], vv[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) { kk[d] = ks[i * HD + d]; vv[d] = vs[i * HD + d]; }
        for (int r = 0; r < S; ++r) {
            if (mg[r] != 0.f) continue;
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) { s = fmaf(qs[r * HD + d], kk[d], s); dp = fmaf(ds[r * HD + d], vv[d], dp); }
            const float p = expf(s * a.sv.scale - stats[3 * r]) * stats[3 * r + 1];
            const float t = p * (dp - stats[3 * r + 2]) * a.sv.scale;
#pragma unroll
            for (int d = 0; d < HD; ++d) { dk[d] = fmaf(t, qs[r * HD + d], dk[d]); dv[d] = fmaf(p, ds[r * HD + d], dv[d]); }
        }
    }
    float* gk = a.dqkv + ((size_t)seq * S + i) * D3 + a.D + h * HD;
    if (i >= a.sv.num_cls) {
        const float2* rp = a.sv.rope + ((size_t)(seq / a.sv.times_div) * a.sv.times_stride + (i - a.sv.num_cls)) * (HD / 2);
#pragma unroll
        for (int e = 0; e < HD / 2; ++e) {
            const float2 cs = rp[e];
            const float x0 = dk[2 * e], x1 = dk[2 * e + 1];
            gk[2 * e] = x0 * cs.x + x1 * cs.y; gk[2 * e + 1] = x1 * cs.x - x0 * cs.y;
        }
    } else {
#pragma unroll
        for (int d = 0; d < HD; ++d) gk[d] = dk[d];
    }
#pragma unroll
    for (int d = 0; d < HD; ++d) gk[a.D + d] = dv[d];
}

template <int HD, bool BWD>
int launch_attention(const AttnArgs& a, const AttnGeom& g, int heads, hipStream_t st) {
    if (g.lds > 48 * 1024)
        if (int rc = ensure_max_lds((const void*)attention_grad_kernel<HD, BWD>, ATTN_MAX_LDS)) return rc;
    hipLaunchKernelGGL((attention_grad_kernel<HD, BWD>), dim3((unsigned)((a.n_seq + g.seqs - 1) / g.seqs), (unsigned)heads), dim3(g.threads), g.lds, st, a);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}
template <bool BWD>
int run_attention(const ttup_uplift* net, AttnArgs a, hipStream_t st) {
    const AttnGeom g = attn_geom(a.sv.S, net->hd, BWD);
    // ttup_uplift_loss_grad has settled this for the call's three sequence lengths before it enqueued anything
    TTUP_REQUIRE(g.ok, TTUP_EINVAL, "uplift gradient: head_dim %d / sequence length %d not served by the attention kernels", net->hd, a.sv.S);
    a.D = net->D; a.P = g.P;
    if (a.n_seq == 0) return TTUP_OK;
    switch (net->hd) {
        case 8: return launch_attention<8, BWD>(a, g, net->heads, st);
        case 16: return launch_attention<16, BWD>(a, g, net->heads, st);
        case 24: return launch_attention<24, BWD>(a, g, net->heads, st);
    }
    return launch_attention<32, BWD>(a, g, net->heads, st);
}

}  // namespace
