// The uplift transformer's training loss (reference uplifting/train.py:105-127) and its gradient with respect to every parameter,
// for the configuration the reference trains: get_model('connectstage', size, 'dynamic', time_rotation).  fp32 throughout.
//
//   loss_rot = sum_b || pred_rot_b - rot_b ||_2        loss_pos = sum (pred_pos - r_world)^2 mask / sum mask        loss = loss_rot + loss_pos
//
// Forward: the layer-by-layer sequence of uplift.hip's forward_chunk on plain fp32 weights (ttup_uplift::plain), every product on
// gemm_f32.h's v_mfma_f32_16x16x4_f32 GEMM, keeping per layer the LayerNorm-1 input, the qkv rows BEFORE RoPE, the attention output,
// the LayerNorm-2 input and the fc1 pre-activation.  LayerNorm statistics, the rotated q / k, the attention probabilities and the
// ReLU outputs are recomputed in the backward pass (the same instructions on the same values: the same bits).
// Backward: per linear layer  dX = dY W  (gemm O_ROWS x O_COLS),  dW = dY^T X  (gemm O_COLS x O_COLS, the row range cut into slices
// of KSLICE rows whose partial products are summed in slice order by reduce_kernel),  db = column sums of dY  (colsum_kernel, same
// slices);  LayerNorm backward one wave per row;  attention backward one group of threads per (sequence, head).
// Determinism: no floating-point atomics anywhere; every reduction has a fixed tree that depends on (batch, len) alone.  The batch is
// processed in groups of trajectories whose size is a function of len only, never of the handle's max_batch / scratch chunk.
#include "no_packed_fp32_begin.h"      // this unit's kernels run beside the CNN's chain kernels: no packed fp32 (common.h)
#include "common.h"
#include "uplift_net.h"
#include "gemm_f32.h"
#include "uplift_tokens.h"
#include <math.h>
#include <vector>

using namespace ttup;
using namespace ttup::upl;
using namespace ttup::gemm;

namespace {

constexpr int KSLICE = 512;                  // rows per partial sum of dW / db / dgamma / dbeta / d cls
constexpr long long GROUP_TOKENS = 262144;   // table-stage tokens (14 per time step) per group of trajectories
constexpr int FLAG_LOCAL = 1;                // transform_mode == 'local'
constexpr int FLAG_CHECK_MASK = 2;           // the reference's mask-format ValueError (model.py:541-546): one read-back and one stream synchronisation

// ------------------------------------------------------------------ GEMM wrappers (gemm_f32.h, GUARD form)
template <int AM, int WM>
int gemm(const float* a, int lda, const float* w, int ldw, float* out, int ldo, long long M, int N, int K, const float* bias, int flags,
         const float* res, int ldr, const float* gate, int ldg, int kslice, hipStream_t st) {
    if (M == 0 || N == 0) return TTUP_OK;
    GemmArgs p = {};
    p.a = a; p.w = w; p.bias = bias; p.res = res; p.out = out; p.M = (int)M; p.N = N; p.K = K; p.flags = flags;
    p.lda = lda; p.ldw = ldw; p.ldo = ldo; p.ldr = ldr; p.gate = gate; p.ldg = ldg;
    p.kslice = kslice > 0 ? kslice : (K + BK - 1) / BK * BK;
    const int slices = (K + p.kslice - 1) / p.kslice;
    hipLaunchKernelGGL((gemm_kernel<AM, true, WM>), dim3((unsigned)((M + BM - 1) / BM), (unsigned)((N + BN - 1) / BN), (unsigned)slices), dim3(256), 0, st, p);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}
// out[m][n] = epilogue(sum_k x[m][k] W[n][k] + b[n])
int linear_fwd(const float* x, int ldx, const float* W, const float* b, float* out, int ldo, long long M, int N, int K, int flags,
               const float* res, int ldr, hipStream_t st) {
    return gemm<O_ROWS, O_ROWS>(x, ldx, W, K, out, ldo, M, N, K, b, flags, res, ldr, nullptr, 0, 0, st);
}
// dx[m][k] = sum_n dy[m][n] W[n][k]   (+ res, or gated by gate > 0)
int linear_dx(const float* dy, int ldy, const float* W, float* dx, int ldx, long long M, int N, int K, int flags, const float* res, int ldr,
              const float* gate, int ldg, hipStream_t st) {
    return gemm<O_ROWS, O_COLS>(dy, ldy, W, K, dx, ldx, M, K, N, nullptr, flags, res, ldr, gate, ldg, 0, st);
}

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

struct Ctx {
    hipStream_t st;
    float* partial;          // scratch of the sliced reductions
};

int reduce_into(const Ctx& c, int slices, long long n, float* out) {
    return launch_1d(reduce_kernel, n, c.st, c.partial, slices, n, out);
}
// g[n] += column sums of z (M rows of leading dimension ldz)
int colsum_into(const Ctx& c, const float* z, long long ldz, long long M, int N, float* g) {
    if (M == 0) return TTUP_OK;
    const int slices = (int)((M + KSLICE - 1) / KSLICE);
    hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)slices), dim3(1024), 0, c.st, z, ldz, M, N, c.partial);
    TTUP_LAUNCH_CHECK();
    return reduce_into(c, slices, N, g);
}
// gW[n][k] += sum_m dy[m][n] x[m][k];  gb[n] += sum_m dy[m][n]
int linear_dw(const Ctx& c, const float* dy, int ldy, const float* x, int ldx, long long M, int N, int K, float* gW, float* gb) {
    if (M == 0) return TTUP_OK;
    const int slices = (int)((M + KSLICE - 1) / KSLICE);
    if (int rc = gemm<O_COLS, O_COLS>(dy, ldy, x, ldx, c.partial, K, N, K, (int)M, nullptr, 0, nullptr, 0, nullptr, 0, KSLICE, c.st)) return rc;
    if (int rc = reduce_into(c, slices, (long long)N * K, gW)) return rc;
    return gb ? colsum_into(c, dy, ldy, M, N, gb) : TTUP_OK;
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
int launch_attention(const AttnArgs& a, int heads, hipStream_t st) {
    const int G = a.P >= 64 ? 1 : 64 / a.P, threads = G * a.P;
    const size_t smem = (size_t)G * ((BWD ? 4 : 2) * a.sv.S * HD + (BWD ? 3 * a.sv.S : 0) + a.sv.S) * sizeof(float);
    TTUP_REQUIRE(smem <= 160 * 1024, TTUP_EINVAL, "uplift gradient: sequence length %d too long for the attention kernels", a.sv.S);
    if (smem > 48 * 1024)
        if (int rc = ensure_max_lds((const void*)attention_grad_kernel<HD, BWD>, 160 * 1024)) return rc;
    hipLaunchKernelGGL((attention_grad_kernel<HD, BWD>), dim3((unsigned)((a.n_seq + G - 1) / G), (unsigned)heads), dim3(threads), smem, st, a);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}
template <bool BWD>
int run_attention(const ttup_uplift* net, AttnArgs a, hipStream_t st) {
    a.D = net->D;
    int P = 16;
    while (P < a.sv.S) P *= 2;
    TTUP_REQUIRE(P <= 256, TTUP_EINVAL, "uplift gradient: sequence length %d above 256", a.sv.S);
    a.P = P;
    if (a.n_seq == 0) return TTUP_OK;
    switch (net->hd) {
        case 8: return launch_attention<8, BWD>(a, net->heads, st);
        case 16: return launch_attention<16, BWD>(a, net->heads, st);
        case 24: return launch_attention<24, BWD>(a, net->heads, st);
        case 32: return launch_attention<32, BWD>(a, net->heads, st);
    }
    set_error("uplift gradient: head_dim %d unsupported", net->hd);
    return TTUP_EINVAL;
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

// ------------------------------------------------------------------ parameters and workspace
struct LinP { const float *w, *b; float *gw, *gb; int n, k; };
struct LayerP { LinP qkv, proj, fc1, fc2; const float *g1, *b1, *g2, *b2; float *dg1, *db1, *dg2, *db2; };
struct HeadP { LinP fc1, fc2, fc3; };
struct Params {
    const float* cls; float* dcls;
    LinP ball1, ball2, tab1, tab2;
    std::vector<LayerP> pos, first, second;
    HeadP pos_head, rot_head;
    long long n_floats = 0;
};
long long embed_floats(int D) { return (long long)D * 3 + D + (long long)D * D + D; }

// walks the plain weights (blob order) and the flat gradient buffer (arch.uplift_variant_schema order without inv_freq) together
void map_params(const ttup_uplift* net, float* grad, Params* P) {
    const int D = net->D;
    const float* w = net->plain;
    float* g = grad;
    long long used = 0;
    auto vec = [&](long long n, const float** pw, float** pg) { *pw = w; *pg = g; w += n; g += n; used += n; };
    auto lin = [&](int n, int k, bool bias, LinP* L) {
        L->n = n; L->k = k; L->b = nullptr; L->gb = nullptr;
        vec((long long)n * k, &L->w, &L->gw);
        if (bias) vec(n, &L->b, &L->gb);
    };
    auto layer = [&](LayerP* L) {
        lin(3 * D, D, true, &L->qkv); lin(D, D, false, &L->proj); lin(D, D, true, &L->fc1); lin(D, D, true, &L->fc2);
        vec(D, &L->g1, &L->dg1); vec(D, &L->b1, &L->db1); vec(D, &L->g2, &L->dg2); vec(D, &L->b2, &L->db2);
    };
    auto head = [&](HeadP* H) { lin(D / 2, D, true, &H->fc1); lin(D / 4, D / 2, true, &H->fc2); lin(3, D / 4, true, &H->fc3); };
    vec(D, &P->cls, &P->dcls);
    g += embed_floats(D); used += embed_floats(D);          // embed.*: in the state dict, read by 'multistage' alone -- no gradient
    lin(D, 2, true, &P->ball1); lin(D, D, true, &P->ball2); lin(D, 2, true, &P->tab1); lin(D, D, true, &P->tab2);
    P->pos.resize(net->pos_layers.size()); P->first.resize(net->layers.size()); P->second.resize(net->second.size());
    for (auto& L : P->pos) layer(&L);
    for (auto& L : P->first) layer(&L);
    head(&P->pos_head);
    for (auto& L : P->second) layer(&L);
    head(&P->rot_head);
    P->n_floats = used;
}

// what the forward keeps of one layer (floats per token: 7 D)
struct Saved { float *x, *qkv, *att, *x2, *hp; };
struct Stage { std::vector<Saved> L; float* out; long long tokens; int n_seq, S, num_cls; };
struct Plan {
    int G = 0;                                   // trajectories per group
    long long n1 = 0, nt = 0, n2 = 0;            // table-stage / temporal / spin tokens of a full group
    long long total = 0;                         // floats
    Stage table, temporal, spin;
    float *tA, *tB, *tC, *tE, *dX, *dY, *tQ, *partial;
    float *ball_h, *ball_tok, *tab_h, *tab_tok, *pos_h1, *pos_h2, *rot_h1, *rot_h2;
    float *m1, *m2, *tmask, *txy, *rope, *rot_t, *d_rot, *d_pos, *mask_sum;
};
bool supported(const ttup_uplift* net) { return net->name == NAME_CONNECT && net->mode == MODE_DYNAMIC && net->plain; }
const char* variant_text(const ttup_uplift* net) {
    static const char* names[] = {"connectstage", "multistage", "singlestage"};
    static const char* modes[] = {"dynamic", "stacked", "originalmethod", "free"};
    static thread_local char buf[64];
    snprintf(buf, sizeof buf, "%s/%s", names[net->name % 3], modes[net->mode % 4]);
    return buf;
}
int group_size(int batch, int len) {
    long long g = GROUP_TOKENS / ((long long)len * 14);
    if (g < 1) g = 1;
    return (int)(g < batch ? g : batch);
}
void make_plan(const ttup_uplift* net, int batch, int len, float* base, Plan* p) {
    const int D = net->D, NT = net->n_table;
    p->G = group_size(batch, len);
    p->n1 = (long long)p->G * len * (NT + 1); p->nt = (long long)p->G * len; p->n2 = (long long)p->G * (len + 1);
    long long off = 0;
    auto take = [&](long long n) { float* r = base ? base + off : nullptr; off += (n + 3) / 4 * 4; return r; };
    auto stage = [&](Stage* s, size_t layers, long long tokens, int n_seq, int S, int num_cls) {
        s->tokens = tokens; s->n_seq = n_seq; s->S = S; s->num_cls = num_cls;
        s->L.resize(layers);
        for (auto& L : s->L) { L.x = take(tokens * D); L.qkv = take(tokens * 3 * D); L.att = take(tokens * D); L.x2 = take(tokens * D); L.hp = take(tokens * D); }
        s->out = take(tokens * D);
    };
    stage(&p->table, net->pos_layers.size(), p->n1, (int)p->nt, NT + 1, 1);
    stage(&p->temporal, net->layers.size(), p->nt, p->G, len, 0);
    stage(&p->spin, net->second.size(), p->n2, p->G, len + 1, 1);
    p->tA = take(p->n1 * D); p->tB = take(p->n1 * D); p->tC = take(p->n1 * D); p->tE = take(p->n1 * D); p->dX = take(p->n1 * D); p->dY = take(p->nt * D);
    p->tQ = take(p->n1 * 3 * D);
    const long long slices = (p->n1 + KSLICE - 1) / KSLICE;
    p->partial = take(slices * 3 * D * D);
    p->ball_h = take(p->nt * D); p->ball_tok = take(p->nt * D); p->tab_h = take((long long)p->G * NT * D); p->tab_tok = take((long long)p->G * NT * D);
    p->pos_h1 = take(p->nt * (D / 2)); p->pos_h2 = take(p->nt * (D / 4)); p->rot_h1 = take((long long)p->G * (D / 2)); p->rot_h2 = take((long long)p->G * (D / 4));
    p->m1 = take(p->nt); p->m2 = take(p->n2); p->tmask = take((long long)p->G * (NT + 1)); p->txy = take((long long)p->G * NT * 2);
    p->rope = take(p->nt * net->hd); p->rot_t = take((long long)p->G * 3); p->d_rot = take((long long)p->G * 3); p->d_pos = take(p->nt * 3);
    p->mask_sum = take(4);
    p->total = off;
}

#define GRC(expr) do { if (int rc_ = (expr)) return rc_; } while (0)
#define LAUNCH1D(kernel, total, ...) do { if ((total) > 0) GRC(launch_1d(kernel, total, c.st, __VA_ARGS__)); } while (0)

int ln_fwd(const Ctx& c, const float* x, const float* g, const float* b, float* y, long long M, int D) {
    if (M == 0) return TTUP_OK;
    hipLaunchKernelGGL(ln_fwd_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, c.st, x, g, b, y, M, D);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// SimpleStaticLayer.forward (model.py:278-300): x -> xo, keeping S
int layer_fwd(const ttup_uplift* net, const Ctx& c, const Plan& p, const LayerP& L, const Saved& S, float* xo, const Stage& sg, int n_seq, const SeqView& sv) {
    const int D = net->D;
    const long long M = (long long)n_seq * sg.S;
    GRC(ln_fwd(c, S.x, L.g1, L.b1, p.tA, M, D));
    GRC(linear_fwd(p.tA, D, L.qkv.w, L.qkv.b, S.qkv, 3 * D, M, 3 * D, D, 0, nullptr, 0, c.st));
    AttnArgs a = {};
    a.qkv = S.qkv; a.sv = sv; a.out = S.att; a.n_seq = n_seq;
    GRC(run_attention<false>(net, a, c.st));
    GRC(linear_fwd(S.att, D, L.proj.w, nullptr, S.x2, D, M, D, D, E_RESID, S.x, D, c.st));
    GRC(ln_fwd(c, S.x2, L.g2, L.b2, p.tA, M, D));
    GRC(linear_fwd(p.tA, D, L.fc1.w, L.fc1.b, S.hp, D, M, D, D, 0, nullptr, 0, c.st));
    LAUNCH1D(relu_kernel, M * D, S.hp, p.tB, M * D);
    return linear_fwd(p.tB, D, L.fc2.w, L.fc2.b, xo, D, M, D, D, E_RESID, S.x2, D, c.st);
}
// its backward: dxo (gradient at the layer's output) -> dxi (at its input; may be the same buffer), parameter gradients accumulated
int layer_bwd(const ttup_uplift* net, const Ctx& c, const Plan& p, const LayerP& L, const Saved& S, const float* dxo, float* dxi, const Stage& sg,
              int n_seq, const SeqView& sv) {
    const int D = net->D;
    const long long M = (long long)n_seq * sg.S;
    // fc2
    LAUNCH1D(relu_kernel, M * D, S.hp, p.tA, M * D);
    GRC(linear_dw(c, dxo, D, p.tA, D, M, D, D, L.fc2.gw, L.fc2.gb));
    GRC(linear_dx(dxo, D, L.fc2.w, p.tB, D, M, D, D, E_GATE, nullptr, 0, S.hp, D, c.st));               // tB = d hp
    // fc1 over LayerNorm 2
    GRC(ln_fwd(c, S.x2, L.g2, L.b2, p.tA, M, D));
    GRC(linear_dw(c, p.tB, D, p.tA, D, M, D, D, L.fc1.gw, L.fc1.gb));
    GRC(linear_dx(p.tB, D, L.fc1.w, p.tA, D, M, D, D, 0, nullptr, 0, nullptr, 0, c.st));                // tA = d LN2(x2)
    hipLaunchKernelGGL(ln_bwd_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, c.st, S.x2, L.g2, p.tA, dxo, p.tC, p.tE, M, D);      // tC = d x2
    TTUP_LAUNCH_CHECK();
    GRC(colsum_into(c, p.tE, D, M, D, L.dg2));
    GRC(colsum_into(c, p.tA, D, M, D, L.db2));
    // proj
    GRC(linear_dw(c, p.tC, D, S.att, D, M, D, D, L.proj.gw, nullptr));
    GRC(linear_dx(p.tC, D, L.proj.w, p.tA, D, M, D, D, 0, nullptr, 0, nullptr, 0, c.st));               // tA = d att
    AttnArgs a = {};
    a.qkv = S.qkv; a.sv = sv; a.o = S.att; a.d_o = p.tA; a.dqkv = p.tQ; a.n_seq = n_seq;
    GRC(run_attention<true>(net, a, c.st));
    // qkv over LayerNorm 1
    GRC(ln_fwd(c, S.x, L.g1, L.b1, p.tB, M, D));
    GRC(linear_dw(c, p.tQ, 3 * D, p.tB, D, M, 3 * D, D, L.qkv.gw, L.qkv.gb));
    GRC(linear_dx(p.tQ, 3 * D, L.qkv.w, p.tA, D, M, 3 * D, D, 0, nullptr, 0, nullptr, 0, c.st));        // tA = d LN1(x)
    hipLaunchKernelGGL(ln_bwd_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, c.st, S.x, L.g1, p.tA, p.tC, dxi, p.tE, M, D);
    TTUP_LAUNCH_CHECK();
    GRC(colsum_into(c, p.tE, D, M, D, L.dg1));
    return colsum_into(c, p.tA, D, M, D, L.db1);
}
int stage_fwd(const ttup_uplift* net, const Ctx& c, const Plan& p, const std::vector<LayerP>& W, const Stage& sg, int n_seq, const SeqView& sv) {
    for (size_t l = 0; l < W.size(); ++l)
        GRC(layer_fwd(net, c, p, W[l], sg.L[l], l + 1 < W.size() ? sg.L[l + 1].x : sg.out, sg, n_seq, sv));
    return TTUP_OK;
}
int stage_bwd(const ttup_uplift* net, const Ctx& c, const Plan& p, const std::vector<LayerP>& W, const Stage& sg, int n_seq, const SeqView& sv, float* dx) {
    for (size_t l = W.size(); l-- > 0;)
        GRC(layer_bwd(net, c, p, W[l], sg.L[l], dx, dx, sg, n_seq, sv));
    return TTUP_OK;
}
// MyHead (model.py:232-261): x (row stride ldx) -> out (M,3), keeping the two hidden activations
int head_fwd(const ttup_uplift* net, const Ctx& c, const HeadP& H, const float* x, int ldx, long long M, float* h1, float* h2, float* out) {
    const int D = net->D;
    GRC(linear_fwd(x, ldx, H.fc1.w, H.fc1.b, h1, D / 2, M, D / 2, D, E_RELU, nullptr, 0, c.st));
    GRC(linear_fwd(h1, D / 2, H.fc2.w, H.fc2.b, h2, D / 4, M, D / 4, D / 2, E_RELU, nullptr, 0, c.st));
    return linear_fwd(h2, D / 4, H.fc3.w, H.fc3.b, out, 3, M, 3, D / 4, 0, nullptr, 0, c.st);
}
// d_out (M,3) -> dx (M,D); t1 / t2 are scratch of M*D/2 and M*D/4 floats
int head_bwd(const ttup_uplift* net, const Ctx& c, const HeadP& H, const float* x, int ldx, long long M, const float* h1, const float* h2,
             const float* d_out, float* t1, float* t2, float* dx) {
    const int D = net->D;
    GRC(linear_dw(c, d_out, 3, h2, D / 4, M, 3, D / 4, H.fc3.gw, H.fc3.gb));
    GRC(linear_dx(d_out, 3, H.fc3.w, t2, D / 4, M, 3, D / 4, E_GATE, nullptr, 0, h2, D / 4, c.st));
    GRC(linear_dw(c, t2, D / 4, h1, D / 2, M, D / 4, D / 2, H.fc2.gw, H.fc2.gb));
    GRC(linear_dx(t2, D / 4, H.fc2.w, t1, D / 2, M, D / 4, D / 2, E_GATE, nullptr, 0, h1, D / 2, c.st));
    GRC(linear_dw(c, t1, D / 2, x, ldx, M, D / 2, D, H.fc1.gw, H.fc1.gb));
    return linear_dx(t1, D / 2, H.fc1.w, dx, D, M, D / 2, D, 0, nullptr, 0, nullptr, 0, c.st);
}
// the 2 -> D -> D embeddings (model.py:105-158): in (M,2) -> tok, keeping the hidden activation; and back (d_tok is overwritten)
int embed_fwd(const ttup_uplift* net, const Ctx& c, const LinP& f1, const LinP& f2, const float* in, long long M, float* h, float* tok) {
    const int D = net->D;
    GRC(linear_fwd(in, 2, f1.w, f1.b, h, D, M, D, 2, E_RELU, nullptr, 0, c.st));
    return linear_fwd(h, D, f2.w, f2.b, tok, D, M, D, D, 0, nullptr, 0, c.st);
}
int embed_bwd(const ttup_uplift* net, const Ctx& c, const LinP& f1, const LinP& f2, const float* in, long long M, const float* h, const float* d_tok, float* tmp) {
    const int D = net->D;
    GRC(linear_dw(c, d_tok, D, h, D, M, D, D, f2.gw, f2.gb));
    GRC(linear_dx(d_tok, D, f2.w, tmp, D, M, D, D, E_GATE, nullptr, 0, h, D, c.st));
    return linear_dw(c, tmp, D, in, 2, M, D, 2, f1.gw, f1.gb);
}

// forward, loss terms and backward of B trajectories (one group)
int group_pass(const ttup_uplift* net, const Ctx& c, const Plan& p, const Params& W, const float* ball, const float* table, const float* mask,
               const float* times, const float* r_world, const float* rotation, int B, int T, int flags, float* loss, float* rot, float* pos) {
    const int D = net->D, NT = net->n_table, S1 = NT + 1;
    const long long nt = (long long)B * T, n1 = nt * S1, n2 = (long long)B * (T + 1);
    if (flags & FLAG_CHECK_MASK)          // the same m1 / m2 / tmask / txy, plus the mask's value classes or-ed into the handle's flag word
        LAUNCH1D(prepare_kernel<true>, nt + (long long)B * NT, mask, table, p.m1, p.m2, p.tmask, p.txy, B, T, NT, net->flags_dev);
    else
        LAUNCH1D(prepare_kernel<false>, nt + (long long)B * NT, mask, table, p.m1, p.m2, p.tmask, p.txy, B, T, NT, (int*)nullptr);
    const float2* rope = net->rope_index;
    const int rope_stride = net->rot_old ? 0 : T;
    if (!net->rot_old) {
        const long long n = nt * (net->hd / 2);
        LAUNCH1D(rope_table_kernel, n, times, net->inv_freq_dev, (float2*)p.rope, net->hd / 2, n);
        rope = (const float2*)p.rope;
    }
    const float scale = 1.0f / sqrtf((float)net->hd);
    const SeqView q_table{p.tmask, net->table_rope, S1, 1, T, 1, 0, scale};
    const SeqView q_time{p.m1, rope, T, 0, 1, 1, rope_stride, scale}, q_spin{p.m2, rope, T + 1, 1, 1, 1, rope_stride, scale};
    // ---- forward
    GRC(embed_fwd(net, c, W.ball1, W.ball2, ball, nt, p.ball_h, p.ball_tok));
    GRC(embed_fwd(net, c, W.tab1, W.tab2, p.txy, (long long)B * NT, p.tab_h, p.tab_tok));
    LAUNCH1D(assemble_table_kernel, n1 * D, p.ball_tok, p.tab_tok, p.table.L[0].x, T, NT, D, n1 * D);
    GRC(stage_fwd(net, c, p, W.pos, p.table, (int)nt, q_table));
    LAUNCH1D(gather_rows_kernel, nt * D, p.table.out, p.temporal.L[0].x, D, S1, nt * D);
    GRC(stage_fwd(net, c, p, W.first, p.temporal, B, q_time));
    GRC(head_fwd(net, c, W.pos_head, p.temporal.out, D, nt, p.pos_h1, p.pos_h2, pos));
    LAUNCH1D(prepend_cls_kernel, n2 * D, p.temporal.out, W.cls, p.spin.L[0].x, T, D, n2 * D);
    GRC(stage_fwd(net, c, p, W.second, p.spin, B, q_spin));
    GRC(head_fwd(net, c, W.rot_head, p.spin.out, (T + 1) * D, B, p.rot_h1, p.rot_h2, rot));
    // ---- loss
    const float* target = rotation;
    if (flags & FLAG_LOCAL) {
        hipLaunchKernelGGL(rotationaxes_kernel, dim3(cdiv(B, 64)), dim3(64), 0, c.st, rotation, r_world, B, T, p.rot_t);
        TTUP_LAUNCH_CHECK();
        target = p.rot_t;
    }
    hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(1024), 0, c.st, rot, pos, target, r_world, mask, p.mask_sum, B, T, p.d_rot, p.d_pos, loss);
    TTUP_LAUNCH_CHECK();
    // ---- backward: rotation head <- cls rows of the spin stage
    GRC(head_bwd(net, c, W.rot_head, p.spin.out, (T + 1) * D, B, p.rot_h1, p.rot_h2, p.d_rot, p.tB, p.tC, p.tA));
    LAUNCH1D(expand_rows_kernel, n2 * D, p.tA, p.dX, D, T + 1, n2 * D);
    GRC(stage_bwd(net, c, p, W.second, p.spin, B, q_spin, p.dX));
    GRC(colsum_into(c, p.dX, (long long)(T + 1) * D, B, D, W.dcls));          // the cls token is broadcast over the batch
    // The spin stage's gradient stops at its input: the reference detaches the tokens it takes from the first stage (full_backprop is
    // False, model.py:553-555 -- "rotation computation should not influence position computations"), so only the cls rows of dX are
    // used and the position head's stream alone reaches the temporal stage.
    GRC(head_bwd(net, c, W.pos_head, p.temporal.out, D, nt, p.pos_h1, p.pos_h2, p.d_pos, p.tB, p.tC, p.dY));
    GRC(stage_bwd(net, c, p, W.first, p.temporal, B, q_time, p.dY));
    // table stage: only row 0 of every 14-token sequence went on
    LAUNCH1D(expand_rows_kernel, n1 * D, p.dY, p.dX, D, S1, n1 * D);
    GRC(stage_bwd(net, c, p, W.pos, p.table, (int)nt, q_table, p.dX));
    {
        const long long total = nt * D + (long long)B * NT * D;
        LAUNCH1D(assemble_bwd_kernel, total, p.dX, p.tA, p.tB, B, T, NT, D);
    }
    GRC(embed_bwd(net, c, W.ball1, W.ball2, ball, nt, p.ball_h, p.tA, p.tC));
    return embed_bwd(net, c, W.tab1, W.tab2, p.txy, (long long)B * NT, p.tab_h, p.tB, p.tC);
}

}  // namespace

extern "C" int ttup_uplift_grad_layout(ttup_uplift* net, long long* n_floats, int* n_tensors, long long* offsets_host, int* used_host, int capacity) {
    TTUP_REQUIRE(net && n_floats && n_tensors, TTUP_EINVAL, "ttup_uplift_grad_layout: null pointer");
    TTUP_REQUIRE(supported(net), TTUP_EINVAL, "ttup_uplift_grad_layout: gradients are served for connectstage/dynamic only, this handle holds %s", variant_text(net));
    const int D = net->D;
    std::vector<long long> sizes;
    std::vector<int> used;
    auto add = [&](long long n, int u = 1) { sizes.push_back(n); used.push_back(u); };
    auto mlp = [&](int din, int u = 1) { add((long long)D * din, u); add(D, u); add((long long)D * D, u); add(D, u); };
    auto layer = [&]() { add(3LL * D * D); add(3 * D); add((long long)D * D); add((long long)D * D); add(D); add((long long)D * D); add(D); add(D); add(D); add(D); add(D); };
    auto head = [&]() { add((long long)(D / 2) * D); add(D / 2); add((long long)(D / 4) * (D / 2)); add(D / 4); add(3LL * (D / 4)); add(3); };
    add(D); mlp(3, 0); mlp(2); mlp(2);
    for (size_t i = 0; i < net->pos_layers.size() + net->layers.size(); ++i) layer();
    head();
    for (size_t i = 0; i < net->second.size(); ++i) layer();
    head();
    long long off = 0;
    for (size_t i = 0; i < sizes.size(); ++i) {
        if (offsets_host && (int)i < capacity) offsets_host[i] = off;
        if (used_host && (int)i < capacity) used_host[i] = used[i];
        off += sizes[i];
    }
    *n_floats = off; *n_tensors = (int)sizes.size();
    return TTUP_OK;
}

extern "C" size_t ttup_uplift_grad_workspace_bytes(ttup_uplift* net, int batch, int len) {
    if (!net || batch <= 0 || len <= 0 || !supported(net)) return 0;
    Plan p;
    make_plan(net, batch, len, nullptr, &p);
    return (size_t)p.total * sizeof(float);
}

extern "C" int ttup_uplift_loss_grad(ttup_uplift* net, const float* ball_dev, const float* table_dev, const float* mask_dev, const float* times_dev,
                                     const float* r_world_dev, const float* rotation_dev, int batch, int len, int flags, void* workspace,
                                     size_t workspace_bytes, float* grad_dev, float* loss_dev, float* rot_dev, float* pos_dev, void* stream) {
    TTUP_REQUIRE(net && ball_dev && table_dev && mask_dev && times_dev && r_world_dev && rotation_dev && workspace && grad_dev && loss_dev && rot_dev && pos_dev,
                 TTUP_EINVAL, "ttup_uplift_loss_grad: null pointer");
    TTUP_REQUIRE(supported(net), TTUP_EINVAL, "ttup_uplift_loss_grad: gradients are served for connectstage/dynamic only, this handle holds %s", variant_text(net));
    TTUP_REQUIRE(batch > 0 && len > 0 && len <= 255, TTUP_EINVAL, "ttup_uplift_loss_grad: batch %d / sequence length %d outside [1,..] x [1,255]", batch, len);
    TTUP_REQUIRE((flags & ~(FLAG_LOCAL | FLAG_CHECK_MASK)) == 0, TTUP_EINVAL, "ttup_uplift_loss_grad: unknown flag bits %d", flags);
    TTUP_REQUIRE(!(flags & FLAG_LOCAL) || len >= 2, TTUP_EINVAL, "ttup_uplift_loss_grad: transform_mode 'local' needs at least two positions");
    TTUP_REQUIRE(!net->rot_old || len <= net->max_len, TTUP_EINVAL, "ttup_uplift_loss_grad: sequence length %d above the handle's %d", len, net->max_len);
    TTUP_REQUIRE(((size_t)workspace & 15) == 0, TTUP_EINVAL, "ttup_uplift_loss_grad: workspace must be 16-byte aligned");
    Plan p;
    make_plan(net, batch, len, (float*)workspace, &p);
    TTUP_REQUIRE(workspace_bytes >= (size_t)p.total * sizeof(float), TTUP_EINVAL, "ttup_uplift_loss_grad: workspace of %zu bytes, %zu needed", workspace_bytes,
                 (size_t)p.total * sizeof(float));
    Params W;
    map_params(net, grad_dev, &W);
    TTUP_REQUIRE(W.n_floats - embed_floats(net->D) == net->plain_floats, TTUP_EINVAL, "ttup_uplift_loss_grad: the handle's plain weights do not fit the layout");
    Ctx c{(hipStream_t)stream, p.partial};
    TTUP_HIP_CHECK(hipMemsetAsync(grad_dev, 0, (size_t)W.n_floats * sizeof(float), c.st));
    TTUP_HIP_CHECK(hipMemsetAsync(loss_dev, 0, 2 * sizeof(float), c.st));
    if (flags & FLAG_CHECK_MASK) TTUP_HIP_CHECK(hipMemsetAsync(net->flags_dev, 0, sizeof(int), c.st));
    hipLaunchKernelGGL(mask_sum_kernel, dim3(1), dim3(1024), 0, c.st, mask_dev, (long long)batch * len, p.mask_sum);
    TTUP_LAUNCH_CHECK();
    for (int b0 = 0; b0 < batch; b0 += p.G) {
        const int nb = batch - b0 < p.G ? batch - b0 : p.G;
        GRC(group_pass(net, c, p, W, ball_dev + (size_t)b0 * len * 2, table_dev + (size_t)b0 * net->n_table * 3, mask_dev + (size_t)b0 * len,
                       times_dev + (size_t)b0 * len, r_world_dev + (size_t)b0 * len * 3, rotation_dev + (size_t)b0 * 3, nb, len, flags, loss_dev,
                       rot_dev + (size_t)b0 * 3, pos_dev + (size_t)b0 * len * 3));
    }
    if (flags & FLAG_CHECK_MASK) {
        // as ttup_uplift_forward: the whole batch's mask must hold 0 and 1 and nothing else (mask.min() == 0 and mask.max() == 1,
        // model.py:541-546; the additive {-1e9, 0} form of the elif branch is not accepted).  The pass is already enqueued when the
        // answer is known, so a refused call has written its outputs: they hold no defined values.
        int seen = 0;
        TTUP_HIP_CHECK(hipMemcpyAsync(&seen, net->flags_dev, sizeof(int), hipMemcpyDeviceToHost, c.st));
        TTUP_HIP_CHECK(hipStreamSynchronize(c.st));
        TTUP_REQUIRE(seen == 3, TTUP_EMASK, "wrong format for masks. Should be 0, 1 or -1e9, 0.");
    }
    return TTUP_OK;
}

#include "no_packed_fp32_end.h"
