// ViTPose-small detector (balldetection/models/vitpose.py, tabledetection/models/vitpose.py over vit_pose/vit_models): patch
// embedding, 12 pre-LN transformer blocks, last_norm, two stride-2 deconvolutions + BN + ReLU, final 1x1 conv, then the argmax /
// 3x3 window of refine.hip.
//
// Arithmetic: fp32 throughout.  Every matrix product runs on v_mfma_f32_16x16x4_f32 (fp32 operands, fp32 accumulation: the same
// products and sums as an fmaf chain, MI355X_MICROARCH "f32-input MFMA"), so the only difference from the reference's fp32 CPU
// forward is the summation order.  A split-bf16 form on the bf16 matrix pipe (uplift.hip's linear_x3) keeps ~16 operand bits,
// which is short of this detector's accuracy bar.
//
// Kernels
//   gemm_kernel<AM>      (csrc/gemm_f32.h, shared with uplift_grad.hip)  C[m][n] = epilogue(sum_k A[m][k] W[n][k]), W row-major (nn.Linear layout).  64x64 block tile, BK = 32,
//                        4 waves of 32x32 (2x2 MFMA tiles), A and W tiles through LDS (row stride 36 floats: the MFMA operand
//                        reads -- 16 rows x 4 k per instruction -- hit 64 distinct banks).  A modes:
//                          A_DENSE  row-major activations;
//                          A_LN     the same through LayerNorm (row mean / rstd from ln_stats_kernel, gain + bias per k): the
//                                   LN prologue of qkv and fc1;
//                          A_PATCH  implicit im2col of the Conv2d(k16, s16, p2) patch embedding on the NCHW input;
//                          A_DECONV implicit 2x2 gather of one output phase of ConvTranspose2d(k4, s2, p1) on NHWC input;
//                          A_PATCH_FRAMES  A_PATCH on per-frame records (3, H, W): channel c of sample b is channel c % 3 of
//                                   record b + c / 3, so consecutive triples share their frames' records (forward_frames).
//                        Epilogue: + bias, then GELU (erf) | + residual | + pos_embed[1+tok] + pos_embed[0] | ReLU; rows go to
//                        a row-major output or, for a deconv phase, to pixel (2y+py, 2x+px) of the NHWC output.
//   ln_stats_kernel      one wave per token: mean and 1/sqrt(var + 1e-6) of 384 values (two-pass, in registers).
//   attention_kernel     flash-style, 32-dim heads, 64 queries per workgroup (16 per wave), K/V tiles of 64 keys through LDS,
//                        online softmax; scores are computed transposed (S^T = K Q^T) so that a lane holds 16 keys of ONE query:
//                        the row max / sum is 15 in-lane ops + 2 cross-lane steps, and P^T in that layout is directly the B
//                        operand of O^T += V^T P^T (the k-order of the product is permuted, the sum is the same).  No N x N matrix.
//   conv1x1_kernel       the final 1x1 conv (256 -> C_out, + bias) from NHWC to the NCHW heatmap, 64 pixels per workgroup staged in
//                        LDS.  It is not fused into deconv 2: a deconv tile holds 64 of the 256 channels the 1x1 reduces over.
#include "no_packed_fp32_begin.h"      // this unit runs beside the CNN's chain kernels: no packed fp32 (common.h)
#include "common.h"
#include "wasb_net.h"
#include "gemm_f32.h"

#include <cstring>
#include <vector>

#define VITPOSE_MAGIC_STR "TTUPVIT1"

namespace ttup {
namespace vit {

using namespace ttup::gemm;

constexpr int DIM = 384, HEADS = 12, HD = 32, MLP = 1536, DEC = 256, DEPTH = 12;

}  // namespace vit
}  // namespace ttup
#include "vitpose_bf16.h"
namespace ttup {
namespace vit {

// one wave per row of DIM floats -> (mean, 1/sqrt(var + eps)), eps 1e-6 (vit.py:274)
__global__ __launch_bounds__(256) void ln_stats_kernel(const float* __restrict__ x, int M, float* __restrict__ stats) {
    const int row = ttup_bid_x() * 4 + (ttup_tid_x() >> 6), lane = ttup_tid_x() & 63;
    if (row >= M) return;
    const float* r = x + (size_t)row * DIM;
    float v[DIM / 64];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < DIM / 64; ++i) { v[i] = r[lane + 64 * i]; s += v[i]; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    const float mu = s * (1.0f / DIM);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < DIM / 64; ++i) { const float d = v[i] - mu; q += d * d; }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) q += __shfl_xor(q, off, 64);
    if (lane == 0) {
        stats[2 * row] = mu;
        stats[2 * row + 1] = 1.0f / sqrtf(q * (1.0f / DIM) + 1e-6f);
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

// x: NHWC (B, H, W, DEC) -> heat (B, cout, H, W) = w (cout, DEC) x + bias; 64 pixels per workgroup
__global__ __launch_bounds__(256) void conv1x1_kernel(const float* __restrict__ x, long long npix, int hw, const float* __restrict__ w,
                                                      const float* __restrict__ bias, int cout, float* __restrict__ heat) {
    __shared__ float sx[64 * (64 + 1)];
    const int tid = ttup_tid_x();
    const long long p0 = (long long)ttup_bid_x() * 64;
    const int pl = tid & 63, cg = tid >> 6;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};          // output channels cg, cg+4, cg+8, cg+12
    for (int c0 = 0; c0 < DEC; c0 += 64) {
        for (int e = tid; e < 64 * 64; e += 256) {
            const int pp = e >> 6, c = e & 63;
            sx[pp * 65 + c] = p0 + pp < npix ? x[(size_t)(p0 + pp) * DEC + c0 + c] : 0.f;
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

// last_norm applied once: out[m][k] = (x[m][k] - mean) * rstd * g[k] + b[k], one quad per thread
__global__ __launch_bounds__(256) void ln_apply_kernel(GemmArgs p) {
    const long long e = (long long)ttup_bid_x() * 256 + ttup_tid_x();
    if (e >= (long long)p.M * (DIM / 4)) return;
    const int m = (int)(e / (DIM / 4)), k = (int)(e - (long long)m * (DIM / 4)) * 4;
    *(f32x4*)(p.out + (size_t)m * DIM + k) = load_a4<A_LN>(p, m, k);
}

struct Block {
    const float *n1w, *n1b, *qkvw, *qkvb, *projw, *projb, *n2w, *n2b, *fc1w, *fc1b, *fc2w, *fc2b;
};

}  // namespace vit
}  // namespace ttup

using namespace ttup;
using namespace ttup::vit;

struct ttup_vitpose {
    int H, W, hp, wp, ntok, in_ch, out_ch, max_batch, micro;
    float* weights = nullptr;                   // every tensor of the blob (after the header), device copy
    const float *pos, *patch_w, *patch_b, *lnw, *lnb, *dc_w[2], *dc_b[2], *fin_w, *fin_b;
    Block blk[DEPTH];
    int dtype = 0;                              // 0: fp32 path; 1: bf16 path
    bf16_t* w16 = nullptr;                      // bf16 handle: the blob rounded to bf16, same offsets as `weights`
    // qkv, att, hid and d2 hold bf16 in a bf16 handle (half the bytes), fp32 otherwise; x, stats and heat are fp32 in both
    float *x = nullptr, *stats = nullptr, *qkv = nullptr, *att = nullptr, *hid = nullptr, *d2 = nullptr, *heat = nullptr;
    // ttup_vitpose_run_stage / read_tap: the stage that ran last (-1: none) and its batch, and the residual stream after the
    // attention half of a block (x itself goes on to the MLP half), allocated on first use
    int tap_stage = -1, tap_batch = 0;
    float* x_attn = nullptr;
    double* stats64 = nullptr;                  // bf16 handle: (M, 2) LN mean, rstd in fp64
    float* frames = nullptr;                    // forward_frames: fp32 (3, H, W) records of one micro-batch's frames
    void* ws = nullptr;
    size_t ws_bytes = 0;
};

static void vitpose_free(ttup_vitpose* n) {
    for (void* p : {(void*)n->weights, (void*)n->w16, (void*)n->x_attn, (void*)n->stats64, (void*)n->x, (void*)n->stats, (void*)n->qkv, (void*)n->att, (void*)n->hid, (void*)n->d2,
                    (void*)n->heat, (void*)n->frames, n->ws})
        if (p) (void)hipFree(p);
    delete n;
}

extern "C" int ttup_vitpose_create_dtype(const void* blob, size_t blob_bytes, int height, int width, int max_batch, int micro_batch,
                                         int in_ch, int out_ch, int dtype, ttup_vitpose** out) {
    TTUP_REQUIRE(out && blob, TTUP_EINVAL, "ttup_vitpose_create: null argument");
    *out = nullptr;
    TTUP_REQUIRE(dtype == 0 || dtype == 1, TTUP_EINVAL, "ttup_vitpose_create: dtype %d is neither 0 (f32) nor 1 (bf16)", dtype);
    TTUP_REQUIRE(height >= 16 && width >= 16 && height % 16 == 0 && width % 16 == 0, TTUP_EINVAL,
                 "ttup_vitpose_create: height and width must be positive multiples of 16 (got %dx%d)", height, width);
    TTUP_REQUIRE(max_batch >= 1 && micro_batch >= 0 && in_ch >= 1 && out_ch >= 1 && out_ch <= 16, TTUP_EINVAL,
                 "ttup_vitpose_create: bad max_batch %d / micro_batch %d / in_ch %d / out_ch %d (1..16)", max_batch, micro_batch, in_ch, out_ch);
    const int ntok = (height / 16) * (width / 16);
    TTUP_REQUIRE(blob_bytes >= 8 + 32 && memcmp(blob, VITPOSE_MAGIC_STR, 8) == 0, TTUP_EFORMAT, "ttup_vitpose_create: not a ViTPose blob");
    int hdr[8];
    memcpy(hdr, (const char*)blob + 8, sizeof hdr);
    TTUP_REQUIRE(hdr[0] == in_ch && hdr[1] == out_ch, TTUP_EFORMAT, "ttup_vitpose_create: blob has in_ch %d / out_ch %d, asked for %d / %d",
                 hdr[0], hdr[1], in_ch, out_ch);
    TTUP_REQUIRE(hdr[2] == DIM && hdr[3] == DEPTH && hdr[4] == HEADS && hdr[5] == MLP && hdr[6] == DEC, TTUP_EFORMAT,
                 "ttup_vitpose_create: only ViTPose-small (384 / 12 / 12 / 1536 / 256) is built");
    TTUP_REQUIRE(hdr[7] == ntok + 1, TTUP_EFORMAT, "ttup_vitpose_create: pos_embed has %d rows, a %dx%d input needs %d", hdr[7], height, width, ntok + 1);
    // float counts in blob order (include/ttup.h)
    std::vector<size_t> sizes = {(size_t)hdr[7] * DIM, (size_t)DIM * in_ch * 256, DIM};
    for (int i = 0; i < DEPTH; ++i)
        for (size_t s : {(size_t)DIM, (size_t)DIM, (size_t)3 * DIM * DIM, (size_t)3 * DIM, (size_t)DIM * DIM, (size_t)DIM, (size_t)DIM, (size_t)DIM,
                         (size_t)MLP * DIM, (size_t)MLP, (size_t)DIM * MLP, (size_t)DIM})
            sizes.push_back(s);
    for (size_t s : {(size_t)DIM, (size_t)DIM, (size_t)4 * DEC * 4 * DIM, (size_t)DEC, (size_t)4 * DEC * 4 * DEC, (size_t)DEC, (size_t)out_ch * DEC, (size_t)out_ch})
        sizes.push_back(s);
    size_t total = 0;
    for (size_t s : sizes) total += s;
    TTUP_REQUIRE(blob_bytes == 40 + total * 4, TTUP_EFORMAT, "ttup_vitpose_create: blob has %zu bytes, expected %zu", blob_bytes, 40 + total * 4);

    ttup_vitpose* n = new ttup_vitpose();
    n->H = height; n->W = width; n->hp = height / 16; n->wp = width / 16; n->ntok = ntok;
    n->in_ch = in_ch; n->out_ch = out_ch; n->max_batch = max_batch; n->dtype = dtype;
    n->micro = micro_batch ? (micro_batch < max_batch ? micro_batch : max_batch) : (max_batch < 8 ? max_batch : 8);
    auto fail = [&](int rc) { vitpose_free(n); return rc; };
#define VP_CHECK(expr) do { if ((expr) != hipSuccess) { ttup::set_error("%s failed (%s:%d)", #expr, __FILE__, __LINE__); return fail(TTUP_EHIP); } } while (0)
    VP_CHECK(hipMalloc((void**)&n->weights, total * 4));
    VP_CHECK(hipMemcpy(n->weights, (const char*)blob + 40, total * 4, hipMemcpyHostToDevice));
    // Every tensor rounded once (RNE); the path reads the matrix weights from here and everything else from `weights`.  Rounding the
    // whole blob keeps one offset table for both (a tensor's bf16 copy sits at its fp32 offset: launch_gemm) at the price of memory
    // that is never read -- the bf16 copies of biases, LN parameters, pos_embed and the final conv (under 1 % of the blob) and the fp32
    // copies of the matrix weights: 1.5 x the fp32 handle's weight memory (about 140 MB instead of 95 MB).  Deliberate.
    if (dtype == 1) {
        std::vector<bf16_t> w16(total);
        const float* src = (const float*)((const char*)blob + 40);
        for (size_t i = 0; i < total; ++i) w16[i] = f32_to_bf16(src[i]);
        VP_CHECK(hipMalloc((void**)&n->w16, total * 2));
        VP_CHECK(hipMemcpy(n->w16, w16.data(), total * 2, hipMemcpyHostToDevice));
    }
    const float* p = n->weights;
    size_t k = 0;
    auto next = [&]() { const float* r = p; p += sizes[k++]; return r; };
    n->pos = next(); n->patch_w = next(); n->patch_b = next();
    for (int i = 0; i < DEPTH; ++i) {
        Block& b = n->blk[i];
        b.n1w = next(); b.n1b = next(); b.qkvw = next(); b.qkvb = next(); b.projw = next(); b.projb = next();
        b.n2w = next(); b.n2b = next(); b.fc1w = next(); b.fc1b = next(); b.fc2w = next(); b.fc2b = next();
    }
    n->lnw = next(); n->lnb = next();
    n->dc_w[0] = next(); n->dc_b[0] = next(); n->dc_w[1] = next(); n->dc_b[1] = next();
    n->fin_w = next(); n->fin_b = next();
    const size_t M = (size_t)n->micro * ntok, esz = dtype == 1 ? 2 : 4;
    VP_CHECK(hipMalloc((void**)&n->x, M * DIM * 4));
    VP_CHECK(hipMalloc((void**)&n->stats, M * 2 * 4));
    if (dtype == 1) VP_CHECK(hipMalloc((void**)&n->stats64, M * 2 * 8));
    VP_CHECK(hipMalloc((void**)&n->qkv, M * 3 * DIM * esz));
    VP_CHECK(hipMalloc((void**)&n->att, M * DIM * esz));
    VP_CHECK(hipMalloc((void**)&n->hid, M * MLP * esz));        // also deconv 1's output (M * 4 * DEC <= M * MLP)
    VP_CHECK(hipMalloc((void**)&n->d2, M * 16 * DEC * esz));
    VP_CHECK(hipMalloc((void**)&n->heat, M * 16 * out_ch * 4));
    if (in_ch % 3 == 0)          // one micro-batch of samples spans micro + in_ch / 3 - 1 frames
        VP_CHECK(hipMalloc((void**)&n->frames, (size_t)(n->micro + in_ch / 3 - 1) * 3 * height * width * 4));
    n->ws_bytes = ttup_refine_workspace_bytes(n->micro * out_ch, height / 4, width / 4);
    VP_CHECK(hipMalloc(&n->ws, n->ws_bytes));
#undef VP_CHECK
    *out = n;
    return TTUP_OK;
}

extern "C" int ttup_vitpose_create(const void* blob, size_t blob_bytes, int height, int width, int max_batch, int micro_batch,
                                   int in_ch, int out_ch, ttup_vitpose** out) {
    return ttup_vitpose_create_dtype(blob, blob_bytes, height, width, max_batch, micro_batch, in_ch, out_ch, 0, out);
}

extern "C" void ttup_vitpose_destroy(ttup_vitpose* net) {
    if (net) vitpose_free(net);
}

extern "C" int ttup_vitpose_micro_batch(ttup_vitpose* net) { return net ? net->micro : -1; }

// One GEMM of the handle's path.  fp32 handle: gemm_kernel on g as it stands.  bf16 handle: gemm_bf16_kernel with the weight read
// from w16 at g.w's offset, the A_DENSE / A_DECONV input (g.a) read as bf16, and the output (g.out) written as bf16 when out_bf16.
template <int AM>
static int launch_gemm(const ttup_vitpose* n, const GemmArgs& a, bool out_bf16, hipStream_t st) {
    if (n->dtype == 0) {
        TTUP_REQUIRE(a.N % BN == 0 && a.K % BK == 0, TTUP_EINVAL, "vitpose gemm: N %d / K %d not multiples of %d / %d", a.N, a.K, BN, BK);
        hipLaunchKernelGGL(gemm_kernel<AM>, dim3(cdiv(a.M, BM), a.N / BN), dim3(256), 0, st, a);
        TTUP_LAUNCH_CHECK();
        return TTUP_OK;
    }
    TTUP_REQUIRE(a.N % TN == 0 && a.K % TK == 0, TTUP_EINVAL, "vitpose bf16 gemm: N %d / K %d not multiples of %d / %d", a.N, a.K, TN, TK);
    Gemm16Args p = {};
    p.g = a;
    p.a16 = (const bf16_t*)a.a;
    p.w16 = n->w16 + (a.w - n->weights);
    p.out16 = out_bf16 ? (bf16_t*)a.out : nullptr;
    p.stats64 = n->stats64;
    hipLaunchKernelGGL(gemm_bf16_kernel<AM>, dim3(cdiv(a.M, TM), a.N / TN), dim3(256), 0, st, p);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

#define VP_RC(expr) do { int _rc = (expr); if (_rc != TTUP_OK) return _rc; } while (0)

static GemmArgs gemm_args(const float* a, const float* w, const float* bias, float* out, int M, int N, int K, int flags) {
    GemmArgs g = {};
    g.a = a; g.w = w; g.bias = bias; g.out = out; g.M = M; g.N = N; g.K = K; g.flags = flags;
    return g;
}

static int ln_stats(const ttup_vitpose* n, int M, hipStream_t st) {
    if (n->dtype == 0) hipLaunchKernelGGL(ln_stats_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, n->x, M, n->stats);
    else hipLaunchKernelGGL(ln_stats64_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, n->x, M, n->stats64);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// patch embedding + bias + pos_embed[1:] + pos_embed[:1]  (vit.py:222, :366): x_in (nb, in_ch, H, W), or with from_frames the samples'
// per-frame records (A_PATCH_FRAMES), -> the residual stream x
static int run_patch(ttup_vitpose* n, const float* x_in, int nb, hipStream_t st, bool from_frames) {
    GemmArgs g = gemm_args(x_in, n->patch_w, n->patch_b, n->x, nb * n->ntok, DIM, n->in_ch * 256, E_POS);
    g.cin = n->in_ch; g.ih = n->H; g.iw = n->W; g.pos = n->pos; g.ntok = n->ntok;
    return from_frames ? launch_gemm<A_PATCH_FRAMES>(n, g, false, st) : launch_gemm<A_PATCH>(n, g, false, st);
}

// one transformer block on the residual stream x; x_attn, when given, receives x as it stands between the two halves
static int run_block(ttup_vitpose* n, int i, int nb, hipStream_t st, float* x_attn = nullptr) {
    const int M = nb * n->ntok;
    const Block& b = n->blk[i];
    // x = x + proj(attn(norm1(x)))
    VP_RC(ln_stats(n, M, st));
    GemmArgs g = gemm_args(n->x, b.qkvw, b.qkvb, n->qkv, M, 3 * DIM, DIM, 0);
    g.ln_g = b.n1w; g.ln_b = b.n1b; g.stats = n->stats;
    VP_RC(launch_gemm<A_LN>(n, g, true, st));
    if (n->dtype == 0)
        hipLaunchKernelGGL(attention_kernel, dim3(cdiv(n->ntok, AQ), HEADS, nb), dim3(256), 0, st, n->qkv, n->ntok, 1.0f / sqrtf((float)HD), n->att);
    else
        hipLaunchKernelGGL(attention_bf16_kernel, dim3(cdiv(n->ntok, 64), HEADS, nb), dim3(256), 0, st, (const bf16_t*)n->qkv, n->ntok,
                           1.0f / sqrtf((float)HD), (bf16_t*)n->att);
    TTUP_LAUNCH_CHECK();
    g = gemm_args(n->att, b.projw, b.projb, n->x, M, DIM, DIM, E_RESID);
    g.res = n->x;
    VP_RC(launch_gemm<A_DENSE>(n, g, false, st));
    if (x_attn) TTUP_HIP_CHECK(hipMemcpyAsync(x_attn, n->x, (size_t)M * DIM * 4, hipMemcpyDeviceToDevice, st));
    // x = x + fc2(gelu(fc1(norm2(x))))
    VP_RC(ln_stats(n, M, st));
    g = gemm_args(n->x, b.fc1w, b.fc1b, n->hid, M, MLP, DIM, E_GELU);
    g.ln_g = b.n2w; g.ln_b = b.n2b; g.stats = n->stats;
    VP_RC(launch_gemm<A_LN>(n, g, true, st));
    g = gemm_args(n->hid, b.fc2w, b.fc2b, n->x, M, DIM, MLP, E_RESID);
    g.res = n->x;
    return launch_gemm<A_DENSE>(n, g, false, st);
}

// the head on the residual stream x: last_norm, the two deconvolutions, the final 1x1 conv -> heat (nb, out_ch, H/4, W/4)
static int run_head(ttup_vitpose* n, int nb, float* heat, hipStream_t st) {
    const int M = nb * n->ntok;
    // last_norm: materialised once (deconv 1 gathers every token four times per phase)
    VP_RC(ln_stats(n, M, st));
    {
        GemmArgs d = gemm_args(n->x, nullptr, nullptr, n->att, M, DIM, DIM, 0);
        d.ln_g = n->lnw; d.ln_b = n->lnb; d.stats = n->stats;
        if (n->dtype == 0) hipLaunchKernelGGL(ln_apply_kernel, dim3(cdiv(M * (DIM / 4), 256)), dim3(256), 0, st, d);
        else hipLaunchKernelGGL(ln_apply_bf16_kernel, dim3(cdiv(M * (DIM / 8), 256)), dim3(256), 0, st, d, (const double*)n->stats64, (bf16_t*)n->att);
        TTUP_LAUNCH_CHECK();
    }
    // deconvolutions: four 2x2 phase GEMMs each, BN folded, ReLU; NHWC (nb, hp, wp, 384) -> (nb, 2hp, 2wp, 256) -> (nb, 4hp, 4wp, 256)
    const float* din = n->att;
    float* douts[2] = {n->hid, n->d2};
    int h = n->hp, w = n->wp, cin = DIM;
    for (int l = 0; l < 2; ++l) {
        for (int ph = 0; ph < 4; ++ph) {
            GemmArgs d = gemm_args(din, n->dc_w[l] + (size_t)ph * DEC * 4 * cin, n->dc_b[l], douts[l], nb * h * w, DEC, 4 * cin, E_RELU);
            d.cin = cin; d.ih = h; d.iw = w; d.py = ph >> 1; d.px = ph & 1;
            VP_RC(launch_gemm<A_DECONV>(n, d, true, st));
        }
        din = douts[l]; h *= 2; w *= 2; cin = DEC;
    }
    const long long npix = (long long)nb * h * w;
    if (n->dtype == 0)
        hipLaunchKernelGGL(conv1x1_kernel, dim3((unsigned)((npix + 63) / 64)), dim3(256), 0, st, n->d2, npix, h * w, n->fin_w, n->fin_b, n->out_ch, heat);
    else
        hipLaunchKernelGGL(conv1x1_bf16_kernel, dim3((unsigned)((npix + 63) / 64)), dim3(256), 0, st, (const bf16_t*)n->d2, npix, h * w, n->fin_w,
                           n->fin_b, n->out_ch, heat);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// one micro-batch of nb samples: x (nb, in_ch, H, W) -> heat (nb, out_ch, H/4, W/4); with from_frames x holds the samples'
// per-frame records instead (A_PATCH_FRAMES)
static int vitpose_run(ttup_vitpose* n, const float* x_in, int nb, float* heat, hipStream_t st, bool from_frames = false) {
    n->tap_stage = -1;
    VP_RC(run_patch(n, x_in, nb, st, from_frames));
    for (int i = 0; i < DEPTH; ++i) VP_RC(run_block(n, i, nb, st));
    return run_head(n, nb, heat, st);
}

// The testing seam: one stage alone on a given input, and what it left in the handle's buffers.
extern "C" int ttup_vitpose_run_stage(ttup_vitpose* net, int stage, const float* in_dev, int batch, void* stream) {
    TTUP_REQUIRE(net && in_dev, TTUP_EINVAL, "ttup_vitpose_run_stage: null handle or input");
    TTUP_REQUIRE(stage >= 0 && stage <= DEPTH + 1, TTUP_EINVAL, "ttup_vitpose_run_stage: stage %d outside 0..%d", stage, DEPTH + 1);
    TTUP_REQUIRE(batch >= 1 && batch <= net->micro, TTUP_EINVAL, "ttup_vitpose_run_stage: batch %d outside 1..%d (the micro-batch)", batch, net->micro);
    TTUP_REQUIRE(((uintptr_t)in_dev & 15) == 0, TTUP_EINVAL, "ttup_vitpose_run_stage: input must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t xbytes = (size_t)batch * net->ntok * DIM * 4;
    net->tap_stage = -1;
    if (stage == 0) {
        VP_RC(run_patch(net, in_dev, batch, st, false));
    } else {
        TTUP_HIP_CHECK(hipMemcpyAsync(net->x, in_dev, xbytes, hipMemcpyDeviceToDevice, st));
        if (stage <= DEPTH) {
            if (!net->x_attn) TTUP_HIP_CHECK(hipMalloc((void**)&net->x_attn, (size_t)net->micro * net->ntok * DIM * 4));
            VP_RC(run_block(net, stage - 1, batch, st, net->x_attn));
        } else {
            VP_RC(run_head(net, batch, net->heat, st));
        }
    }
    net->tap_stage = stage; net->tap_batch = batch;
    return TTUP_OK;
}

extern "C" int ttup_vitpose_read_tap(ttup_vitpose* net, const char* tap, void* dst, size_t bytes) {
    TTUP_REQUIRE(net && tap && dst, TTUP_EINVAL, "ttup_vitpose_read_tap: null argument");
    TTUP_REQUIRE(net->tap_stage >= 0, TTUP_EINVAL, "ttup_vitpose_read_tap: no stage has run since the last forward");
    const int s = net->tap_stage;
    const bool blk = s >= 1 && s <= DEPTH, head = s == DEPTH + 1;
    const size_t M = (size_t)net->tap_batch * net->ntok, esz = net->dtype == 1 ? 2 : 4;
    // name, written by this stage, buffer, elements, element size
    const struct { const char* name; bool ok; const void* buf; size_t count, size; } taps[] = {
        {"x_attn", blk, net->x_attn, M * DIM, 4}, {"x", s == 0 || blk, net->x, M * DIM, 4},
        {"qkv", blk, net->qkv, M * 3 * DIM, esz}, {"att", blk, net->att, M * DIM, esz}, {"hid", blk, net->hid, M * MLP, esz},
        {"ln", head, net->att, M * DIM, esz}, {"d1", head, net->hid, M * 4 * DEC, esz}, {"d2", head, net->d2, M * 16 * DEC, esz},
        {"heat", head, net->heat, M * 16 * net->out_ch, 4}};
    for (const auto& t : taps) {
        if (strcmp(tap, t.name) != 0) continue;
        TTUP_REQUIRE(t.ok, TTUP_EINVAL, "ttup_vitpose_read_tap: stage %d does not write tap '%s'", s, tap);
        TTUP_REQUIRE(bytes == t.count * t.size, TTUP_EINVAL, "ttup_vitpose_read_tap: tap '%s' has %zu bytes, the buffer %zu", tap, t.count * t.size, bytes);
        TTUP_HIP_CHECK(hipDeviceSynchronize());          // whatever stream the stage ran on, and whether it still exists
        TTUP_HIP_CHECK(hipMemcpy(dst, t.buf, bytes, hipMemcpyDefault));
        return TTUP_OK;
    }
    ttup::set_error("ttup_vitpose_read_tap: unknown tap '%s'", tap);
    return TTUP_EINVAL;
}

extern "C" int ttup_vitpose_forward(ttup_vitpose* net, const float* x_dev, int batch, float* heat_dev, int64_t* argmax_dev,
                                    float* win_dev, void* stream) {
    TTUP_REQUIRE(net && x_dev, TTUP_EINVAL, "ttup_vitpose_forward: null handle or input");
    TTUP_REQUIRE(batch >= 0 && batch <= net->max_batch, TTUP_EINVAL, "ttup_vitpose_forward: batch %d outside 0..%d", batch, net->max_batch);
    TTUP_REQUIRE((argmax_dev == nullptr) == (win_dev == nullptr), TTUP_EINVAL, "ttup_vitpose_forward: argmax and window outputs go together");
    TTUP_REQUIRE(((uintptr_t)x_dev & 15) == 0, TTUP_EINVAL, "ttup_vitpose_forward: input must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int hh = net->H / 4, ww = net->W / 4, co = net->out_ch;
    const size_t in_per = (size_t)net->in_ch * net->H * net->W, heat_per = (size_t)co * hh * ww;
    for (int b0 = 0; b0 < batch; b0 += net->micro) {
        const int nb = batch - b0 < net->micro ? batch - b0 : net->micro;
        float* heat = heat_dev ? heat_dev + b0 * heat_per : net->heat;
        VP_RC(vitpose_run(net, x_dev + b0 * in_per, nb, heat, st));
        if (argmax_dev)
            VP_RC(refine_argmax(heat, nb * co, hh, ww, (long long*)argmax_dev + (size_t)b0 * co, win_dev + (size_t)b0 * co * 9, net->ws,
                                net->ws_bytes, st));
    }
    return TTUP_OK;
}

// n_frames BGR uint8 HWC frames (device, any size) -> the outputs of ttup_vitpose_forward on ttup_preprocess_triples (in_ch 9) or
// ttup_preprocess_frames (in_ch 3) of them, bit for bit: each micro-batch's frames are pre-processed once into fp32 records (the
// same launch_preprocess) and the patch embedding gathers its triples from them.
extern "C" int ttup_vitpose_forward_frames(ttup_vitpose* net, const uint8_t* frames_dev, int n_frames, int src_h, int src_w,
                                           float* heat_dev, int64_t* argmax_dev, float* win_dev, void* stream) {
    TTUP_REQUIRE(net && frames_dev, TTUP_EINVAL, "ttup_vitpose_forward_frames: null handle or frames");
    TTUP_REQUIRE(net->frames, TTUP_EINVAL, "ttup_vitpose_forward_frames: in_ch %d is not a whole number of BGR frames", net->in_ch);
    TTUP_REQUIRE(src_h > 0 && src_w > 0, TTUP_EINVAL, "ttup_vitpose_forward_frames: bad frame size %dx%d", src_h, src_w);
    const int nf = net->in_ch / 3;
    TTUP_REQUIRE(n_frames >= nf, TTUP_EINVAL, "ttup_vitpose_forward_frames: %d frames, a %d-channel sample needs at least %d", n_frames,
                 net->in_ch, nf);
    const int batch = n_frames - nf + 1;
    TTUP_REQUIRE(batch <= net->max_batch, TTUP_EINVAL, "ttup_vitpose_forward_frames: %d samples, the handle takes at most %d", batch, net->max_batch);
    TTUP_REQUIRE((argmax_dev == nullptr) == (win_dev == nullptr), TTUP_EINVAL, "ttup_vitpose_forward_frames: argmax and window outputs go together");
    hipStream_t st = (hipStream_t)stream;
    const int hh = net->H / 4, ww = net->W / 4, co = net->out_ch;
    const size_t heat_per = (size_t)co * hh * ww;
    for (int b0 = 0; b0 < batch; b0 += net->micro) {
        const int nb = batch - b0 < net->micro ? batch - b0 : net->micro;
        // records of frames b0 .. b0 + nb + nf - 2 (<= micro + nf - 1 of them: the workspace)
        VP_RC(launch_preprocess(frames_dev, n_frames, src_h, src_w, net->H, net->W, net->frames, TTUP_LAYOUT_NCHW_F32, TTUP_DTYPE_F32, b0,
                                nb + nf - 1, 1, st));
        float* heat = heat_dev ? heat_dev + b0 * heat_per : net->heat;
        VP_RC(vitpose_run(net, net->frames, nb, heat, st, true));
        if (argmax_dev)
            VP_RC(refine_argmax(heat, nb * co, hh, ww, (long long*)argmax_dev + (size_t)b0 * co, win_dev + (size_t)b0 * co * 9, net->ws,
                                net->ws_bytes, st));
    }
    return TTUP_OK;
}
#include "no_packed_fp32_end.h"
