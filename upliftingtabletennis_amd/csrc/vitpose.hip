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
//   ln_stats_kernel, attention_kernel, ln_apply_kernel, conv1x1_kernel and their bf16-path counterparts: csrc/vitpose_kernels.h.
// The host's decisions (blob layout, buffers, the list of GEMMs, taps) are csrc/vitpose_plan.h; this unit is the driver.
#include "no_packed_fp32_begin.h"      // this unit runs beside the CNN's chain kernels: no packed fp32 (common.h)
#include "common.h"
#include "wasb_net.h"
#include "vitpose_kernels.h"

#include <cstring>
#include <vector>

using namespace ttup;
using namespace ttup::vit;

struct ttup_vitpose {
    int H, W, hp, wp, ntok, in_ch, out_ch, max_batch, micro;
    int dtype = 0;                              // 0: fp32 path; 1: bf16 path
    BlobLayout blob;                            // where every tensor lies in `weights` and `w16` (floats)
    float* weights = nullptr;                   // every tensor of the blob (after the header), device copy
    bf16_t* w16 = nullptr;                      // bf16 handle: the blob rounded to bf16
    // One micro-batch's activations and workspaces (plan_buffers).  qkv, att, hid and d2 hold bf16 in a bf16 handle (half the
    // bytes), fp32 otherwise; x, stats and heat are fp32 in both.
    BufferPlan plan;
    char* arena = nullptr;
    // ttup_vitpose_run_stage / read_tap: the stage that ran last (-1: none) and its batch, and the residual stream after the
    // attention half of a block (x itself goes on to the MLP half), allocated on first use
    int tap_stage = -1, tap_batch = 0;
    float* x_attn = nullptr;

    template <class T = float> T* buf(int b) const { return b == B_XATTN ? (T*)x_attn : plan.bytes[b] ? (T*)(arena + plan.off[b]) : nullptr; }
};

static void vitpose_free(ttup_vitpose* n) {
    for (void* p : {(void*)n->weights, (void*)n->w16, (void*)n->arena, (void*)n->x_attn})
        if (p) (void)hipFree(p);
    delete n;
}

extern "C" int ttup_vitpose_create_dtype(const void* blob, size_t blob_bytes, int height, int width, int max_batch, int micro_batch,
                                         int in_ch, int out_ch, int dtype, ttup_vitpose** out) {
    TTUP_REQUIRE(out && blob, TTUP_EINVAL, "ttup_vitpose_create: null argument");
    *out = nullptr;
    TTUP_REQUIRE(dtype == 0 || dtype == 1, TTUP_EINVAL, "ttup_vitpose_create: dtype %d is neither 0 (f32) nor 1 (bf16)", dtype);
    const Refusal r = check_create(blob, blob_bytes, height, width, max_batch, micro_batch, in_ch, out_ch);
    TTUP_REQUIRE(r.rc == TTUP_OK, r.rc, "%s", r.msg);

    ttup_vitpose* n = new ttup_vitpose();
    n->H = height; n->W = width; n->hp = height / 16; n->wp = width / 16; n->ntok = n->hp * n->wp;
    n->in_ch = in_ch; n->out_ch = out_ch; n->max_batch = max_batch; n->dtype = dtype;
    n->micro = vit::micro_batch(max_batch, micro_batch);
    n->blob = blob_layout(in_ch, out_ch, n->ntok + 1);
    n->plan = plan_buffers(height, width, in_ch, out_ch, n->micro, dtype, ttup_refine_workspace_bytes(n->micro * out_ch, height / 4, width / 4));
    const size_t total = n->blob.total;
    const float* src = (const float*)((const char*)blob + BLOB_HEADER);
    auto fail = [&](int rc) { vitpose_free(n); return rc; };
#define VP_CHECK(expr) do { if ((expr) != hipSuccess) { ttup::set_error("%s failed (%s:%d)", #expr, __FILE__, __LINE__); return fail(TTUP_EHIP); } } while (0)
    VP_CHECK(hipMalloc((void**)&n->weights, total * 4));
    VP_CHECK(hipMemcpy(n->weights, src, total * 4, hipMemcpyHostToDevice));
    // Every tensor rounded once (RNE); the path reads the matrix weights from here and everything else from `weights`.  Rounding the
    // whole blob keeps one offset table for both (a tensor's bf16 copy sits at its fp32 offset: launch_gemm) at the price of memory
    // that is never read -- the bf16 copies of biases, LN parameters, pos_embed and the final conv (under 1 % of the blob) and the fp32
    // copies of the matrix weights: 1.5 x the fp32 handle's weight memory (about 140 MB instead of 95 MB).  Deliberate.
    if (dtype == 1) {
        std::vector<bf16_t> w16(total);
        for (size_t i = 0; i < total; ++i) w16[i] = f32_to_bf16(src[i]);
        VP_CHECK(hipMalloc((void**)&n->w16, total * 2));
        VP_CHECK(hipMemcpy(n->w16, w16.data(), total * 2, hipMemcpyHostToDevice));
    }
    VP_CHECK(hipMalloc((void**)&n->arena, n->plan.total));
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

// ------------------------------------------------------------------ launches: the one place that asks for the handle's dtype
#define VP_RC(expr) do { int _rc = (expr); if (_rc != TTUP_OK) return _rc; } while (0)

// fp32 handle: gemm_kernel on g as it stands.  bf16 handle: gemm_bf16_kernel with the weight read from w16 at g.w's offset, the
// A_DENSE / A_DECONV input (g.a) read as bf16, and the output (g.out) written as bf16 when bf16_out.  N and K are whole numbers of
// either kernel's tiles (vitpose_plan.h).
template <int AM>
static int launch_gemm(const ttup_vitpose* n, const GemmArgs& a, bool bf16_out, hipStream_t st) {
    if (n->dtype == 0) {
        hipLaunchKernelGGL(gemm_kernel<AM>, dim3(cdiv(a.M, BM), a.N / BN), dim3(256), 0, st, a);
    } else {
        Gemm16Args p = {};
        p.g = a;
        p.a16 = (const bf16_t*)a.a;
        p.w16 = n->w16 + (a.w - n->weights);
        p.out16 = bf16_out ? (bf16_t*)a.out : nullptr;
        p.stats64 = n->buf<double>(B_STATS64);
        hipLaunchKernelGGL(gemm_bf16_kernel<AM>, dim3(cdiv(a.M, TM), a.N / TN), dim3(256), 0, st, p);
    }
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// LayerNorm statistics of the M rows of the residual stream x
static int launch_ln_stats(const ttup_vitpose* n, int M, hipStream_t st) {
    if (n->dtype == 0) hipLaunchKernelGGL(ln_stats_kernel<float>, dim3(cdiv(M, 4)), dim3(256), 0, st, n->buf(B_X), M, n->buf(B_STATS));
    else hipLaunchKernelGGL(ln_stats_kernel<double>, dim3(cdiv(M, 4)), dim3(256), 0, st, n->buf(B_X), M, n->buf<double>(B_STATS64));
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// d.out = LayerNorm(d.a), materialised
static int launch_ln_apply(const ttup_vitpose* n, const GemmArgs& d, hipStream_t st) {
    if (n->dtype == 0) hipLaunchKernelGGL(ln_apply_kernel, dim3(cdiv(d.M * (DIM / 4), 256)), dim3(256), 0, st, d);
    else hipLaunchKernelGGL(ln_apply_bf16_kernel, dim3(cdiv(d.M * (DIM / 8), 256)), dim3(256), 0, st, d, n->buf<const double>(B_STATS64), (bf16_t*)d.out);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// att = softmax(q k^T / sqrt(HD)) v per head, from qkv
static int launch_attention(const ttup_vitpose* n, int nb, hipStream_t st) {
    const dim3 grid(cdiv(n->ntok, AQ), HEADS, nb);
    const float scale = 1.0f / sqrtf((float)HD);
    if (n->dtype == 0) hipLaunchKernelGGL(attention_kernel, grid, dim3(256), 0, st, n->buf(B_QKV), n->ntok, scale, n->buf(B_ATT));
    else hipLaunchKernelGGL(attention_bf16_kernel, grid, dim3(256), 0, st, n->buf<const bf16_t>(B_QKV), n->ntok, scale, n->buf<bf16_t>(B_ATT));
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// heat (nb, out_ch, 4hp, 4wp) = final 1x1 conv of d2
static int launch_conv1x1(const ttup_vitpose* n, int nb, float* heat, hipStream_t st) {
    const int hw = 16 * n->ntok;
    const long long npix = (long long)nb * hw;
    const dim3 grid((unsigned)((npix + 63) / 64));
    const float *w = n->weights + n->blob.fin_w, *bias = n->weights + n->blob.fin_b;
    if (n->dtype == 0) hipLaunchKernelGGL(conv1x1_kernel<float>, grid, dim3(256), 0, st, n->buf(B_D2), npix, hw, w, bias, n->out_ch, heat);
    else hipLaunchKernelGGL(conv1x1_kernel<bf16_t>, grid, dim3(256), 0, st, n->buf<const bf16_t>(B_D2), npix, hw, w, bias, n->out_ch, heat);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// Step `id` of the forward's list (vitpose_plan.h: shapes, epilogue, buffers) at batch nb, its weight and bias at float offsets w and
// bias of the blob; g brings what the step's A mode reads beyond that
static GemmArgs gemm_args(const ttup_vitpose* n, int id, int nb, size_t w, size_t bias, GemmArgs g) {
    const GemmSpec& s = GEMMS[id];
    if (s.in != B_IN) g.a = n->buf(s.in);
    g.w = n->weights + w; g.bias = n->weights + bias; g.out = n->buf(s.out);
    g.M = s.m_per_token * nb * n->ntok; g.N = s.N; g.K = s.K ? s.K : n->in_ch * 256; g.flags = s.flags;
    if (s.flags & E_RESID) g.res = g.out;
    return g;
}
template <int ID, int AM = GEMMS[ID].am>
static int run_gemm(const ttup_vitpose* n, int nb, size_t w, size_t bias, const GemmArgs& g, hipStream_t st) {
    return launch_gemm<AM>(n, gemm_args(n, ID, nb, w, bias, g), GEMMS[ID].bf16_out, st);
}
// what A_LN reads: gain and bias at float offsets of the blob, and the statistics launch_ln_stats left
static GemmArgs ln_args(const ttup_vitpose* n, size_t gain, size_t bias) {
    GemmArgs g = {};
    g.ln_g = n->weights + gain; g.ln_b = n->weights + bias; g.stats = n->buf(B_STATS);
    return g;
}

// ------------------------------------------------------------------ the model
// patch embedding + bias + pos_embed[1:] + pos_embed[:1]  (vit.py:222, :366): x_in (nb, in_ch, H, W), or with from_frames the samples'
// per-frame records (A_PATCH_FRAMES), -> the residual stream x
static int run_patch(ttup_vitpose* n, const float* x_in, int nb, hipStream_t st, bool from_frames) {
    GemmArgs g = {};
    g.a = x_in; g.cin = n->in_ch; g.ih = n->H; g.iw = n->W; g.pos = n->weights + n->blob.pos; g.ntok = n->ntok;
    return from_frames ? run_gemm<G_PATCH, A_PATCH_FRAMES>(n, nb, n->blob.patch_w, n->blob.patch_b, g, st)
                       : run_gemm<G_PATCH>(n, nb, n->blob.patch_w, n->blob.patch_b, g, st);
}

// one transformer block on the residual stream x; x_attn, when given, receives x as it stands between the two halves
static int run_block(ttup_vitpose* n, int i, int nb, hipStream_t st, float* x_attn = nullptr) {
    const int M = nb * n->ntok;
    const BlockOffsets& b = n->blob.blk[i];
    // x = x + proj(attn(norm1(x)))
    VP_RC(launch_ln_stats(n, M, st));
    VP_RC(run_gemm<G_QKV>(n, nb, b.qkvw, b.qkvb, ln_args(n, b.n1w, b.n1b), st));
    VP_RC(launch_attention(n, nb, st));
    VP_RC(run_gemm<G_PROJ>(n, nb, b.projw, b.projb, {}, st));
    if (x_attn) TTUP_HIP_CHECK(hipMemcpyAsync(x_attn, n->buf(B_X), (size_t)M * DIM * 4, hipMemcpyDeviceToDevice, st));
    // x = x + fc2(gelu(fc1(norm2(x))))
    VP_RC(launch_ln_stats(n, M, st));
    VP_RC(run_gemm<G_FC1>(n, nb, b.fc1w, b.fc1b, ln_args(n, b.n2w, b.n2b), st));
    return run_gemm<G_FC2>(n, nb, b.fc2w, b.fc2b, {}, st);
}

// deconvolution l (0, 1) as four 2x2 phase GEMMs, BN folded, ReLU: NHWC (nb, s hp, s wp, cin) -> (nb, 2s hp, 2s wp, 256), s = l + 1
template <int ID>
static int run_deconv(const ttup_vitpose* n, int l, int nb, hipStream_t st) {
    GemmArgs d = {};
    d.cin = GEMMS[ID].K / 4; d.ih = (l + 1) * n->hp; d.iw = (l + 1) * n->wp;
    for (int ph = 0; ph < 4; ++ph) {
        d.py = ph >> 1; d.px = ph & 1;
        VP_RC(run_gemm<ID>(n, nb, n->blob.dc_w[l] + (size_t)ph * DEC * GEMMS[ID].K, n->blob.dc_b[l], d, st));
    }
    return TTUP_OK;
}

// the head on the residual stream x: last_norm, the two deconvolutions, the final 1x1 conv -> heat (nb, out_ch, H/4, W/4)
static int run_head(ttup_vitpose* n, int nb, float* heat, hipStream_t st) {
    // last_norm: materialised once (deconv 1 gathers every token four times per phase)
    VP_RC(launch_ln_stats(n, nb * n->ntok, st));
    VP_RC(launch_ln_apply(n, gemm_args(n, G_LAST_NORM, nb, 0, 0, ln_args(n, n->blob.lnw, n->blob.lnb)), st));
    VP_RC(run_deconv<G_DECONV1>(n, 0, nb, st));
    VP_RC(run_deconv<G_DECONV2>(n, 1, nb, st));
    return launch_conv1x1(n, nb, heat, st);
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
    TTUP_REQUIRE(stage >= 0 && stage < STAGES, TTUP_EINVAL, "ttup_vitpose_run_stage: stage %d outside 0..%d", stage, STAGES - 1);
    TTUP_REQUIRE(batch >= 1 && batch <= net->micro, TTUP_EINVAL, "ttup_vitpose_run_stage: batch %d outside 1..%d (the micro-batch)", batch, net->micro);
    TTUP_REQUIRE(((uintptr_t)in_dev & 15) == 0, TTUP_EINVAL, "ttup_vitpose_run_stage: input must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t xbytes = (size_t)batch * net->ntok * DIM * 4;
    net->tap_stage = -1;
    if (stage == 0) {
        VP_RC(run_patch(net, in_dev, batch, st, false));
    } else {
        TTUP_HIP_CHECK(hipMemcpyAsync(net->buf(B_X), in_dev, xbytes, hipMemcpyDeviceToDevice, st));
        if (stage <= DEPTH) {
            if (!net->x_attn) TTUP_HIP_CHECK(hipMalloc((void**)&net->x_attn, (size_t)net->micro * net->ntok * DIM * 4));
            VP_RC(run_block(net, stage - 1, batch, st, net->x_attn));
        } else {
            VP_RC(run_head(net, batch, net->buf(B_HEAT), st));
        }
    }
    net->tap_stage = stage; net->tap_batch = batch;
    return TTUP_OK;
}

extern "C" int ttup_vitpose_read_tap(ttup_vitpose* net, const char* tap, void* dst, size_t bytes) {
    TTUP_REQUIRE(net && tap && dst, TTUP_EINVAL, "ttup_vitpose_read_tap: null argument");
    TTUP_REQUIRE(net->tap_stage >= 0, TTUP_EINVAL, "ttup_vitpose_read_tap: no stage has run since the last forward");
    const int s = net->tap_stage;
    for (const Tap& t : TAPS) {
        if (strcmp(tap, t.name) != 0) continue;
        TTUP_REQUIRE(s >= t.first && s <= t.last, TTUP_EINVAL, "ttup_vitpose_read_tap: stage %d does not write tap '%s'", s, tap);
        const size_t want = (size_t)net->tap_batch * net->ntok * (t.cols ? t.cols : 16 * net->out_ch) * elem_size(t.buf, net->dtype);
        TTUP_REQUIRE(bytes == want, TTUP_EINVAL, "ttup_vitpose_read_tap: tap '%s' has %zu bytes, the buffer %zu", tap, want, bytes);
        TTUP_HIP_CHECK(hipDeviceSynchronize());          // whatever stream the stage ran on, and whether it still exists
        TTUP_HIP_CHECK(hipMemcpy(dst, net->buf<char>(t.buf), bytes, hipMemcpyDefault));
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
        float* heat = heat_dev ? heat_dev + b0 * heat_per : net->buf(B_HEAT);
        VP_RC(vitpose_run(net, x_dev + b0 * in_per, nb, heat, st));
        if (argmax_dev)
            VP_RC(refine_argmax(heat, nb * co, hh, ww, (long long*)argmax_dev + (size_t)b0 * co, win_dev + (size_t)b0 * co * 9, net->buf<void>(B_WS),
                                net->plan.bytes[B_WS], st));
    }
    return TTUP_OK;
}

// The backbone alone: the patch embedding, the blocks and last_norm per micro-batch -> out (batch * tokens, DIM), what run_head's
// deconvolutions read (the same launches, so the same bits as the "ln" tap)
extern "C" int ttup_vitpose_features(ttup_vitpose* net, const float* x_dev, int batch, float* out_dev, void* stream) {
    TTUP_REQUIRE(net && x_dev && out_dev, TTUP_EINVAL, "ttup_vitpose_features: null argument");
    TTUP_REQUIRE(net->dtype == 0, TTUP_EINVAL, "ttup_vitpose_features: a bf16 handle keeps last_norm's output in bf16; use an f32 handle");
    TTUP_REQUIRE(batch >= 0, TTUP_EINVAL, "ttup_vitpose_features: negative batch %d", batch);
    TTUP_REQUIRE(((uintptr_t)x_dev & 15) == 0, TTUP_EINVAL, "ttup_vitpose_features: input must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t in_per = (size_t)net->in_ch * net->H * net->W, out_per = (size_t)net->ntok * DIM;
    for (int b0 = 0; b0 < batch; b0 += net->micro) {
        const int nb = batch - b0 < net->micro ? batch - b0 : net->micro;
        net->tap_stage = -1;
        VP_RC(run_patch(net, x_dev + b0 * in_per, nb, st, false));
        for (int i = 0; i < DEPTH; ++i) VP_RC(run_block(net, i, nb, st));
        VP_RC(launch_ln_stats(net, nb * net->ntok, st));
        VP_RC(launch_ln_apply(net, gemm_args(net, G_LAST_NORM, nb, 0, 0, ln_args(net, net->blob.lnw, net->blob.lnb)), st));
        TTUP_HIP_CHECK(hipMemcpyAsync(out_dev + b0 * out_per, net->buf(GEMMS[G_LAST_NORM].out), nb * out_per * 4, hipMemcpyDeviceToDevice, st));
    }
    return TTUP_OK;
}

// n_frames BGR uint8 HWC frames (device, any size) -> the outputs of ttup_vitpose_forward on ttup_preprocess_triples (in_ch 9) or
// ttup_preprocess_frames (in_ch 3) of them, bit for bit: each micro-batch's frames are pre-processed once into fp32 records (the
// same launch_preprocess) and the patch embedding gathers its triples from them.
extern "C" int ttup_vitpose_forward_frames(ttup_vitpose* net, const uint8_t* frames_dev, int n_frames, int src_h, int src_w,
                                           float* heat_dev, int64_t* argmax_dev, float* win_dev, void* stream) {
    TTUP_REQUIRE(net && frames_dev, TTUP_EINVAL, "ttup_vitpose_forward_frames: null handle or frames");
    TTUP_REQUIRE(net->buf(B_FRAMES), TTUP_EINVAL, "ttup_vitpose_forward_frames: in_ch %d is not a whole number of BGR frames", net->in_ch);
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
        VP_RC(launch_preprocess(frames_dev, n_frames, src_h, src_w, net->H, net->W, net->buf(B_FRAMES), TTUP_LAYOUT_NCHW_F32, TTUP_DTYPE_F32, b0,
                                nb + nf - 1, 1, st));
        float* heat = heat_dev ? heat_dev + b0 * heat_per : net->buf(B_HEAT);
        VP_RC(vitpose_run(net, net->buf(B_FRAMES), nb, heat, st, true));
        if (argmax_dev)
            VP_RC(refine_argmax(heat, nb * co, hh, ww, (long long*)argmax_dev + (size_t)b0 * co, win_dev + (size_t)b0 * co * 9, net->buf<void>(B_WS),
                                net->plan.bytes[B_WS], st));
    }
    return TTUP_OK;
}
#include "no_packed_fp32_end.h"
