// The ViTPose-small backbone in training mode, and its backward: images in, last_norm's output out, with every
// block's activations kept; then the gradient into last_norm's output in, the gradients of the 149 backbone tensors out.  The forward
// is vitpose.hip's -- the same gemm_kernel instances and the same LN / attention arithmetic, so with unit branch scales the same bits
// as ttup_vitpose_features -- with a per-sample scale on each residual branch (stochastic depth: x + s[b] * branch).
//
// Arithmetic: fp32 operands and accumulation on v_mfma_f32_16x16x4_f32 for every product; every sum over tokens that is not a GEMM's
// k loop in fp64 over slices of SLICE_TOKENS tokens added in slice order; the k-slices of a dW product are fp32 partials added in
// slice order.  No atomics: the same call gives the same bits.
//
// Forward   patch GEMM (A_PATCH, E_POS) -> X[0]; im2col kept.  Per block: ln_stats; qkv = gemm<A_LN>; attention_lse (att, lse);
//           proj -> BR; XMID = X + s1 BR; ln_stats; fc1 = gemm<A_LN> -> PRE; HID = gelu(PRE); fc2 -> BR; X[i+1] = XMID + s2 BR.
//           ln_stats; ln_apply -> feat.
// Backward  G = ln_bwd(dfeat).  Per block, last first: BR = s2 G; db; HID = gelu(PRE); dW2 = BR^T HID; DHID = BR W2, times gelu';
//           db; LN = norm2(XMID); dW1 = DHID^T LN; DLN = DHID W1; d gamma, d beta; G += ln_bwd(DLN).  BR = s1 G; db; dWp = BR^T ATT;
//           DLN = BR Wp (d att); delta, dkv, dq -> DQKV; db; LN = norm1(X); dWqkv = DQKV^T LN; DLN = DQKV Wqkv; d gamma, d beta;
//           G += ln_bwd(DLN).  Then dpos, the patch bias (column sums of G) and the patch dW = G^T COL.
// Every dX is the guarded gemm_kernel<O_ROWS, true, O_COLS> (the weight read by columns), every dW gemm_kernel<O_COLS, true, O_COLS>
// over k-slices and dw_reduce.  The host's decisions are csrc/vitpose_grad_plan.h; this unit is the driver.
#include "no_packed_fp32_begin.h"      // runs beside the CNN's chain kernels: no packed fp32 (common.h)
#include "common.h"
#include "gemm_f32.h"
#include "vitpose_grad_kernels.h"

#include <string.h>

using namespace ttup;
using namespace ttup::vgrad;
using ttup::gemm::GemmArgs;
using ttup::gemm::gemm_kernel;

struct ttup_vitpose_grad {
    int in_ch = 0, hp = 0, wp = 0, ntok = 0, max_batch = 0;
    long long max_rows = 0;
    Workspace ws;
    char* arena = nullptr;
    int batch = 0;          // what the last forward ran on (0: none)

    template <class T = float> T* buf(int b) const { return (T*)(arena + ws.off[b]); }
    // block i's slot of a kept buffer with `cols` floats a token
    float* slot(int b, int i, int cols) const { return buf(b) + (size_t)i * max_rows * cols; }
    const float* scale(int i, int half) const { return buf(B_SCALE) + ((size_t)i * 2 + half) * batch_scale; }
    int batch_scale = 0;    // the batch the scales were written for
};

extern "C" size_t ttup_vitpose_grad_workspace_bytes(int in_ch, int hp, int wp, int max_batch) {
    return check_create(in_ch, hp, wp, max_batch).rc == TTUP_OK ? plan_workspace((long long)hp * wp * max_batch, in_ch, max_batch).total : 0;
}

extern "C" int ttup_vitpose_grad_create(int in_ch, int hp, int wp, int max_batch, ttup_vitpose_grad** out) {
    TTUP_REQUIRE(out, TTUP_EINVAL, "ttup_vitpose_grad_create: null argument");
    *out = nullptr;
    const Refusal r = check_create(in_ch, hp, wp, max_batch);
    TTUP_REQUIRE(r.rc == TTUP_OK, r.rc, "%s", r.msg);
    ttup_vitpose_grad* h = new ttup_vitpose_grad();
    h->in_ch = in_ch; h->hp = hp; h->wp = wp; h->ntok = hp * wp; h->max_batch = max_batch;
    h->max_rows = (long long)h->ntok * max_batch;
    h->ws = plan_workspace(h->max_rows, in_ch, max_batch);
    if (hipMalloc((void**)&h->arena, h->ws.total) != hipSuccess) {
        ttup::set_error("ttup_vitpose_grad_create: hipMalloc of %zu bytes failed", h->ws.total);
        delete h;
        return TTUP_ENOMEM;
    }
    *out = h;
    return TTUP_OK;
}

extern "C" void ttup_vitpose_grad_destroy(ttup_vitpose_grad* h) {
    if (!h) return;
    if (h->arena) (void)hipFree(h->arena);
    delete h;
}

#define VG_RC(expr) do { int _rc = (expr); if (_rc != TTUP_OK) return _rc; } while (0)
static unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }
static bool all_set(const float* const* t) {
    for (int i = 0; i < TENSORS; ++i)
        if (!t[i]) return false;
    return true;
}

// ------------------------------------------------------------------ launches
static int launch_ln_stats(const float* x, int M, float* stats, hipStream_t st) {
    hipLaunchKernelGGL(ln_stats_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, x, M, stats);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}
// what A_LN reads
static GemmArgs ln_args(const float* x, const float* stats, const float* gain, const float* bias) {
    GemmArgs g = {};
    g.a = x; g.stats = stats; g.ln_g = gain; g.ln_b = bias;
    return g;
}
// out = LayerNorm(g.a), materialised
static int launch_ln_apply(GemmArgs g, int M, float* out, hipStream_t st) {
    g.M = M; g.K = DIM; g.out = out;
    hipLaunchKernelGGL(ln_apply_kernel, dim3(blocks((long long)M * (DIM / 4), 256)), dim3(256), 0, st, g);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}
// the forward's GEMMs: out (M, N) = A w^T + bias, w (N, K) as the reference keeps it; N and K are whole numbers of tiles
template <int AM>
static int launch_fwd_gemm(GemmArgs g, int M, int N, int K, const float* w, const float* bias, float* out, int flags, hipStream_t st) {
    g.M = M; g.N = N; g.K = K; g.w = w; g.bias = bias; g.out = out; g.flags = flags;
    hipLaunchKernelGGL(gemm_kernel<AM>, dim3(cdiv(M, BM), N / BN), dim3(256), 0, st, g);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}
// out = (x ? x : 0) + s[b] y over M rows of DIM
static int launch_scale_add(const ttup_vitpose_grad* h, const float* x, const float* y, const float* s, int M, float* out, hipStream_t st) {
    const long long quads = (long long)M * (DIM / 4);
    hipLaunchKernelGGL(scale_add_kernel, dim3(blocks(quads, 256)), dim3(256), 0, st, x, y, s, h->ntok, quads, out);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}
// dx (M, N) = dy (M, K) w, w (K, N) as the reference keeps it (read by columns)
static int launch_dx(const float* dy, const float* w, int M, int N, int K, float* dx, hipStream_t st) {
    GemmArgs g = {};
    g.a = dy; g.lda = K; g.w = w; g.ldw = N; g.out = dx; g.ldo = N;
    g.M = M; g.N = N; g.K = K; g.kslice = K;
    hipLaunchKernelGGL((gemm_kernel<gemm::O_ROWS, true, gemm::O_COLS>), dim3(cdiv(M, BM), cdiv(N, BN), 1), dim3(256), 0, st, g);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}
// dw (n_out, n_in) = dy^T a over `rows` rows: dy (rows, n_out), a (rows, n_in), cut into k-slices added in slice order
static int launch_dw(const ttup_vitpose_grad* h, const float* dy, const float* a, int rows, int n_out, int n_in, float* dw, hipStream_t st) {
    const int ns = slices(rows);
    GemmArgs g = {};
    g.a = dy; g.lda = n_out; g.w = a; g.ldw = n_in; g.out = h->buf(B_PARTIAL); g.ldo = n_in;
    g.M = n_out; g.N = n_in; g.K = rows; g.kslice = SLICE_TOKENS;
    hipLaunchKernelGGL((gemm_kernel<gemm::O_COLS, true, gemm::O_COLS>), dim3(cdiv(n_out, BM), cdiv(n_in, BN), ns), dim3(256), 0, st, g);
    TTUP_LAUNCH_CHECK();
    const long long n = (long long)n_out * n_in;
    hipLaunchKernelGGL(dw_reduce_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, (const float*)h->buf(B_PARTIAL), ns, n, dw);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}
// out[c] = sum over rows of d[row][c] (ncols a multiple of 64)
static int launch_col_sums(const ttup_vitpose_grad* h, const float* d, int rows, int ncols, float* out, hipStream_t st) {
    const int ns = slices(rows);
    hipLaunchKernelGGL(col_sums_kernel<false>, dim3(ncols / 64, ns), dim3(1024), 0, st, d, (const float*)nullptr, (const float*)nullptr, ncols, (long long)rows,
                       (long long)SLICE_TOKENS, h->buf<double>(B_SUMS));
    TTUP_LAUNCH_CHECK();
    hipLaunchKernelGGL(sums_finalize_kernel, dim3(blocks(ncols, 256)), dim3(256), 0, st, (const double*)h->buf<double>(B_SUMS), ns, ncols, out, (float*)nullptr);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}
// One LayerNorm's backward: dy (M, DIM) the gradient into its output, x and stats what the forward kept -> d gamma, d beta, and the
// gradient into x written (acc 0) or added (acc 1) to g
static int launch_ln_bwd(const ttup_vitpose_grad* h, const float* x, const float* stats, const float* dy, const float* gamma, int M, int acc, float* dgamma,
                         float* dbeta, float* g, hipStream_t st) {
    const int ns = slices(M);
    hipLaunchKernelGGL(col_sums_kernel<true>, dim3(DIM / 64, ns), dim3(1024), 0, st, dy, x, stats, DIM, (long long)M, (long long)SLICE_TOKENS,
                       h->buf<double>(B_SUMS));
    TTUP_LAUNCH_CHECK();
    hipLaunchKernelGGL(sums_finalize_kernel, dim3(blocks(DIM, 256)), dim3(256), 0, st, (const double*)h->buf<double>(B_SUMS), ns, DIM, dbeta, dgamma);
    TTUP_LAUNCH_CHECK();
    hipLaunchKernelGGL(ln_bwd_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, x, stats, dy, gamma, M, acc, g);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// ------------------------------------------------------------------ forward
extern "C" int ttup_vitpose_grad_forward(ttup_vitpose_grad* h, const float* x_dev, int batch, const ttup_vitpose_backbone_params* p,
                                         const float* drop_scale_dev, long long drop_scale_len, float* feat_dev, void* stream) {
    TTUP_REQUIRE(h && x_dev && p && feat_dev, TTUP_EINVAL, "ttup_vitpose_grad_forward: null argument");
    TTUP_REQUIRE(all_set(p->t), TTUP_EINVAL, "ttup_vitpose_grad_forward: null parameter");
    TTUP_REQUIRE((drop_scale_dev == nullptr) == (drop_scale_len == 0), TTUP_EINVAL, "ttup_vitpose_grad_forward: drop_scale and its length go together");
    const Refusal r = check_forward(h->max_batch, batch, drop_scale_len);
    TTUP_REQUIRE(r.rc == TTUP_OK, r.rc, "%s", r.msg);
    TTUP_REQUIRE(((uintptr_t)x_dev & 15) == 0 && ((uintptr_t)feat_dev & 15) == 0, TTUP_EINVAL, "ttup_vitpose_grad_forward: input and output must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int M = batch * h->ntok, Kp = h->in_ch * 256;
    const float scale = 1.0f / sqrtf((float)HD);
    h->batch = 0;                                      // nothing to run a backward on until this forward is complete
    h->batch_scale = batch;
    if (drop_scale_dev) {
        TTUP_HIP_CHECK(hipMemcpyAsync(h->buf(B_SCALE), drop_scale_dev, (size_t)drop_scale_len * 4, hipMemcpyDeviceToDevice, st));
    } else {
        hipLaunchKernelGGL(fill_kernel, dim3(blocks(DEPTH * 2 * batch, 256)), dim3(256), 0, st, h->buf(B_SCALE), DEPTH * 2 * batch, 1.0f);
        TTUP_LAUNCH_CHECK();
    }
    // patch embedding + bias + pos_embed[1:] + pos_embed[:1], and the im2col its dW reads
    GemmArgs pe = {};
    pe.a = x_dev; pe.cin = h->in_ch; pe.ih = 16 * h->hp; pe.iw = 16 * h->wp; pe.pos = p->t[T_POS]; pe.ntok = h->ntok;
    VG_RC(launch_fwd_gemm<gemm::A_PATCH>(pe, M, DIM, Kp, p->t[T_PATCHW], p->t[T_PATCHB], h->slot(B_X, 0, DIM), gemm::E_POS, st));
    pe.M = M; pe.K = Kp; pe.out = h->buf(B_COL);
    hipLaunchKernelGGL(im2col_kernel, dim3(blocks((long long)M * (Kp / 4), 256)), dim3(256), 0, st, pe);
    TTUP_LAUNCH_CHECK();
    for (int i = 0; i < DEPTH; ++i) {
        const float* const* t = p->t + block_tensor(i, 0);
        float *x = h->slot(B_X, i, DIM), *xmid = h->slot(B_XMID, i, DIM), *xout = h->slot(B_X, i + 1, DIM);
        float *st1 = h->slot(B_ST1, i, 2), *st2 = h->slot(B_ST2, i, 2), *qkv = h->slot(B_QKV, i, 3 * DIM), *att = h->slot(B_ATT, i, DIM);
        // x = x + s1 proj(attn(norm1(x)))
        VG_RC(launch_ln_stats(x, M, st1, st));
        VG_RC(launch_fwd_gemm<gemm::A_LN>(ln_args(x, st1, t[T_N1W], t[T_N1B]), M, 3 * DIM, DIM, t[T_QKVW], t[T_QKVB], qkv, 0, st));
        hipLaunchKernelGGL(attention_lse_kernel, dim3(cdiv(h->ntok, AQ), HEADS, batch), dim3(256), 0, st, (const float*)qkv, h->ntok, scale, att,
                           h->slot(B_LSE, i, HEADS));
        TTUP_LAUNCH_CHECK();
        GemmArgs d = {};
        d.a = att;
        VG_RC(launch_fwd_gemm<gemm::A_DENSE>(d, M, DIM, DIM, t[T_PROJW], t[T_PROJB], h->buf(B_BR), 0, st));
        VG_RC(launch_scale_add(h, x, h->buf(B_BR), h->scale(i, 0), M, xmid, st));
        // x = x + s2 fc2(gelu(fc1(norm2(x))))
        VG_RC(launch_ln_stats(xmid, M, st2, st));
        VG_RC(launch_fwd_gemm<gemm::A_LN>(ln_args(xmid, st2, t[T_N2W], t[T_N2B]), M, MLP, DIM, t[T_FC1W], t[T_FC1B], h->slot(B_PRE, i, MLP), 0, st));
        hipLaunchKernelGGL(gelu_kernel, dim3(blocks((long long)M * (MLP / 4), 256)), dim3(256), 0, st, (const float*)h->slot(B_PRE, i, MLP),
                           (long long)M * (MLP / 4), h->buf(B_HID));
        TTUP_LAUNCH_CHECK();
        d.a = h->buf(B_HID);
        VG_RC(launch_fwd_gemm<gemm::A_DENSE>(d, M, DIM, MLP, t[T_FC2W], t[T_FC2B], h->buf(B_BR), 0, st));
        VG_RC(launch_scale_add(h, xmid, h->buf(B_BR), h->scale(i, 1), M, xout, st));
    }
    const float* xl = h->slot(B_X, DEPTH, DIM);
    VG_RC(launch_ln_stats(xl, M, h->buf(B_STL), st));
    VG_RC(launch_ln_apply(ln_args(xl, h->buf(B_STL), p->t[T_LNW], p->t[T_LNB]), M, feat_dev, st));
    h->batch = batch;
    return TTUP_OK;
}

// ------------------------------------------------------------------ backward
extern "C" int ttup_vitpose_grad_backward(ttup_vitpose_grad* h, const float* dfeat_dev, int batch, const ttup_vitpose_backbone_params* p,
                                          const ttup_vitpose_backbone_grads* gr, void* stream) {
    TTUP_REQUIRE(h && dfeat_dev && p && gr, TTUP_EINVAL, "ttup_vitpose_grad_backward: null argument");
    TTUP_REQUIRE(all_set(p->t), TTUP_EINVAL, "ttup_vitpose_grad_backward: null parameter");
    TTUP_REQUIRE(all_set(gr->t), TTUP_EINVAL, "ttup_vitpose_grad_backward: null gradient output");
    const Refusal r = check_backward(h->batch, batch);
    TTUP_REQUIRE(r.rc == TTUP_OK, r.rc, "%s", r.msg);
    TTUP_REQUIRE(((uintptr_t)dfeat_dev & 15) == 0, TTUP_EINVAL, "ttup_vitpose_grad_backward: the feature gradient must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int M = batch * h->ntok, Kp = h->in_ch * 256;
    const float scale = 1.0f / sqrtf((float)HD);
    float *G = h->buf(B_G), *BR = h->buf(B_BR), *LN = h->buf(B_LN), *DLN = h->buf(B_DLN), *HID = h->buf(B_HID), *DHID = h->buf(B_DHID), *DQKV = h->buf(B_DQKV);
    VG_RC(launch_ln_bwd(h, h->slot(B_X, DEPTH, DIM), h->buf(B_STL), dfeat_dev, p->t[T_LNW], M, 0, gr->t[T_LNW], gr->t[T_LNB], G, st));
    for (int i = DEPTH - 1; i >= 0; --i) {
        const float* const* t = p->t + block_tensor(i, 0);
        float* const* d = gr->t + block_tensor(i, 0);
        const float *x = h->slot(B_X, i, DIM), *xmid = h->slot(B_XMID, i, DIM), *st1 = h->slot(B_ST1, i, 2), *st2 = h->slot(B_ST2, i, 2);
        const float *qkv = h->slot(B_QKV, i, 3 * DIM), *att = h->slot(B_ATT, i, DIM), *pre = h->slot(B_PRE, i, MLP), *lse = h->slot(B_LSE, i, HEADS);
        const long long hq = (long long)M * (MLP / 4);
        // the MLP half
        VG_RC(launch_scale_add(h, nullptr, G, h->scale(i, 1), M, BR, st));
        VG_RC(launch_col_sums(h, BR, M, DIM, d[T_FC2B], st));
        hipLaunchKernelGGL(gelu_kernel, dim3(blocks(hq, 256)), dim3(256), 0, st, pre, hq, HID);
        TTUP_LAUNCH_CHECK();
        VG_RC(launch_dw(h, BR, HID, M, DIM, MLP, d[T_FC2W], st));
        VG_RC(launch_dx(BR, t[T_FC2W], M, MLP, DIM, DHID, st));
        hipLaunchKernelGGL(gelu_bwd_kernel, dim3(blocks(hq, 256)), dim3(256), 0, st, pre, hq, DHID);
        TTUP_LAUNCH_CHECK();
        VG_RC(launch_col_sums(h, DHID, M, MLP, d[T_FC1B], st));
        VG_RC(launch_ln_apply(ln_args(xmid, st2, t[T_N2W], t[T_N2B]), M, LN, st));
        VG_RC(launch_dw(h, DHID, LN, M, MLP, DIM, d[T_FC1W], st));
        VG_RC(launch_dx(DHID, t[T_FC1W], M, DIM, MLP, DLN, st));
        VG_RC(launch_ln_bwd(h, xmid, st2, DLN, t[T_N2W], M, 1, d[T_N2W], d[T_N2B], G, st));
        // the attention half
        VG_RC(launch_scale_add(h, nullptr, G, h->scale(i, 0), M, BR, st));
        VG_RC(launch_col_sums(h, BR, M, DIM, d[T_PROJB], st));
        VG_RC(launch_dw(h, BR, att, M, DIM, DIM, d[T_PROJW], st));
        VG_RC(launch_dx(BR, t[T_PROJW], M, DIM, DIM, DLN, st));
        const AttnGrid gd = attn_delta_grid(M), ga = attn_bwd_grid(h->ntok, batch);
        hipLaunchKernelGGL(attn_delta_kernel, dim3(gd.x, gd.y, gd.z), dim3(256), 0, st, (const float*)DLN, att, (long long)M, h->buf(B_DELTA));
        TTUP_LAUNCH_CHECK();
        hipLaunchKernelGGL(attn_bwd_dkv_kernel, dim3(ga.x, ga.y, ga.z), dim3(256), 0, st, qkv, (const float*)DLN, lse, (const float*)h->buf(B_DELTA), h->ntok,
                           scale, DQKV);
        TTUP_LAUNCH_CHECK();
        hipLaunchKernelGGL(attn_bwd_dq_kernel, dim3(ga.x, ga.y, ga.z), dim3(256), 0, st, qkv, (const float*)DLN, lse, (const float*)h->buf(B_DELTA), h->ntok,
                           scale, DQKV);
        TTUP_LAUNCH_CHECK();
        VG_RC(launch_col_sums(h, DQKV, M, 3 * DIM, d[T_QKVB], st));
        VG_RC(launch_ln_apply(ln_args(x, st1, t[T_N1W], t[T_N1B]), M, LN, st));
        VG_RC(launch_dw(h, DQKV, LN, M, 3 * DIM, DIM, d[T_QKVW], st));
        VG_RC(launch_dx(DQKV, t[T_QKVW], M, DIM, 3 * DIM, DLN, st));
        VG_RC(launch_ln_bwd(h, x, st1, DLN, t[T_N1W], M, 1, d[T_N1W], d[T_N1B], G, st));
    }
    // G = d x0: dpos[0] = the patch bias's gradient = its column sums; dpos[1 + t] = its sum over samples; dW = G^T im2col
    VG_RC(launch_col_sums(h, G, M, DIM, gr->t[T_PATCHB], st));
    VG_RC(launch_col_sums(h, G, M, DIM, gr->t[T_POS], st));
    hipLaunchKernelGGL(dpos_rows_kernel, dim3(blocks((long long)h->ntok * DIM, 256)), dim3(256), 0, st, (const float*)G, batch, h->ntok, gr->t[T_POS]);
    TTUP_LAUNCH_CHECK();
    return launch_dw(h, G, h->buf(B_COL), M, DIM, Kp, gr->t[T_PATCHW], st);
}

// The testing seam: what the last forward kept of block `block` (0..11; "x" also 12: what last_norm reads) -- "x", "x_mid", "att"
// (rows, 384), "qkv" (rows, 1152), "lse" (rows, 12), "pre" (rows, 1536) -- and, after a backward, "dqkv" (rows, 1152) of block 0,
// the last one it ran
extern "C" int ttup_vitpose_grad_read_tap(ttup_vitpose_grad* h, const char* tap, int block, void* dst, size_t bytes) {
    TTUP_REQUIRE(h && tap && dst, TTUP_EINVAL, "ttup_vitpose_grad_read_tap: null argument");
    TTUP_REQUIRE(h->batch > 0, TTUP_EINVAL, "ttup_vitpose_grad_read_tap: no forward has run on this handle");
    const struct { const char* name; int buf, cols, last; } taps[] = {
        {"x", B_X, DIM, DEPTH}, {"x_mid", B_XMID, DIM, DEPTH - 1}, {"att", B_ATT, DIM, DEPTH - 1}, {"qkv", B_QKV, 3 * DIM, DEPTH - 1},
        {"lse", B_LSE, HEADS, DEPTH - 1}, {"pre", B_PRE, MLP, DEPTH - 1}, {"dqkv", B_DQKV, 3 * DIM, 0},
    };
    const size_t rows = (size_t)h->batch * h->ntok;
    for (const auto& t : taps) {
        if (strcmp(tap, t.name) != 0) continue;
        TTUP_REQUIRE(block >= 0 && block <= t.last, TTUP_EINVAL, "ttup_vitpose_grad_read_tap: tap '%s' has blocks 0..%d, asked for %d", tap, t.last, block);
        TTUP_REQUIRE(bytes == rows * t.cols * 4, TTUP_EINVAL, "ttup_vitpose_grad_read_tap: tap '%s' has %zu bytes, the buffer %zu", tap, rows * t.cols * 4, bytes);
        TTUP_HIP_CHECK(hipDeviceSynchronize());
        TTUP_HIP_CHECK(hipMemcpy(dst, h->slot(t.buf, block, t.cols), bytes, hipMemcpyDefault));
        return TTUP_OK;
    }
    ttup::set_error("ttup_vitpose_grad_read_tap: unknown tap '%s'", tap);
    return TTUP_EINVAL;
}
#include "no_packed_fp32_end.h"
