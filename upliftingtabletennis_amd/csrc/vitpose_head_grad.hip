// ViTPose's keypoint head (TopdownHeatmapSimpleHead: two ConvTranspose2d(k4, s2, p1, no bias) + BatchNorm2d + ReLU, a 1x1 conv) in
// training mode, and its backward: features in; heatmaps, the eight parameter gradients and the gradient into the features out
// (DESIGN.md section 29).  The inference forward (csrc/vitpose.hip) folds BN into the weights at pack time; this one keeps BN apart,
// takes batch statistics over the whole batch, updates the running statistics and keeps the activations the backward reads.
//
// Arithmetic: fp32 operands and accumulation on v_mfma_f32_16x16x4_f32 for every product (gemm_kernel, csrc/gemm_f32.h); every sum
// over pixels that is not a GEMM's k loop (the BN statistics, d gamma / d beta, dWf / dbf) in fp64 over slices of fixed size added in
// slice order; the k-slices of a dW product are fp32 partials added in slice order.  No atomics: the same call gives the same bits.
//
// Forward   pack W1, W2 (phase matrices for the forward, (cin, 16 cout) for the backward) -> per deconvolution: four
//           gemm_kernel<A_DECONV> phases (flags 0, a zero bias) -> z NHWC; bn_sums / bn_finalize; bn_relu -> a -> conv1x1 -> heat.
// Backward  conv1x1_bwd (da2, gated) ; dwf partial sums ; then per deconvolution, last first: bn_sums<BWD> / bn_bwd_finalize
//           (d gamma, d beta); bn_dz in place; dW' = A^T G as the guarded gemm_kernel<O_COLS, true, O_DGRAD> over k-slices and
//           dw_reduce; dA = G Wperm^T as gemm_kernel<A_DGRAD>.  G is the gather of gemm_modes.h's dgrad_index, never materialised.
// The host's decisions are csrc/vitpose_head_plan.h; this unit is the driver.
#include "no_packed_fp32_begin.h"      // runs beside the CNN's chain kernels: no packed fp32 (common.h)
#include "common.h"
#include "gemm_f32.h"
#include "vitpose_head_grad_kernels.h"

#include <string.h>

using namespace ttup;
using namespace ttup::vhead;
using ttup::gemm::GemmArgs;
using ttup::gemm::gemm_kernel;

struct ttup_vitpose_head {
    int out_ch = 0;
    long long max_rows = 0;
    Workspace ws;
    char* arena = nullptr;
    int batch = 0, hp = 0, wp = 0, train = 0;          // what the last forward ran on (batch 0: none)

    template <class T = float> T* buf(int b) const { return (T*)(arena + ws.off[b]); }
    float* small(int off) const { return buf(B_SMALL) + off; }
};

extern "C" size_t ttup_vitpose_head_workspace_bytes(int out_ch, long long max_rows) {
    return check_create(out_ch, max_rows).rc == TTUP_OK ? plan_workspace(max_rows, out_ch).total : 0;
}

extern "C" int ttup_vitpose_head_create(int out_ch, long long max_rows, ttup_vitpose_head** out) {
    TTUP_REQUIRE(out, TTUP_EINVAL, "ttup_vitpose_head_create: null argument");
    *out = nullptr;
    const Refusal r = check_create(out_ch, max_rows);
    TTUP_REQUIRE(r.rc == TTUP_OK, r.rc, "%s", r.msg);
    ttup_vitpose_head* h = new ttup_vitpose_head();
    h->out_ch = out_ch; h->max_rows = max_rows;
    h->ws = plan_workspace(max_rows, out_ch);
    if (hipMalloc((void**)&h->arena, h->ws.total) != hipSuccess) {
        ttup::set_error("ttup_vitpose_head_create: hipMalloc of %zu bytes failed", h->ws.total);
        delete h;
        return TTUP_ENOMEM;
    }
    *out = h;
    return TTUP_OK;
}

extern "C" void ttup_vitpose_head_destroy(ttup_vitpose_head* h) {
    if (!h) return;
    if (h->arena) (void)hipFree(h->arena);
    delete h;
}

#define VH_RC(expr) do { int _rc = (expr); if (_rc != TTUP_OK) return _rc; } while (0)
static unsigned blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// z (NHWC, batch x 2ih x 2iw x DEC) = conv_transpose2d(a (NHWC, batch x ih x iw x cin)) by the four phase matrices wph
static int run_deconv(const ttup_vitpose_head* h, const float* a, const float* wph, int cin, int batch, int ih, int iw, float* z, hipStream_t st) {
    GemmArgs g = {};
    g.a = a; g.bias = h->small(SmallOff::ZERO); g.out = z;
    g.M = batch * ih * iw; g.N = DEC; g.K = 4 * cin; g.cin = cin; g.ih = ih; g.iw = iw;
    for (int ph = 0; ph < 4; ++ph) {
        g.py = ph >> 1; g.px = ph & 1;
        g.w = wph + (size_t)ph * DEC * 4 * cin;
        hipLaunchKernelGGL(gemm_kernel<gemm::A_DECONV>, dim3(cdiv(g.M, BM), DEC / BN), dim3(256), 0, st, g);
        TTUP_LAUNCH_CHECK();
    }
    return TTUP_OK;
}

// BN l (0, 1) + ReLU on z, the (4 << 2l) * tokens rows of DEC at level l + 1 -> a
static int run_bn_relu(const ttup_vitpose_head* h, int l, const float* z, long long tokens, int train, const ttup_vitpose_head_params* p, float* a,
                       hipStream_t st) {
    float* bn = h->small(l ? SmallOff::BN2 : SmallOff::BN1);
    const int ns = slices(tokens);
    const long long rows = tokens << (2 * l + 2);
    double* sums = h->buf<double>(B_SUMS);
    if (train) {
        hipLaunchKernelGGL(bn_sums_kernel<false>, dim3(DEC / 64, ns), dim3(1024), 0, st, z, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                           rows, slice_rows(l + 1), sums);
        TTUP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(1), dim3(DEC), 0, st, sums, ns, rows, train, l ? p->bn2_running_mean : p->bn1_running_mean,
                       l ? p->bn2_running_var : p->bn1_running_var, (long long*)(l ? p->bn2_num_batches_tracked : p->bn1_num_batches_tracked), bn);
    TTUP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_relu_kernel, dim3(blocks(rows * (DEC / 4), 256)), dim3(256), 0, st, z, bn, l ? p->bn2_weight : p->bn1_weight,
                       l ? p->bn2_bias : p->bn1_bias, a, rows * (DEC / 4));
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

extern "C" int ttup_vitpose_head_forward(ttup_vitpose_head* h, const float* feat_dev, int batch, int hp, int wp, const ttup_vitpose_head_params* p,
                                         int train, float* heat_dev, void* stream) {
    TTUP_REQUIRE(h && feat_dev && p && heat_dev, TTUP_EINVAL, "ttup_vitpose_head_forward: null argument");
    TTUP_REQUIRE(p->deconv1_weight && p->bn1_weight && p->bn1_bias && p->bn1_running_mean && p->bn1_running_var && p->bn1_num_batches_tracked &&
                 p->deconv2_weight && p->bn2_weight && p->bn2_bias && p->bn2_running_mean && p->bn2_running_var && p->bn2_num_batches_tracked &&
                 p->final_weight && p->final_bias, TTUP_EINVAL, "ttup_vitpose_head_forward: null parameter");
    const Refusal r = check_forward(h->max_rows, batch, hp, wp);
    TTUP_REQUIRE(r.rc == TTUP_OK, r.rc, "%s", r.msg);
    TTUP_REQUIRE(((uintptr_t)feat_dev & 15) == 0, TTUP_EINVAL, "ttup_vitpose_head_forward: the features must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long T = (long long)batch * hp * wp;
    h->batch = 0;                                      // nothing to run a backward on until this forward is complete
    // the weights as the two passes read them, and the features the backward's dW1 reads
    hipLaunchKernelGGL(pack_kernel, dim3(blocks(16LL * DIM * DEC, 256)), dim3(256), 0, st, p->deconv1_weight, DIM, DEC, h->buf(B_WPH1), h->buf(B_WPERM1));
    TTUP_LAUNCH_CHECK();
    hipLaunchKernelGGL(pack_kernel, dim3(blocks(16LL * DEC * DEC, 256)), dim3(256), 0, st, p->deconv2_weight, DEC, DEC, h->buf(B_WPH2), h->buf(B_WPERM2));
    TTUP_LAUNCH_CHECK();
    hipLaunchKernelGGL(keep_small_kernel, dim3(MAX_OUT), dim3(256), 0, st, p->bn1_weight, p->bn2_weight, p->final_weight, h->out_ch, h->buf(B_SMALL));
    TTUP_LAUNCH_CHECK();
    TTUP_HIP_CHECK(hipMemcpyAsync(h->buf(B_FEAT), feat_dev, (size_t)T * DIM * 4, hipMemcpyDeviceToDevice, st));
    VH_RC(run_deconv(h, h->buf(B_FEAT), h->buf(B_WPH1), DIM, batch, hp, wp, h->buf(B_Z1), st));
    VH_RC(run_bn_relu(h, 0, h->buf(B_Z1), T, train != 0, p, h->buf(B_A1), st));
    VH_RC(run_deconv(h, h->buf(B_A1), h->buf(B_WPH2), DEC, batch, 2 * hp, 2 * wp, h->buf(B_Z2), st));
    VH_RC(run_bn_relu(h, 1, h->buf(B_Z2), T, train != 0, p, h->buf(B_A2), st));
    const long long npix = 16 * T;
    hipLaunchKernelGGL(conv1x1_fwd_kernel, dim3(blocks(npix, 64)), dim3(256), 0, st, h->buf(B_A2), npix, 16 * hp * wp, p->final_weight, p->final_bias,
                       h->out_ch, heat_dev);
    TTUP_LAUNCH_CHECK();
    h->batch = batch; h->hp = hp; h->wp = wp; h->train = train != 0;
    return TTUP_OK;
}

// One deconvolution's backward.  On entry d (rows_out x DEC, the level above) holds dy of BN l -- ungated when `gate` is given; on
// return it holds dz, dgamma / dbeta / dw hold that layer's gradients and da (rows_in x cin) the gradient into the layer's input a.
static int run_layer_bwd(const ttup_vitpose_head* h, int l, float* d, const float* z, const float* gate, const float* a, int cin, const float* wperm,
                         float* dgamma, float* dbeta, float* dw, float* da, hipStream_t st) {
    const long long T = (long long)h->batch * h->hp * h->wp;
    const int ih = (l + 1) * h->hp, iw = (l + 1) * h->wp, ns = slices(T);
    const long long rows_in = (long long)h->batch * ih * iw, rows_out = 4 * rows_in;
    float* bn = h->small(l ? SmallOff::BN2 : SmallOff::BN1);
    const float* gamma = h->small(l ? SmallOff::G2 : SmallOff::G1);
    double* sums = h->buf<double>(B_SUMS);
    hipLaunchKernelGGL(bn_sums_kernel<true>, dim3(DEC / 64, ns), dim3(1024), 0, st, z, (const float*)d, gate, (const float*)bn, rows_out, slice_rows(l + 1), sums);
    TTUP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(1), dim3(DEC), 0, st, sums, ns, rows_out, h->train, dgamma, dbeta, bn);
    TTUP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_dz_kernel, dim3(blocks(rows_out * (DEC / 4), 256)), dim3(256), 0, st, d, z, gate, (const float*)bn, gamma, rows_out * (DEC / 4));
    TTUP_LAUNCH_CHECK();
    // dW' (cin, 16 DEC) = a^T G: a read by columns, G gathered from dz, the rows cut into k-slices
    GemmArgs g = {};
    g.a = a; g.lda = cin; g.w = d; g.out = h->buf(B_PARTIAL); g.ldo = 16 * DEC;
    g.M = cin; g.N = 16 * DEC; g.K = (int)rows_in; g.kslice = (int)slice_rows(l);
    g.cin = DEC; g.ih = ih; g.iw = iw;
    hipLaunchKernelGGL((gemm_kernel<gemm::O_COLS, true, gemm::O_DGRAD>), dim3(cdiv(g.M, BM), cdiv(g.N, BN), ns), dim3(256), 0, st, g);
    TTUP_LAUNCH_CHECK();
    hipLaunchKernelGGL(dw_reduce_kernel, dim3(blocks((long long)cin * 16 * DEC, 256)), dim3(256), 0, st, (const float*)h->buf(B_PARTIAL), ns, cin, DEC, dw);
    TTUP_LAUNCH_CHECK();
    // da (rows_in, cin) = G Wperm^T
    GemmArgs q = {};
    q.a = d; q.w = wperm; q.bias = h->small(SmallOff::ZERO); q.out = da;
    q.M = (int)rows_in; q.N = cin; q.K = 16 * DEC; q.cin = DEC; q.ih = ih; q.iw = iw;
    hipLaunchKernelGGL(gemm_kernel<gemm::A_DGRAD>, dim3(cdiv(q.M, BM), cin / BN), dim3(256), 0, st, q);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

extern "C" int ttup_vitpose_head_backward(ttup_vitpose_head* h, const float* dheat_dev, int batch, int hp, int wp, const ttup_vitpose_head_grads* g,
                                          void* stream) {
    TTUP_REQUIRE(h && dheat_dev && g, TTUP_EINVAL, "ttup_vitpose_head_backward: null argument");
    TTUP_REQUIRE(g->deconv1_weight && g->bn1_weight && g->bn1_bias && g->deconv2_weight && g->bn2_weight && g->bn2_bias && g->final_weight && g->final_bias &&
                 g->feat, TTUP_EINVAL, "ttup_vitpose_head_backward: null gradient output");
    const Refusal r = check_backward(h->batch, h->hp, h->wp, batch, hp, wp);
    TTUP_REQUIRE(r.rc == TTUP_OK, r.rc, "%s", r.msg);
    TTUP_REQUIRE(((uintptr_t)g->feat & 15) == 0, TTUP_EINVAL, "ttup_vitpose_head_backward: the feature gradient must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long T = (long long)batch * hp * wp, npix = 16 * T;
    const int ns = slices(T), C = h->out_ch;
    hipLaunchKernelGGL(conv1x1_bwd_kernel, dim3(blocks(npix * (DEC / 4), 256)), dim3(256), 0, st, dheat_dev, (const float*)h->buf(B_A2),
                       (const float*)h->small(SmallOff::WF), npix, 16 * hp * wp, C, h->buf(B_D2));
    TTUP_LAUNCH_CHECK();
    hipLaunchKernelGGL(dwf_partial_kernel, dim3(ns * DWF_SUB), dim3(DEC), 0, st, dheat_dev, (const float*)h->buf(B_A2), npix, 16 * hp * wp, C, slice_rows(2),
                       h->buf<double>(B_DWF));
    TTUP_LAUNCH_CHECK();
    hipLaunchKernelGGL(dwf_finalize_kernel, dim3(blocks(C * DEC + C, 256)), dim3(256), 0, st, (const double*)h->buf<double>(B_DWF), ns * DWF_SUB, C,
                       g->final_weight, g->final_bias);
    TTUP_LAUNCH_CHECK();
    VH_RC(run_layer_bwd(h, 1, h->buf(B_D2), h->buf(B_Z2), nullptr, h->buf(B_A1), DEC, h->buf(B_WPERM2), g->bn2_weight, g->bn2_bias, g->deconv2_weight,
                        h->buf(B_D1), st));
    return run_layer_bwd(h, 0, h->buf(B_D1), h->buf(B_Z1), h->buf(B_A1), h->buf(B_FEAT), DIM, h->buf(B_WPERM1), g->bn1_weight, g->bn1_bias,
                         g->deconv1_weight, g->feat, st);
}

// The testing seam: what the last forward kept.  z1 / a1 (batch, 2hp, 2wp, 256) and z2 / a2 (batch, 4hp, 4wp, 256) NHWC; mean1, var1,
// mean2, var2 (256): the statistics the BN used (train: the batch's mean and biased variance; eval: the running ones)
extern "C" int ttup_vitpose_head_read_tap(ttup_vitpose_head* h, const char* tap, void* dst, size_t bytes) {
    TTUP_REQUIRE(h && tap && dst, TTUP_EINVAL, "ttup_vitpose_head_read_tap: null argument");
    TTUP_REQUIRE(h->batch > 0, TTUP_EINVAL, "ttup_vitpose_head_read_tap: no forward has run on this handle");
    const size_t T = (size_t)h->batch * h->hp * h->wp;
    const struct { const char* name; const float* src; size_t count; } taps[] = {
        {"z1", h->buf(B_Z1), T * 4 * DEC}, {"a1", h->buf(B_A1), T * 4 * DEC}, {"z2", h->buf(B_Z2), T * 16 * DEC}, {"a2", h->buf(B_A2), T * 16 * DEC},
        {"mean1", h->small(SmallOff::BN1 + S_MEAN * DEC), (size_t)DEC}, {"var1", h->small(SmallOff::BN1 + S_VAR * DEC), (size_t)DEC},
        {"mean2", h->small(SmallOff::BN2 + S_MEAN * DEC), (size_t)DEC}, {"var2", h->small(SmallOff::BN2 + S_VAR * DEC), (size_t)DEC},
    };
    for (const auto& t : taps) {
        if (strcmp(tap, t.name) != 0) continue;
        TTUP_REQUIRE(bytes == t.count * 4, TTUP_EINVAL, "ttup_vitpose_head_read_tap: tap '%s' has %zu bytes, the buffer %zu", tap, t.count * 4, bytes);
        TTUP_HIP_CHECK(hipDeviceSynchronize());
        TTUP_HIP_CHECK(hipMemcpy(dst, t.src, bytes, hipMemcpyDefault));
        return TTUP_OK;
    }
    ttup::set_error("ttup_vitpose_head_read_tap: unknown tap '%s'", tap);
    return TTUP_EINVAL;
}
#include "no_packed_fp32_end.h"
