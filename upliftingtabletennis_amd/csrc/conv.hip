// Implicit-GEMM convolution for the WASB/HRNet CNN on gfx950 (reference: balldetection/models/wasb.py
// conv/BN/ReLU/residual call sites :48-64, :85-105, :227-245, :446-451).
//
// GEMM view (per output tile):  D[cout][pixel] = sum_k  W[cout][k] * X[k][pixel],   k = (tap, cin)
//   A operand = weights  (M = cout, 16 per MFMA tile), pre-packed on the host in fragment order
//   B operand = pixels   (N = 16 consecutive output x of one row), read from an LDS halo tile
//   v_mfma_f32_16x16x32_bf16, fp32 accumulators; epilogue = +bias (+residual) (ReLU) -> bf16 NHWC.
// A lane ends up with 4*MT consecutive output channels of one pixel (the cout permutation is folded
// into the weight packing), so stores are 8..64 contiguous bytes per lane and a wave writes whole
// 16-pixel NHWC runs.
#include "conv_mfma.h"
#include "conv64.h"
#include "conv_stem.h"
#include "conv_bneck.h"
#include "conv_bb.h"
#include "chain16.h"
#include "conv_pointwise.h"

namespace ttup {

int launch_stem(const PackedConv& p1, const PackedConv& p2, const PackedConv& p3, const void* x0, void* t2, void* a1,
                int batch, int h, int w, hipStream_t st, int frames_per_sample) {
    TTUP_REQUIRE((p1.cout == 64 && p1.cin_total == 16 && p1.k == 3 && p1.stride == 1 && p1.ck == 16) ||
                 (p1.cout == 64 && p1.cin_total == 128 && p1.k == 1 && p1.ck == 32), TTUP_EINVAL, "stem: unexpected conv1 shape");
    TTUP_REQUIRE(p2.cout == 64 && p2.cin_total == 64 && p2.k == 3 && p2.stride == 1 && p2.ck == 32, TTUP_EINVAL, "stem: unexpected conv2 shape");
    TTUP_REQUIRE(p3.cout == 32 && p3.cin_total == 64 && p3.k == 1 && p3.ck == 32, TTUP_EINVAL, "stem: unexpected follower shape");
    StemArgs a;
    a.x0 = (const bf16_t*)x0; a.w1 = (const bf16_t*)p1.w_dev; a.b1 = p1.bias_dev; a.w2 = (const bf16_t*)p2.w_dev; a.b2 = p2.bias_dev;
    a.w3 = (const bf16_t*)p3.w_dev; a.b3 = p3.bias_dev; a.t2 = (bf16_t*)t2; a.a1 = (bf16_t*)a1;
    a.H = h; a.W = w; a.tiles_x = cdiv(w, 32); a.tiles_per_img = a.tiles_x * cdiv(h, 8); a.total_tiles = a.tiles_per_img * batch;
    constexpr size_t SMEM = (size_t)(5 * 4 * 64 * 8 + 2 * 9 * 4 * 64 * 8 + 2 * 340 * 32 + 432 * 16) * 2;          // (the 4-step form needs 7.5 KB less; one size for all)
    static_assert(SMEM <= 160 * 1024, "LDS budget");
    TTUP_REQUIRE(frames_per_sample == 0 || frames_per_sample == 1 || frames_per_sample == 3, TTUP_EINVAL, "stem: frames per sample must be 0 (X0 records), 1 or 3");
    const bool k4 = p1.k == 1;          // conv1 packed as 128 slots x 1 tap: the 4-step three-frame form (csrc/wasb_graph.h)
    TTUP_REQUIRE(k4 == (frames_per_sample == 3), TTUP_EINVAL, "stem: the 4-step conv1 packing is the three-frame form");
    // (a two-wave-group pipeline of the stem, round 5: 14 % slower -- git show d528471:upliftingtabletennis_amd/csrc/experiments/rejected_kernels.hip.inc)
    const dim3 grid(persistent_grid(a.total_tiles));
    if (k4) return launch_noted(stem_kernel<3, true>, grid, 512, SMEM, st, a, "stem_kernel<3, true>");
    if (frames_per_sample == 1) return launch_noted(stem_kernel<1, false>, grid, 512, SMEM, st, a, "stem_kernel<1, false>");
    return launch_noted(stem_kernel<0, false>, grid, 512, SMEM, st, a, "stem_kernel<0, false>");
}

int launch_bneck_trans(const PackedConv& p1, const PackedConv& p5, const PackedConv& p6, const void* a2, const void* t2,
                       void* b0, void* b1, int batch, int h, int w, hipStream_t st) {
    TTUP_REQUIRE(p1.cout == 128 && p1.cin_total == 96 && p1.c0 == 32 && p1.k == 1 && p1.ck == 32, TTUP_EINVAL, "bneck_trans: unexpected conv1 shape");
    TTUP_REQUIRE(p5.cout == 16 && p5.cin_total == 128 && p5.k == 3 && p5.stride == 1 && p5.ck == 32, TTUP_EINVAL, "bneck_trans: unexpected conv5 shape");
    TTUP_REQUIRE(p6.cout == 32 && p6.cin_total == 128 && p6.k == 3 && p6.stride == 2 && p6.ck == 32, TTUP_EINVAL, "bneck_trans: unexpected conv6 shape");
    TTUP_REQUIRE(h % 2 == 0 && w % 2 == 0, TTUP_EINVAL, "bneck_trans: even input size required");
    FusedArgs a;
    a.a2 = (const bf16_t*)a2; a.t2 = (const bf16_t*)t2;
    a.w1 = (const bf16_t*)p1.w_dev; a.b1 = p1.bias_dev; a.w5 = (const bf16_t*)p5.w_dev; a.b5 = p5.bias_dev;
    a.w6 = (const bf16_t*)p6.w_dev; a.b6 = p6.bias_dev; a.b0 = (bf16_t*)b0; a.b1o = (bf16_t*)b1;
    a.H = h; a.W = w; a.tiles_x = cdiv(w, 32); a.tiles_per_img = a.tiles_x * cdiv(h, 8); a.total_tiles = a.tiles_per_img * batch;
    constexpr size_t SMEM = (size_t)(340 * 128 + 3 * 8 * 64 * 8 + 4 * 9 * 64 * 8) * 2 + 512;
    return launch_noted(bneck_trans_kernel, dim3(persistent_grid(a.total_tiles)), 512, SMEM, st, a, "bneck_trans_kernel");
}

// tile of the C=16 two-block chain (multiples of 8: the fuse-term slices are aligned to the tile)
constexpr int BB2_TH = 24, BB2_TW = 32;
int bb_chain_tiles_per_img(int h, int w) { return cdiv(w, BB2_TW) * cdiv(h, BB2_TH); }

int launch_bb_chain(const PackedConv* const* convs, int n_convs, const void* x, void* y, int batch, int h, int w,
                    const PackedConv* follow, void* y_follow, hipStream_t st, const BBSum* sum) {
    TTUP_REQUIRE(n_convs == 2 || n_convs == 4, TTUP_EINVAL, "bb_chain: 2 or 4 convs expected");
    const int c = convs[0]->cout;
    BBArgs a;
    a.x = (const bf16_t*)x; a.y = (bf16_t*)y;
    if (sum) {
        TTUP_REQUIRE(c == 16 && n_convs == 4 && sum->n_terms >= 0 && sum->n_terms <= 3, TTUP_EINVAL, "bb_chain: the fused fuse-layer sum rides on the 16-channel two-block chain");
        TTUP_REQUIRE(sum->ysum || (sum->heat && sum->head_w && sum->pv && sum->pi), TTUP_EINVAL, "bb_chain: fused sum needs an output");
        a.nsum = sum->n_terms; a.ysum = (bf16_t*)sum->ysum;
        for (int k = 0; k < sum->n_terms; ++k) { a.st[k] = (const bf16_t*)sum->terms[k]; a.ssh[k] = sum->shifts[k]; }
        a.heat = sum->heat; a.hw = sum->head_w; a.hbias = sum->head_bias; a.pv = sum->pv; a.pi = sum->pi;
    }
    if (follow) {
        TTUP_REQUIRE(c == 32 && n_convs == 2 && follow->cout == 16 && follow->cin_total == 32 && follow->k == 1 && follow->ck == 32 && y_follow, TTUP_EINVAL,
                     "bb_chain: the fused follower is a 1x1 32->16 conv on a 32-channel block");
        a.wf = (const bf16_t*)follow->w_dev; a.bf = follow->bias_dev; a.yf = (bf16_t*)y_follow;
    }
    for (int i = 0; i < n_convs; ++i) {
        const PackedConv& p = *convs[i];
        TTUP_REQUIRE(p.cout == c && p.cin_total == c && p.k == 3 && p.stride == 1 && p.ck == (c == 16 ? 16 : 32), TTUP_EINVAL, "bb_chain: unexpected conv shape");
        a.w[i] = (const bf16_t*)p.w_dev; a.bias[i] = p.bias_dev;
    }
    // tile shapes tuned on MI355X: larger tiles amortise the per-tile overhead and waste fewer ragged 16-pixel MFMA groups
    if (c == 16 && n_convs == 4) {
        // the epilogue forms the network uses are compiled out in c16_chain_kernel (csrc/chain16.h); anything else -- other term layouts,
        // TTUP_BB2_GENERIC=1 (read once per process) -- takes the run-time form (bb_chain2_kernel)
        static const bool generic = env_set("TTUP_BB2_GENERIC");
        bool shifts_ok = true;          // the compiled-out forms assume term k at 1/2^(k+1) resolution (HRNet's fuse layers)
        for (int k = 0; k < a.nsum && k < 3; ++k) shifts_ok = shifts_ok && a.ssh[k] == k + 1;
        const bool sum_stored = !generic && shifts_ok && a.nsum >= 1 && a.nsum <= 3 && a.ysum && !a.heat;      // a.y (the pre-fuse tensor) optional
        const bool tail = !generic && shifts_ok && a.nsum == 3 && a.heat && !a.y && !a.ysum;
        const bool plain = !generic && a.nsum == 0 && !a.heat && !a.ysum && a.y;
        if (plain) return launch_c16_t<BB2_TH, BB2_TW, 4>(a, batch, h, w, st);
        if (tail) return launch_c16_t<BB2_TH, BB2_TW, 7>(a, batch, h, w, st);
        if (sum_stored && a.nsum == 1) return launch_c16_t<BB2_TH, BB2_TW, 1>(a, batch, h, w, st);
        if (sum_stored && a.nsum == 2) return launch_c16_t<BB2_TH, BB2_TW, 2>(a, batch, h, w, st);
        if (sum_stored && a.nsum == 3) return launch_c16_t<BB2_TH, BB2_TW, 3>(a, batch, h, w, st);
        return launch_bb2_t<16, BB2_TH, BB2_TW>(a, batch, h, w, st);
    }
    if (c == 16 && n_convs == 2) return launch_bb_t<16, 8, 32>(a, batch, h, w, st);
    if (c == 32 && n_convs == 2) {
        // (a two-wave-group pipeline of this block, round 5: bit-identical and 1.5 % slower -- git show d528471:upliftingtabletennis_amd/csrc/experiments/rejected_kernels.hip.inc)
        return launch_bb_t<32, 22, 30>(a, batch, h, w, st);                   // conv regions 24x32 / 22x30
    }
    set_error("bb_chain: C=%d with %d convs unsupported", c, n_convs);
    return TTUP_EINVAL;
}

// ------------------------------------------------------------------ host side: packing
void free_conv(PackedConv* p) {
    if (p->w_dev) (void)hipFree(p->w_dev);
    if (p->bias_dev) (void)hipFree(p->bias_dev);
    if (p->w3_dev) (void)hipFree(p->w3_dev);
    p->w_dev = nullptr; p->bias_dev = nullptr; p->w3_dev = nullptr;
}

int pack_conv(const FoldedConv& a, const FoldedConv* b, int cin_pad, int dtype, PackedConv* out) {
    const int k = a.k, taps = k * k, cout = a.cout;
    const int c0 = cin_pad > a.cin ? cin_pad : a.cin;
    const int c1 = b ? b->cin : 0;
    TTUP_REQUIRE(!b || (b->cout == cout && b->k == k && k == 1), TTUP_EINVAL, "two-source conv needs matching 1x1 convs");
    TTUP_REQUIRE(cout % 16 == 0 && cout <= 128, TTUP_EINVAL, "cout %d unsupported", cout);
    const int cin_total = c0 + c1;
    out->cout = cout; out->cin_total = cin_total; out->c0 = c0; out->k = k; out->stride = a.stride;
    std::vector<float> bias(cout);
    for (int i = 0; i < cout; ++i) bias[i] = a.bias[i] + (b ? b->bias[i] : 0.f);
    auto wval = [&](int co, int ci, int tap) -> float {
        if (ci < c0) return ci < a.cin ? a.w[((size_t)co * a.cin + ci) * taps + tap] : 0.f;
        return b->w[((size_t)co * b->cin + (ci - c0)) * taps + tap];
    };
    TTUP_HIP_CHECK(hipMalloc((void**)&out->bias_dev, cout * sizeof(float)));
    TTUP_HIP_CHECK(hipMemcpy(out->bias_dev, bias.data(), cout * sizeof(float), hipMemcpyHostToDevice));
    if (dtype == TTUP_DTYPE_F32) {
        std::vector<float> w((size_t)taps * cin_total * cout);
        for (int t = 0; t < taps; ++t)
            for (int ci = 0; ci < cin_total; ++ci)
                for (int co = 0; co < cout; ++co) w[((size_t)t * cin_total + ci) * cout + co] = wval(co, ci, t);
        out->w_bytes = w.size() * sizeof(float);
        out->ck = 0;
        TTUP_HIP_CHECK(hipMalloc(&out->w_dev, out->w_bytes));
        TTUP_HIP_CHECK(hipMemcpy(out->w_dev, w.data(), out->w_bytes, hipMemcpyHostToDevice));
        return pack_conv_x3(w, cout, cin_total, c0, k, a.stride, out);          // + the split-bf16 packing of the same weights (sets ck)
    }
    TTUP_REQUIRE(c0 % 16 == 0 && c1 % 32 == 0, TTUP_EINVAL, "channel counts %d+%d unsupported", c0, c1);
    int ck = (c0 % 32 == 0) ? 32 : 16;
    TTUP_REQUIRE(ck == 32 || (c1 == 0 && k == 3), TTUP_EINVAL, "16-channel chunks only for single-source 3x3");
    const int mt = cout / 16, ksteps = ck == 32 ? taps : (taps + 1) / 2, nchunk = cin_total / ck;
    std::vector<bf16_t> w((size_t)nchunk * ksteps * mt * 64 * 8);
    size_t idx = 0;
    for (int c = 0; c < nchunk; ++c)
        for (int s = 0; s < ksteps; ++s)
            for (int m = 0; m < mt; ++m)
                for (int l = 0; l < 64; ++l) {
                    const int i = l & 15, g = l >> 4;
                    const int co = (i >> 2) * (4 * mt) + m * 4 + (i & 3);
                    for (int j = 0; j < 8; ++j) {
                        int tap, ci;
                        if (ck == 32) { tap = s; ci = c * 32 + 8 * g + j; }
                        else { tap = 2 * s + (g >> 1); ci = c * 16 + 8 * (g & 1) + j; }
                        w[idx++] = f32_to_bf16(tap < taps ? wval(co, ci, tap) : 0.f);
                    }
                }
    out->ck = ck;
    out->w_bytes = w.size() * sizeof(bf16_t);
    TTUP_HIP_CHECK(hipMalloc(&out->w_dev, out->w_bytes));
    TTUP_HIP_CHECK(hipMemcpy(out->w_dev, w.data(), out->w_bytes, hipMemcpyHostToDevice));
    return TTUP_OK;
}

int launch_conv(const PackedConv& p, const ConvLaunch& l, int dtype, hipStream_t st) {
    if (dtype == TTUP_DTYPE_F32) {
        TTUP_REQUIRE(!l.res2 && !l.res3, TTUP_EINVAL, "conv: extra fuse-layer terms are a bf16-path fusion");
        static const bool direct = env_set("TTUP_F32_DIRECT");        // cross-checks: one thread per output, plain fp32 fma chain
        static const bool exact = env_set("TTUP_F32_EXACT");          // ... / exact fp32 products on the fp32 matrix pipe
        if (!direct && !exact && conv_x3_supported(p)) return launch_conv_x3(p, l, st);
        if (!direct && conv_f32_mfma_supported(p)) return launch_conv_f32_mfma(p, l, st);
        TTUP_REQUIRE(!l.n_active, TTUP_EINVAL, "conv: a device-side batch needs the matrix-pipe fp32 kernel");
        ConvFArgs a;
        a.src0 = (const float*)l.src0; a.src1 = (const float*)l.src1; a.w = (const float*)p.w_dev; a.bias = p.bias_dev;
        a.residual = (const float*)l.residual; a.dst = (float*)l.dst;
        a.c0 = p.c0; a.c1 = p.cin_total - p.c0; a.cout = p.cout; a.ks = p.k; a.stride = p.stride;
        a.H = l.h; a.W = l.w; a.OH = (l.h + p.stride - 1) / p.stride; a.OW = (l.w + p.stride - 1) / p.stride; a.relu = l.relu;
        a.total = (long long)l.batch * a.OH * a.OW * a.cout;
        const int threads = 256;
        const long long blocks = (a.total + threads - 1) / threads;
        kernel_note("conv_direct_f32_kernel");
        hipLaunchKernelGGL(conv_direct_f32_kernel, dim3((unsigned)blocks), dim3(threads), 0, st, a);
        TTUP_LAUNCH_CHECK();
        return TTUP_OK;
    }
    TTUP_REQUIRE(!(l.res2 || l.res3) || (p.stride == 2 && !l.follow), TTUP_EINVAL, "conv: extra fuse-layer terms ride on the stride-2 chain convs only");
    if (l.follow) {
        TTUP_REQUIRE(p.k == 3 && p.stride == 1 && p.ck == 32 && p.cout == 64, TTUP_EINVAL, "conv: fused follower needs a 3x3 s1 conv with 64 outputs");
        return launch_mfma<32, 64, 3, 1, 8, 32, 8, true>(p, l, st);
    }
    if (p.k == 3 && p.stride == 1 && p.ck == 32 && p.cout == 64 && p.cin_total == 64 && p.c0 == 64 && !l.src1) return launch_conv64(p, l, st);
    if (l.pair) return launch_s2_pair(p, l, st);
    TTUP_REQUIRE(!l.lin16 && !l.lin32, TTUP_EINVAL, "conv: linear 1x1 followers ride on the 64 -> 64 3x3 kernel only");
    if (p.k == 3 && p.stride == 1) return p.ck == 32 ? dispatch_cout<32, 3, 1, 8, 32>(p, l, st) : dispatch_cout<16, 3, 1, 8, 32>(p, l, st);
    if (p.k == 3 && p.stride == 2) return p.ck == 32 ? dispatch_cout<32, 3, 2, 4, 32>(p, l, st) : dispatch_cout<16, 3, 2, 4, 32>(p, l, st);
    if (p.k == 1 && p.stride == 1 && p.ck == 32) return dispatch_cout<32, 1, 1, 8, 32>(p, l, st);
    set_error("conv: k=%d stride=%d ck=%d unsupported", p.k, p.stride, p.ck);
    return TTUP_EINVAL;
}

int launch_upsum(const void* base, const void* const* terms, const int* shifts, int n_terms, void* dst,
                 int batch, int h, int w, int c, int dtype, hipStream_t stream, const int* n_active, const Roi* roi) {
    UpsumArgs a;
    a.base = base; a.n = n_terms; a.dst = dst; a.H = h; a.W = w; a.C = c; a.batch = batch;
    if (roi) a.roi = *roi;
    TTUP_REQUIRE(!a.roi.flag || dtype == TTUP_DTYPE_F32, TTUP_EINVAL, "upsum: output regions are an fp32-path feature");
    for (int k = 0; k < 3; ++k) { a.t[k] = k < n_terms ? terms[k] : nullptr; a.shift[k] = k < n_terms ? shifts[k] : 0; }
    a.total = (long long)batch * h * w * c;
    a.n_active = n_active; a.per_sample = (long long)h * w * c;
    if (a.total == 0) return TTUP_OK;
    long long blocks = (a.total + 255) / 256;
    if (n_active && blocks > 8192) blocks = 8192;             // grid-stride: the launch is sized for the largest batch
    TTUP_REQUIRE(!n_active || dtype == TTUP_DTYPE_F32, TTUP_EINVAL, "upsum: a device-side batch is an fp32-path feature");
    kernel_note(dtype == TTUP_DTYPE_F32 ? "upsum_kernel<float>" : c % 8 == 0 ? "upsum_bf16x8_kernel" : "upsum_kernel<bf16>");
    if (dtype == TTUP_DTYPE_F32) hipLaunchKernelGGL(upsum_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    else if (c % 8 == 0) {
        a.total /= 8;
        hipLaunchKernelGGL(upsum_bf16x8_kernel, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, stream, a);
    } else hipLaunchKernelGGL(upsum_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

int launch_nchw_to_nhwc(const float* src, void* dst, int batch, int cin, int cpad, int h, int w, int dtype, hipStream_t stream) {
    const long long total = (long long)batch * h * w * cpad;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (dtype == TTUP_DTYPE_F32) hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, dim3(blocks), dim3(256), 0, stream, src, (float*)dst, cin, cpad, h * w, total);
    else hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16_t>, dim3(blocks), dim3(256), 0, stream, src, (bf16_t*)dst, cin, cpad, h * w, total);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

int launch_nhwc_to_nchw(const void* src, float* dst, int batch, int c, int h, int w, int dtype, hipStream_t stream) {
    const long long total = (long long)batch * h * w * c;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (dtype == TTUP_DTYPE_F32) hipLaunchKernelGGL(nhwc_to_nchw_kernel<float>, dim3(blocks), dim3(256), 0, stream, (const float*)src, dst, c, h * w, total);
    else hipLaunchKernelGGL(nhwc_to_nchw_kernel<bf16_t>, dim3(blocks), dim3(256), 0, stream, (const bf16_t*)src, dst, c, h * w, total);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

int launch_head(const void* src, const float* w_dev, const float* bias_dev, int n_out, float* heat, int batch, int h, int w, int cin, int dtype,
                hipStream_t stream, const int* n_active, const Roi* roi) {
    const Roi r = roi ? *roi : Roi();
    TTUP_REQUIRE(cin == 16, TTUP_EINVAL, "head expects 16 input channels, got %d", cin);
    const long long hw = (long long)h * w, npix = (long long)batch * hw;
    if (npix == 0) return TTUP_OK;
    long long blocks = (npix + 255) / 256;
    if (n_active && blocks > 8192) blocks = 8192;
    if (dtype == TTUP_DTYPE_F32) hipLaunchKernelGGL((head_kernel<float, 16>), dim3((unsigned)blocks), dim3(256), 0, stream, (const float*)src, w_dev, bias_dev, n_out, heat, hw, npix, n_active, r, w);
    else hipLaunchKernelGGL((head_kernel<bf16_t, 16>), dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16_t*)src, w_dev, bias_dev, n_out, heat, hw, npix, n_active, r, w);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

int launch_preprocess(const uint8_t* frames, int n_frames, int src_h, int src_w, int dst_h, int dst_w,
                      void* out, int out_layout, int dtype, int first_triple, int n_triples, int frames_per_sample, hipStream_t stream) {
    TTUP_REQUIRE(frames_per_sample == 1 || frames_per_sample == 3, TTUP_EINVAL, "frames_per_sample must be 1 or 3");
    TTUP_REQUIRE(first_triple >= 0 && first_triple + n_triples + frames_per_sample - 1 <= n_frames, TTUP_EINVAL, "sample range outside the clip");
    PreArgs a;
    a.frames = frames; a.out = out; a.src_h = src_h; a.src_w = src_w; a.dst_h = dst_h; a.dst_w = dst_w;
    a.first_triple = first_triple; a.n_triples = n_triples; a.layout = out_layout; a.nf = frames_per_sample;
    a.total = (long long)n_triples * dst_h * dst_w;
    a.scale_x = (double)src_w / dst_w; a.scale_y = (double)src_h / dst_h;
    a.crops = nullptr; a.n_active = nullptr; a.crop0 = 0; a.crop_h = 0; a.crop_w = 0;
    if (a.total == 0) return TTUP_OK;
    if (int rc = device_normalise_lut(&a.lut)) return rc;       // one table per device
    TTUP_REQUIRE(dst_h <= 65535 && n_triples <= 65535, TTUP_EINVAL, "preprocess: grid limit (rows, samples <= 65535)");
    const dim3 grid((unsigned)cdiv(dst_w, 256), (unsigned)dst_h, (unsigned)n_triples);
    TTUP_REQUIRE(out_layout != TTUP_LAYOUT_NHWC4_FRAME || (frames_per_sample == 1 && dtype == TTUP_DTYPE_BF16), TTUP_EINVAL, "per-frame records are bf16, one frame per sample");
    static const bool no_fast = env_set("TTUP_NO_PRE4");
    if (out_layout == TTUP_LAYOUT_NHWC4_FRAME && src_w == dst_w && dst_w % 4 == 0 && ((size_t)frames & 3) == 0 && !no_fast)      // aligned 12-byte row loads
        hipLaunchKernelGGL(preprocess_frames4_kernel, dim3((unsigned)cdiv(dst_w, 1024), (unsigned)cdiv(dst_h, PRE4_ROWS), (unsigned)n_triples), dim3(256), 0, stream, a);
    else if ((dtype == TTUP_DTYPE_F32 || out_layout == TTUP_LAYOUT_NCHW_F32) && out_layout != TTUP_LAYOUT_NHWC4_FRAME)
        hipLaunchKernelGGL(preprocess_kernel<float>, grid, dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(preprocess_kernel<bf16_t>, grid, dim3(256), 0, stream, a);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

// crop mode: fp32 NHWC16 windows of the pre-processed triples, chosen on the device (csrc/certify.hip)
int launch_preprocess_crops(const uint8_t* frames, int n_frames, int src_h, int src_w, int dst_h, int dst_w, float* out,
                            const CropRec* crops_dev, int crop0, const int* n_active_dev, int max_crops, int crop_h, int crop_w,
                            int frames_per_sample, hipStream_t stream) {
    PreArgs a;
    a.frames = frames; a.out = out; a.src_h = src_h; a.src_w = src_w; a.dst_h = dst_h; a.dst_w = dst_w;
    a.first_triple = 0; a.n_triples = n_frames - frames_per_sample + 1; a.layout = TTUP_LAYOUT_NHWC16; a.nf = frames_per_sample;
    a.total = (long long)max_crops * crop_h * crop_w;
    a.scale_x = (double)src_w / dst_w; a.scale_y = (double)src_h / dst_h;
    a.crops = crops_dev; a.n_active = n_active_dev; a.crop0 = crop0; a.crop_h = crop_h; a.crop_w = crop_w;
    if (a.total == 0) return TTUP_OK;
    if (int rc = device_normalise_lut(&a.lut)) return rc;
    TTUP_REQUIRE(a.total < (1ll << 32), TTUP_EINVAL, "preprocess crops: more than 2^32 crop pixels");
    hipLaunchKernelGGL(preprocess_kernel<float>, dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, stream, a);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

}  // namespace ttup
