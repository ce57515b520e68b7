// a2: the WASB / HRNet ball-heatmap CNN as a static op list over NHWC buffers.  This unit turns a device-free plan of the graph
// (csrc/wasb_graph.h, from the folded convs of csrc/wasb_blob.h) into a handle, runs it (run_op, run_head_op, forward_micro,
// forward_impl), prunes the fp32 crop net to a cone (compute_roi) and carries the C ABI; the timing entry points are in
// csrc/wasb_timing.h.  It launches kernels and holds none.
#include "wasb_net.h"
#include "wasb_blob.h"
#include <string.h>
#include <stdlib.h>
#include <memory>

using namespace ttup;

ttup_wasb::~ttup_wasb() {
    cert_free(this);
    for (auto& c : convs) free_conv(&c);
    for (auto& L : lanes) {
        for (void* q : L.ptr) if (q) (void)hipFree(q);
        if (L.heat_scratch) (void)hipFree(L.heat_scratch);
        if (L.refine_ws) (void)hipFree(L.refine_ws);
        if (L.argmax_scratch) (void)hipFree(L.argmax_scratch);
        if (L.win_scratch) (void)hipFree(L.win_scratch);
        if (L.stream) (void)hipStreamDestroy(L.stream);
        if (L.done) (void)hipEventDestroy(L.done);
    }
    if (fork) (void)hipEventDestroy(fork);
    if (pass_done) (void)hipEventDestroy(pass_done);
    if (head_w_dev) (void)hipFree(head_w_dev);
    if (head_b_dev) (void)hipFree(head_b_dev);
}

namespace {

// the packed convs of a block chain and the terms of the fuse-layer sum in its epilogue
void chain_args(const ttup_wasb* net, const Op& op, const PackedConv* cv[4], BBSum* sum) {
    for (int k = 0; k < 4; ++k) cv[k] = k < op.n_chain ? &net->convs[op.chain[k]] : nullptr;
    sum->n_terms = op.n_terms;
    for (int k = 0; k < op.n_terms; ++k) { sum->terms[k] = net->tensors[op.terms[k]].ptr; sum->shifts[k] = op.shifts[k]; }
}

int run_op(ttup_wasb* net, const Op& op, int mb, hipStream_t st) {
    if (op.kind == Op::CONV) {
        const Tensor& s = net->tensors[op.src0];
        ConvLaunch l;
        l.src0 = s.ptr; l.src1 = op.src1 >= 0 ? net->tensors[op.src1].ptr : nullptr;
        l.residual = op.residual >= 0 ? net->tensors[op.residual].ptr : nullptr;
        l.dst = net->tensors[op.dst].ptr; l.batch = mb; l.h = s.h; l.w = s.w; l.relu = op.relu; l.n_active = net->n_active;
        if (!net->op_roi.empty() && net->roi_flag) { l.roi = net->op_roi[&op - net->ops.data()]; l.roi.flag = net->roi_flag; }
        if (op.conv2 >= 0) { l.follow = &net->convs[op.conv2]; l.dst2 = net->tensors[op.dst2].ptr; }
        if (op.lin16 >= 0) { l.lin16 = &net->convs[op.lin16]; l.lin16_dst = net->tensors[op.lin16_dst].ptr; }
        if (op.lin32 >= 0) { l.lin32 = &net->convs[op.lin32]; l.lin32_dst = net->tensors[op.lin32_dst].ptr; }
        if (op.pair >= 0) { l.pair = &net->convs[op.pair]; l.pair_dst = net->tensors[op.pair_dst].ptr; l.pair_relu = op.pair_relu; }
        if (op.res2 >= 0) l.res2 = net->tensors[op.res2].ptr;
        if (op.res3 >= 0) { l.res3 = net->tensors[op.res3].ptr; l.sh3 = op.sh3; }
        const int rc = launch_conv(net->convs[op.conv], l, net->dtype, st);
        if (rc) return rc;
    } else if (op.kind == Op::STEM) {
        const Tensor& s = net->tensors[op.src0];
        const bool fm = net->frames_mode && net->t_frames >= 0 && op.conv1f >= 0;
        const int rc = launch_stem(net->convs[fm ? op.conv1f : op.conv], net->convs[op.conv2], net->convs[op.conv3], fm ? net->tensors[net->t_frames].ptr : s.ptr,
                                   net->tensors[op.dst].ptr, net->tensors[op.dst2].ptr, mb, s.h, s.w, st, fm ? net->in_ch / 3 : 0);
        if (rc) return rc;
    } else if (op.kind == Op::UPSUM_HEAD) {
        return TTUP_OK;       // launched by forward_micro (run_head_op), which knows the output buffers
    } else if (op.kind == Op::BB_CHAIN) {
        if (op.head) return TTUP_OK;      // launched by forward_micro (run_head_op), which knows the output buffers
        const Tensor& s = net->tensors[op.src0];
        const PackedConv* cv[4]; BBSum sum;
        chain_args(net, op, cv, &sum);
        int rc;
        if (op.n_chain == 4 && op.n_terms > 0) {          // fuse-layer sum in the epilogue: dst2 = relu(dst + sum up(terms))
            sum.ysum = net->tensors[op.dst2].ptr;
            rc = launch_bb_chain(cv, 4, s.ptr, op.dst >= 0 ? net->tensors[op.dst].ptr : nullptr, mb, s.h, s.w, nullptr, nullptr, st, &sum);
        } else {
            rc = launch_bb_chain(cv, op.n_chain, s.ptr, net->tensors[op.dst].ptr, mb, s.h, s.w,
                                 op.conv2 >= 0 ? &net->convs[op.conv2] : nullptr, op.dst2 >= 0 ? net->tensors[op.dst2].ptr : nullptr, st);
        }
        if (rc) return rc;
    } else if (op.kind == Op::BNECK_TRANS) {
        const Tensor& s = net->tensors[op.src0];
        const int rc = launch_bneck_trans(net->convs[op.conv], net->convs[op.conv2], net->convs[op.conv3], s.ptr, net->tensors[op.src1].ptr,
                                          net->tensors[op.dst].ptr, net->tensors[op.dst2].ptr, mb, s.h, s.w, st);
        if (rc) return rc;
    } else {
        const Tensor& d = net->tensors[op.dst];
        const void* terms[3] = {nullptr, nullptr, nullptr};
        for (int k = 0; k < op.n_terms; ++k) terms[k] = net->tensors[op.terms[k]].ptr;
        Roi roi;
        if (!net->op_roi.empty() && net->roi_flag) { roi = net->op_roi[&op - net->ops.data()]; roi.flag = net->roi_flag; }
        const int rc = launch_upsum(net->tensors[op.src0].ptr, terms, op.shifts, op.n_terms, d.ptr, mb, d.h, d.w, d.c, net->dtype, st, net->n_active, &roi);
        if (rc) return rc;
    }
    return TTUP_OK;
}

int run_graph(ttup_wasb* net, int mb, hipStream_t st) {
    for (const Op& op : net->ops) { const int rc = run_op(net, op, mb, st); if (rc) return rc; }
    return TTUP_OK;
}

// the fused last op of the bf16 ball path: stage-4 fuse sum + head + argmax partials (+ window gather)
int run_head_op(ttup_wasb* net, int mb, float* heat, long long* am, float* wn, hipStream_t st) {
    const Op& op = net->ops.back();
    if (op.kind == Op::BB_CHAIN) {
        // last block chain of the full-resolution branch + stage-4 fuse sum + 1x1 head + per-tile argmax partials
        const Tensor& s = net->tensors[op.src0];
        const int nblk = bb_chain_tiles_per_img(s.h, s.w);
        TTUP_REQUIRE(net->refine_ws && net->refine_ws_bytes >= (size_t)mb * nblk * 12, TTUP_EINVAL, "head: workspace too small");
        const PackedConv* cv[4]; BBSum sum;
        chain_args(net, op, cv, &sum);
        sum.heat = heat; sum.head_w = net->head_w_dev; sum.head_bias = net->head_bias;
        sum.pi = (long long*)net->refine_ws; sum.pv = (float*)(sum.pi + (size_t)mb * nblk);
        int rc = launch_bb_chain(cv, 4, s.ptr, nullptr, mb, s.h, s.w, nullptr, nullptr, st, &sum);
        if (rc) return rc;
        if (am || wn) {
            TTUP_REQUIRE(am && wn, TTUP_EINVAL, "head: argmax and window outputs come together");
            rc = launch_argmax_finish(heat, mb, s.h, s.w, nblk, sum.pv, sum.pi, am, wn, st);
        }
        return rc;
    }
    const void* terms[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < op.n_terms; ++k) terms[k] = net->tensors[op.terms[k]].ptr;
    return launch_upsum_head(net->tensors[op.src0].ptr, terms, op.shifts, op.n_terms, net->head_w_dev, net->head_bias, heat, mb, net->H, net->W,
                             am, wn, net->refine_ws, net->refine_ws_bytes, st);
}

int forward_micro(ttup_wasb* net, const float* x_dev, const uint8_t* frames_dev, int n_frames, int src_h, int src_w, int batch, int b0,
                  float* heat_dev, int64_t* argmax_dev, float* win_dev, int lane, hipStream_t st) {
    const int H = net->H, W = net->W;
    const size_t hw = (size_t)H * W;
    const int K = net->n_out;
    const int mb = batch - b0 < net->micro ? batch - b0 : net->micro;
    net->use_lane(lane);
    int rc;
    const int nf = net->in_ch / 3;
    net->frames_mode = !x_dev && net->t_frames >= 0;
    if (x_dev) rc = launch_nchw_to_nhwc(x_dev + (size_t)b0 * net->in_ch * hw, net->tensors[net->t_input].ptr, mb, net->in_ch, 16, H, W, net->dtype, st);
    else if (net->frames_mode)      // every frame of the micro-batch (mb + nf - 1 of them) is pre-processed once; the stem assembles the samples
        rc = launch_preprocess(frames_dev, n_frames, src_h, src_w, H, W, net->tensors[net->t_frames].ptr, TTUP_LAYOUT_NHWC4_FRAME, net->dtype, b0, mb + nf - 1, 1, st);
    else rc = launch_preprocess(frames_dev, n_frames, src_h, src_w, H, W, net->tensors[net->t_input].ptr, TTUP_LAYOUT_NHWC16, net->dtype, b0, mb, nf, st);
    if (rc) return rc;
    rc = run_graph(net, mb, st);
    if (rc) return rc;
    float* heat = heat_dev ? heat_dev + (size_t)b0 * K * hw : net->heat_scratch;
    if (net->fused_head) {
        const bool peaks = argmax_dev || win_dev;
        long long* am = peaks ? (argmax_dev ? (long long*)argmax_dev + b0 : net->argmax_scratch) : nullptr;
        float* wn = peaks ? (win_dev ? win_dev + (size_t)b0 * 9 : net->win_scratch) : nullptr;
        rc = run_head_op(net, mb, heat, am, wn, st);
        if (rc) return rc;
        // certified argmax: pixels within 2*eps of this bf16 maximum are the only ones that can be the fp32 argmax
        if (net->cert.enabled && argmax_dev && win_dev) return cert_scan(net, heat, am, b0, mb, st);
        return TTUP_OK;
    }
    rc = launch_head(net->tensors[net->t_out].ptr, net->head_w_dev, net->head_b_dev, K, heat, mb, H, W, 16, net->dtype, st, net->n_active);
    if (rc) return rc;
    if (argmax_dev || win_dev) {
        long long* am = argmax_dev ? (long long*)argmax_dev + (size_t)b0 * K : net->argmax_scratch;
        float* wn = win_dev ? win_dev + (size_t)b0 * K * 9 : net->win_scratch;
        rc = refine_argmax(heat, mb * K, H, W, am, wn, net->refine_ws, net->refine_ws_bytes, st);
        if (rc) return rc;
        // certified argmax of the multi-channel head (table keypoints): the same scan / plan per heatmap, crops shared by a frame's channels
        if (net->cert.enabled && argmax_dev && win_dev) return cert_scan(net, heat, am, b0, mb, st);
    }
    return TTUP_OK;
}

int forward_impl(ttup_wasb* net, const float* x_dev, const uint8_t* frames_dev, int n_frames, int src_h, int src_w,
                 int batch, float* heat_dev, int64_t* argmax_dev, float* win_dev, hipStream_t st) {
    const int n_micro = (batch + net->micro - 1) / net->micro;
    const int n_lanes = n_micro < (int)net->lanes.size() ? (n_micro > 0 ? n_micro : 1) : (int)net->lanes.size();
    const hipStream_t caller = st;
    const bool certify = net->cert.enabled && argmax_dev && win_dev && batch > 0;
    // Consecutive calls may come in on different caller streams (StreamWorker.submit alternates two) while the activations, the
    // heatmap scratch and the argmax workspace of a lane belong to ONE micro-batch at a time.  Handles with lane streams run every
    // micro-batch on its lane's stream -- also when the call has a single micro-batch -- so stream order serialises the lane's
    // buffers.  Single-lane handles (max_batch <= micro-batch, TTUP_LANES=1) run on the caller's stream: a call then waits for the
    // previous call's last micro-batch, whatever stream that call was issued on.
    const bool lane_streams = net->lanes[0].stream != nullptr;
    if (!lane_streams && net->pass_recorded) TTUP_HIP_CHECK(hipStreamWaitEvent(caller, net->pass_done, 0));
    if (certify) { const int rc = cert_begin(net, batch, caller); if (rc) return rc; }
    if (lane_streams) {
        TTUP_HIP_CHECK(hipEventRecord(net->fork, caller));
        for (int l = 0; l < n_lanes; ++l) TTUP_HIP_CHECK(hipStreamWaitEvent(net->lanes[l].stream, net->fork, 0));
    }
    int rc_all = TTUP_OK, last_lane = 0;
    for (int b0 = 0, i = 0; b0 < batch && rc_all == TTUP_OK; b0 += net->micro, ++i) {
        rc_all = forward_micro(net, x_dev, frames_dev, n_frames, src_h, src_w, batch, b0, heat_dev, argmax_dev, win_dev,
                               i % n_lanes, lane_streams ? net->lanes[i % n_lanes].stream : caller);
        last_lane = i % n_lanes;
    }
    if (lane_streams) {       // join even after an error so the caller's stream never runs ahead of enqueued work
        for (int l = 0; l < n_lanes; ++l) {
            (void)hipEventRecord(net->lanes[l].done, net->lanes[l].stream);
            (void)hipStreamWaitEvent(caller, net->lanes[l].done, 0);
        }
    } else if (hipEventRecord(net->pass_done, caller) == hipSuccess) net->pass_recorded = true;
    net->use_lane(last_lane);
    if (rc_all) return rc_all;
    net->last_batch = batch < net->micro ? batch : net->micro;
    if (certify) return cert_finish(net, x_dev, frames_dev, n_frames, src_h, src_w, batch, argmax_dev, win_dev, caller);
    return TTUP_OK;
}

}  // namespace

namespace ttup {
int run_ops(ttup_wasb* net, int mb, hipStream_t st) { return run_graph(net, mb, st); }

// Cone pruning of a layer-by-layer fp32 graph: walk the ops backwards from the heatmap region [lo, hi) x [lo, hi) and record, for
// every tensor, the union of what its consumers read.  A 3x3 conv reads one pixel around its outputs (times the stride), a fuse sum
// reads the same pixels of its base and pixel >> shift of every upsampled term.  The recorded regions are SUPERSETS by construction
// (kernels round them out to whole tiles): every value an op reads inside its own region has been produced.
int compute_roi(ttup_wasb* net, int lo, int hi, int lo2, int hi2) {
    TTUP_REQUIRE(net && net->dtype == TTUP_DTYPE_F32 && net->t_out >= 0, TTUP_EINVAL, "compute_roi: an fp32 handle is expected");
    const size_t nt = net->tensors.size();
    struct R { int y0, y1, x0, x1; bool any; };
    // one backward walk from the heatmap region [l, h) x [l, h): out[k] = the region of op k's output in the cone (any == false: none)
    auto walk = [&](int l, int h, std::vector<R>& out) -> int {
        std::vector<R> need(nt, R{0, 0, 0, 0, false});
        auto add = [&](int t, int y0, int y1, int x0, int x1) {
            const Tensor& tn = net->tensors[t];
            y0 = y0 < 0 ? 0 : y0; x0 = x0 < 0 ? 0 : x0; y1 = y1 > tn.h ? tn.h : y1; x1 = x1 > tn.w ? tn.w : x1;
            if (y1 <= y0 || x1 <= x0) return;
            R& r = need[t];
            if (!r.any) r = R{y0, y1, x0, x1, true};
            else { r.y0 = y0 < r.y0 ? y0 : r.y0; r.y1 = y1 > r.y1 ? y1 : r.y1; r.x0 = x0 < r.x0 ? x0 : r.x0; r.x1 = x1 > r.x1 ? x1 : r.x1; }
        };
        add(net->t_out, l, h, l, h);
        out.assign(net->ops.size(), R{0, 1, 0, 1, false});          // nothing in the cone reads the op: one pixel
        for (int k = (int)net->ops.size() - 1; k >= 0; --k) {
            const Op& op = net->ops[k];
            TTUP_REQUIRE(op.kind == Op::CONV || op.kind == Op::UPSUM, TTUP_EINVAL, "compute_roi: fused op in an fp32 graph");
            TTUP_REQUIRE(op.conv2 < 0 && op.lin16 < 0 && op.lin32 < 0 && op.pair < 0 && op.res2 < 0 && op.res3 < 0, TTUP_EINVAL, "compute_roi: fused epilogue in an fp32 graph");
            const R d = need[op.dst];
            if (!d.any) continue;
            out[k] = d;
            if (op.kind == Op::CONV) {
                const PackedConv& p = net->convs[op.conv];
                const int s_ = p.stride, pad = p.k / 2;
                add(op.src0, d.y0 * s_ - pad, (d.y1 - 1) * s_ + pad + 1, d.x0 * s_ - pad, (d.x1 - 1) * s_ + pad + 1);
                if (op.src1 >= 0) add(op.src1, d.y0 * s_ - pad, (d.y1 - 1) * s_ + pad + 1, d.x0 * s_ - pad, (d.x1 - 1) * s_ + pad + 1);
                if (op.residual >= 0) add(op.residual, d.y0, d.y1, d.x0, d.x1);
            } else {
                add(op.src0, d.y0, d.y1, d.x0, d.x1);
                for (int j = 0; j < op.n_terms; ++j) { const int sh = op.shifts[j]; add(op.terms[j], d.y0 >> sh, ((d.y1 - 1) >> sh) + 1, d.x0 >> sh, ((d.x1 - 1) >> sh) + 1); }
            }
        }
        return TTUP_OK;
    };
    std::vector<R> r1, r2;
    if (int rc = walk(lo, hi, r1)) return rc;
    const bool two = hi2 > lo2;
    if (two) { if (int rc = walk(lo2, hi2, r2)) return rc; }
    net->op_roi.assign(net->ops.size(), Roi());
    for (size_t k = 0; k < net->ops.size(); ++k) {
        Roi& o = net->op_roi[k];
        o.y0 = r1[k].y0; o.y1 = r1[k].y1; o.x0 = r1[k].x0; o.x1 = r1[k].x1;
        if (two) { o.sy0 = r2[k].y0; o.sy1 = r2[k].y1; o.sx0 = r2[k].x0; o.sx1 = r2[k].x1; }
    }
    if (env_set("TTUP_DEBUG_ROI")) {
        double full = 0, kept = 0, kept2 = 0;
        for (size_t k = 0; k < net->ops.size(); ++k) {
            const Op& op = net->ops[k];
            const Tensor& d = net->tensors[op.dst];
            const Roi& o = net->op_roi[k];
            double w = (double)d.h * d.w;
            if (op.kind == Op::CONV) { const PackedConv& p = net->convs[op.conv]; w *= (double)p.cout * p.cin_total * p.k * p.k; } else w *= d.c;
            full += w; kept += w * ((double)(o.y1 - o.y0) * (o.x1 - o.x0)) / ((double)d.h * d.w);
            kept2 += w * ((double)(o.sy1 - o.sy0) * (o.sx1 - o.sx0)) / ((double)d.h * d.w);
            fprintf(stderr, "roi op %2zu %s dst %3dx%3dx%3d -> [%d,%d)x[%d,%d)  class 2 [%d,%d)x[%d,%d)\n", k, op.kind == Op::CONV ? "conv " : "upsum", d.h, d.w, d.c, o.y0, o.y1, o.x0, o.x1,
                    o.sy0, o.sy1, o.sx0, o.sx1);
        }
        fprintf(stderr, "roi: %.1f %% of the graph's multiply-adds kept (class 2: %.1f %%)\n", 100.0 * kept / full, 100.0 * kept2 / full);
    }
    net->out_roi = Roi();
    net->out_roi.y0 = lo; net->out_roi.y1 = hi; net->out_roi.x0 = lo; net->out_roi.x1 = hi;
    if (two) { net->out_roi.sy0 = lo2; net->out_roi.sy1 = hi2; net->out_roi.sx0 = lo2; net->out_roi.sx1 = hi2; }
    return TTUP_OK;
}
}

// micro_override / lanes_override > 0 fix the micro-batch and the lane count (the certified argmax's fp32 crop net runs its
// whole batch as one micro-batch on one lane); 0 = TTUP_MICRO_BATCH / TTUP_LANES or the defaults
int ttup_wasb_create_internal(const void* blob, size_t blob_bytes, int height, int width, int max_batch, int dtype, int micro_override, int lanes_override, ttup_wasb** out) {
    TTUP_REQUIRE(blob && out, TTUP_EINVAL, "ttup_wasb_create: null pointer");
    TTUP_REQUIRE(height > 0 && width > 0 && height % 8 == 0 && width % 8 == 0, TTUP_EINVAL,
                 "ttup_wasb_create: input size %dx%d must be positive multiples of 8", height, width);
    TTUP_REQUIRE(max_batch > 0, TTUP_EINVAL, "ttup_wasb_create: max_batch must be positive");
    TTUP_REQUIRE(dtype == TTUP_DTYPE_BF16 || dtype == TTUP_DTYPE_F32, TTUP_EINVAL, "ttup_wasb_create: unknown dtype %d", dtype);
    std::vector<FoldedConv> folded;
    std::vector<float> head_w, head_b;
    int in_ch = 0, head_out = 0;
    int rc = parse_blob(blob, blob_bytes, &folded, &in_ch, &head_out, &head_w, &head_b);
    if (rc) return rc;
    TTUP_REQUIRE((in_ch == 9 || in_ch == 3) && head_out >= 1 && head_out <= 16, TTUP_EFORMAT, "wasb blob: in_ch=%d head_out=%d unsupported (ball detector 9/3, table detector 3/13)", in_ch, head_out);
    int ndev = 0;
    TTUP_HIP_CHECK(hipGetDeviceCount(&ndev));
    TTUP_REQUIRE(ndev > 0, TTUP_EHIP, "ttup_wasb_create: no HIP device");
    std::unique_ptr<ttup_wasb> net(new ttup_wasb);
    net->H = height; net->W = width; net->max_batch = max_batch; net->dtype = dtype; net->in_ch = in_ch;
    net->blob.assign((const char*)blob, (const char*)blob + blob_bytes);
    net->n_out = head_out == 3 ? 1 : head_out;       // ball detector keeps the middle of its 3 channels (wasb.py:606)
    // micro-batch: enough tiles to fill 256 CUs, small enough that layer outputs stay cache-friendly
    int micro = micro_override > 0 ? micro_override : (int)env_ll("TTUP_MICRO_BATCH", 8);
    if (micro < 1) micro = 1;
    net->micro = micro < max_batch ? micro : max_batch;
    GraphSwitches sw;          // sampled here, once per net
    sw.fuse = !env_set("TTUP_NO_FUSE"); sw.fuse_sum = !env_set("TTUP_NO_FUSE_SUM"); sw.fuse_lin = !env_set("TTUP_NO_FUSE_LIN");
    sw.pair = !env_set("TTUP_NO_PAIR"); sw.stem = !env_set("TTUP_NO_STEM"); sw.frames_mode = !env_set("TTUP_NO_FRAMES_MODE");
    const GraphPlan plan = build_graph(folded, in_ch, net->n_out, height, width, net->micro, dtype, sw);
    if (plan.rc) return plan.rc;
    net->ops = plan.ops; net->taps = plan.taps;
    net->t_input = plan.t_input; net->t_out = plan.t_out; net->t_frames = plan.t_frames; net->fused_head = plan.fused_head;
    for (const TensorShape& s : plan.tensors) { Tensor t; static_cast<TensorShape&>(t) = s; net->tensors.push_back(t); }
    for (const ConvRequest& r : plan.convs) {
        net->convs.emplace_back();          // in the list before it is filled: the destructor frees a partly packed conv as well
        PackedConv& p = net->convs.back();
        rc = pack_conv(plan.source_a(r, folded), r.b >= 0 ? &folded[r.b] : nullptr, r.cin_pad, dtype, &p);
        if (rc) return rc;
        TTUP_REQUIRE(p.cout == r.cout && p.cin_total == r.cin_total && p.c0 == r.c0 && p.k == r.k && p.stride == r.stride, TTUP_EINVAL,
                     "wasb: conv %zu was packed as %d x %d+%d, k %d / s%d; the plan has %d x %d+%d, k %d / s%d", net->convs.size() - 1,
                     p.cout, p.c0, p.cin_total - p.c0, p.k, p.stride, r.cout, r.c0, r.cin_total - r.c0, r.k, r.stride);
    }
    // head weights of the returned channels: the ball detector keeps only channel 1 of its 3 (wasb.py:606), the table
    // detector all 13 (tabledetection/models/hrnet.py:586-589)
    {
        const int first = head_out == 3 ? 1 : 0;
        TTUP_HIP_CHECK(hipMalloc((void**)&net->head_w_dev, (size_t)net->n_out * 16 * sizeof(float)));
        TTUP_HIP_CHECK(hipMemcpy(net->head_w_dev, head_w.data() + (size_t)first * 16, (size_t)net->n_out * 16 * sizeof(float), hipMemcpyHostToDevice));
        TTUP_HIP_CHECK(hipMalloc((void**)&net->head_b_dev, (size_t)net->n_out * sizeof(float)));
        TTUP_HIP_CHECK(hipMemcpy(net->head_b_dev, head_b.data() + first, (size_t)net->n_out * sizeof(float), hipMemcpyHostToDevice));
        net->head_bias = head_b[first];
    }
    const size_t hw = (size_t)height * width;
    net->refine_ws_bytes = ttup_refine_workspace_bytes(net->micro * net->n_out, height, width);
    if (upsum_head_ws_bytes(net->micro, height, width) > net->refine_ws_bytes) net->refine_ws_bytes = upsum_head_ws_bytes(net->micro, height, width);
    {
        int n_lanes = lanes_override > 0 ? lanes_override : (int)env_ll("TTUP_LANES", 2);
        const int n_micro = (max_batch + net->micro - 1) / net->micro;
        if (n_lanes > n_micro) n_lanes = n_micro;
        if (n_lanes < 1) n_lanes = 1;
        if (n_lanes > 4) n_lanes = 4;
        net->lanes.resize(n_lanes);
        for (int l = 0; l < n_lanes; ++l) {
            ttup_wasb::Lane& L = net->lanes[l];
            L.ptr.assign(net->tensors.size(), nullptr);
            for (size_t i = 0; i < net->tensors.size(); ++i) {
                const size_t bytes = plan.tensor_bytes(i);
                if (hipMalloc(&L.ptr[i], bytes) != hipSuccess) { L.ptr[i] = nullptr; set_error("hipMalloc of %zu bytes failed", bytes); return TTUP_ENOMEM; }
            }
            TTUP_HIP_CHECK(hipMalloc((void**)&L.heat_scratch, (size_t)net->micro * net->n_out * hw * sizeof(float)));
            TTUP_HIP_CHECK(hipMalloc(&L.refine_ws, net->refine_ws_bytes));
            TTUP_HIP_CHECK(hipMalloc((void**)&L.argmax_scratch, (size_t)net->micro * net->n_out * sizeof(long long)));
            TTUP_HIP_CHECK(hipMalloc((void**)&L.win_scratch, (size_t)net->micro * net->n_out * 9 * sizeof(float)));
            if (n_lanes > 1) {
                TTUP_HIP_CHECK(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
                TTUP_HIP_CHECK(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
            }
        }
        if (n_lanes > 1) TTUP_HIP_CHECK(hipEventCreateWithFlags(&net->fork, hipEventDisableTiming));
        TTUP_HIP_CHECK(hipEventCreateWithFlags(&net->pass_done, hipEventDisableTiming));
        net->use_lane(0);
    }
    // measurement aid (tools/ops_report_f32.py): TTUP_DEBUG_FORCE_ROI=1 prunes EVERY sample of an fp32 handle to the cone of its central
    // 24-pixel core, as the certified argmax's crop net does for interior crops -- per-op timings of the pruned graph (the flags leak
    // with the process: a debugging switch)
    if (dtype == TTUP_DTYPE_F32 && env_set("TTUP_DEBUG_FORCE_ROI") && net->H == net->W && net->H >= 2 * 72 + 24) {
        int* flags = nullptr;
        TTUP_HIP_CHECK(hipMalloc((void**)&flags, (size_t)max_batch * sizeof(int)));
        std::vector<int> ones((size_t)max_batch, env_ll("TTUP_DEBUG_FORCE_ROI", 0) == 2 ? 2 : 1);          // = 2: the class-2 regions (16-pixel core)
        TTUP_HIP_CHECK(hipMemcpy(flags, ones.data(), ones.size() * sizeof(int), hipMemcpyHostToDevice));
        if (int rc = compute_roi(net.get(), 72, net->H - 72, 72, 88)) return rc;
        net->roi_flag = flags;
    }
    TTUP_HIP_CHECK(hipDeviceSynchronize());
    *out = net.release();
    return TTUP_OK;
}

extern "C" int ttup_wasb_create(const void* blob, size_t blob_bytes, int height, int width, int max_batch, int dtype, ttup_wasb** out) {
    return ttup_wasb_create_internal(blob, blob_bytes, height, width, max_batch, dtype, 0, 0, out);
}

// micro_batch / lanes: 0 = the defaults (8 frames, two lanes; TTUP_MICRO_BATCH / TTUP_LANES); lanes = 1 runs every micro-batch on
// the caller's stream -- for a handle that shares the device with another busy handle (the hub pipeline's two detectors), where a
// second lane only adds streams that collide on the runtime's few hardware queues
extern "C" int ttup_wasb_create_ex(const void* blob, size_t blob_bytes, int height, int width, int max_batch, int dtype, int micro_batch, int lanes,
                                   ttup_wasb** out) {
    TTUP_REQUIRE(micro_batch >= 0 && lanes >= 0 && lanes <= 4, TTUP_EINVAL, "ttup_wasb_create_ex: micro_batch %d / lanes %d out of range", micro_batch, lanes);
    return ttup_wasb_create_internal(blob, blob_bytes, height, width, max_batch, dtype, micro_batch, lanes, out);
}

// The handle's internal streams: its lane streams (none for a single-lane handle), then the stream of the certified argmax's fp32
// passes (when enabled).  For callers that want to know which streams share a hardware queue (tools/queue_probe.py).
extern "C" int ttup_wasb_streams(ttup_wasb* net, void** out, int cap, int* n_out) {
    TTUP_REQUIRE(net && out && n_out && cap >= 0, TTUP_EINVAL, "ttup_wasb_streams: bad argument");
    int n = 0;
    for (auto& L : net->lanes) if (L.stream && n < cap) out[n++] = (void*)L.stream;
    if (net->cert.enabled && net->cert.stream && n < cap) out[n++] = (void*)net->cert.stream;
    *n_out = n;
    return TTUP_OK;
}

extern "C" void ttup_wasb_destroy(ttup_wasb* net) {
    if (!net) return;
    (void)hipDeviceSynchronize();
    delete net;
}

extern "C" int ttup_wasb_forward(ttup_wasb* net, const float* x_dev, int batch, float* heat_dev, int64_t* argmax_dev, float* win_dev, void* stream) {
    TTUP_REQUIRE(net && x_dev, TTUP_EINVAL, "ttup_wasb_forward: null pointer");
    TTUP_REQUIRE(batch >= 0 && batch <= net->max_batch, TTUP_EINVAL, "ttup_wasb_forward: batch %d outside [0,%d]", batch, net->max_batch);
    return forward_impl(net, x_dev, nullptr, 0, 0, 0, batch, heat_dev, argmax_dev, win_dev, (hipStream_t)stream);
}

extern "C" int ttup_wasb_forward_frames(ttup_wasb* net, const uint8_t* frames_dev, int n_frames, int src_h, int src_w,
                                        float* heat_dev, int64_t* argmax_dev, float* win_dev, void* stream) {
    TTUP_REQUIRE(net && frames_dev, TTUP_EINVAL, "ttup_wasb_forward_frames: null pointer");
    const int nf = net->in_ch / 3;       // 3 frames per sample for the ball detector, 1 for the table detector
    TTUP_REQUIRE(n_frames >= nf && src_h > 0 && src_w > 0, TTUP_EINVAL, "ttup_wasb_forward_frames: need at least %d frames", nf);
    const int batch = n_frames - (nf - 1);
    TTUP_REQUIRE(batch <= net->max_batch, TTUP_EINVAL, "ttup_wasb_forward_frames: %d triples exceed max_batch %d", batch, net->max_batch);
    return forward_impl(net, nullptr, frames_dev, n_frames, src_h, src_w, batch, heat_dev, argmax_dev, win_dev, (hipStream_t)stream);
}

extern "C" int ttup_wasb_read_tap(ttup_wasb* net, const char* name, int batch, float* out_dev, int* c, int* h, int* w, void* stream) {
    TTUP_REQUIRE(net && name, TTUP_EINVAL, "ttup_wasb_read_tap: null pointer");
    auto it = net->taps.find(name);
    TTUP_REQUIRE(it != net->taps.end(), TTUP_EINVAL, "ttup_wasb_read_tap: unknown tap '%s'", name);
    const Tensor& t = net->tensors[it->second];
    if (c) *c = t.c; if (h) *h = t.h; if (w) *w = t.w;
    if (!out_dev) return TTUP_OK;
    TTUP_REQUIRE(batch > 0 && batch <= net->micro, TTUP_EINVAL, "ttup_wasb_read_tap: batch %d exceeds the micro-batch %d held in memory", batch, net->micro);
    return launch_nhwc_to_nchw(t.ptr, out_dev, batch, t.c, t.h, t.w, net->dtype, (hipStream_t)stream);
}

#include "wasb_timing.h"

extern "C" int ttup_preprocess_triples(const uint8_t* frames_dev, int n_frames, int src_h, int src_w, int dst_h, int dst_w,
                                       float* out_dev, void* stream) {
    TTUP_REQUIRE(frames_dev && out_dev, TTUP_EINVAL, "ttup_preprocess_triples: null pointer");
    TTUP_REQUIRE(n_frames >= 3 && src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0, TTUP_EINVAL, "ttup_preprocess_triples: bad shape");
    return launch_preprocess(frames_dev, n_frames, src_h, src_w, dst_h, dst_w, out_dev, TTUP_LAYOUT_NCHW_F32, TTUP_DTYPE_F32, 0, n_frames - 2, 3, (hipStream_t)stream);
}

extern "C" int ttup_preprocess_frames(const uint8_t* frames_dev, int n_frames, int src_h, int src_w, int dst_h, int dst_w,
                                      float* out_dev, void* stream) {
    TTUP_REQUIRE(frames_dev && out_dev, TTUP_EINVAL, "ttup_preprocess_frames: null pointer");
    TTUP_REQUIRE(n_frames >= 1 && src_h > 0 && src_w > 0 && dst_h > 0 && dst_w > 0, TTUP_EINVAL, "ttup_preprocess_frames: bad shape");
    return launch_preprocess(frames_dev, n_frames, src_h, src_w, dst_h, dst_w, out_dev, TTUP_LAYOUT_NCHW_F32, TTUP_DTYPE_F32, 0, n_frames, 1, (hipStream_t)stream);
}

// Scheduling priority of the handle's internal lane streams (high != 0: the greatest priority of the device).  Two handles that
// share the GPU (the hub path runs the table and the ball detector side by side) can thus be ordered: the high-priority one
// finishes first and its host-side consumer overlaps with the other's kernels.  Synchronises; single-lane handles run on the
// caller's stream and are not affected.
extern "C" int ttup_wasb_set_priority(ttup_wasb* net, int high) {
    TTUP_REQUIRE(net, TTUP_EINVAL, "ttup_wasb_set_priority: null handle");
    if (net->lanes.size() < 2) return TTUP_OK;
    TTUP_HIP_CHECK(hipDeviceSynchronize());
    int least = 0, greatest = 0;
    TTUP_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    for (auto& L : net->lanes) {
        if (L.stream) (void)hipStreamDestroy(L.stream);
        L.stream = nullptr;
        TTUP_HIP_CHECK(hipStreamCreateWithPriority(&L.stream, hipStreamNonBlocking, high ? greatest : least));
    }
    return TTUP_OK;
}

extern "C" int ttup_wasb_micro_batch(ttup_wasb* net) { return net ? net->micro : 0; }
extern "C" int ttup_wasb_out_channels(ttup_wasb* net) { return net ? net->n_out : 0; }
