// Measurement aids for bench.py and tools/ops_report.py: what each op of a handle launches (op_info) and the three
// ttup_wasb_time_* entry points.  Private to csrc/wasb_net.hip, which includes it after run_op / run_head_op.
#pragma once
// info: 8 ints per op {kind(0 conv,1 upsum,2 bneck_trans,3 bb_chain,4 stem,5 upsum_head), algorithmic MACs per output element
// (or cin), cout, k, stride, out_h, out_w, cin_padded / chain length}; name: the HIP kernel the op launches.
namespace {
void op_info(const ttup_wasb* net, int i, int* o, char* name) {
    const Op& op = net->ops[i];
    const Tensor& d = net->tensors[op.dst >= 0 ? op.dst : op.src0];
    const bool bf = net->dtype == TTUP_DTYPE_BF16;
    char nm[64] = "";
    if (op.kind == Op::STEM) {
        o[0] = 4; o[1] = 9 * 9 * 64 + 9 * 64 * 64 + 64 * 32; o[2] = 1; o[3] = 1; o[4] = 1; o[5] = d.h; o[6] = d.w; o[7] = 0;
        snprintf(nm, sizeof nm, "stem_kernel");
    } else if (op.kind == Op::BB_CHAIN) {
        o[0] = 3; o[1] = op.n_chain * d.c * 9; o[2] = d.c; o[3] = 1; o[4] = 1; o[5] = d.h; o[6] = d.w; o[7] = op.n_chain;
        if (op.n_chain == 4) snprintf(nm, sizeof nm, "bb_chain2_kernel<16>%s", op.head ? "+sum+head" : op.n_terms > 0 ? "+sum" : "");
        else snprintf(nm, sizeof nm, "bb_chain_kernel<%d,1>%s", d.c, op.conv2 >= 0 ? "+1x1" : "");
        if (op.conv2 >= 0) o[1] += 16;          // fused 1x1 32->16 follower: 32*16 MACs per pixel = 16 per output element of the block
    } else if (op.kind == Op::BNECK_TRANS) {
        // algorithmic MACs per output pixel of B0: 96*128 (1x1) + 1152*16 (3x3 s1) + 1152*32/4 (3x3 s2 at quarter density)
        o[0] = 2; o[1] = 96 * 128 + 1152 * 16 + 1152 * 8; o[2] = 1; o[3] = 1; o[4] = 1; o[5] = d.h; o[6] = d.w; o[7] = 0;
        snprintf(nm, sizeof nm, "bneck_trans_kernel");
    } else if (op.kind == Op::CONV) {
        const PackedConv& pc = net->convs[op.conv];
        o[0] = 0; o[1] = (i == 0) ? net->in_ch : pc.cin_total; o[2] = pc.cout; o[3] = pc.k; o[4] = pc.stride; o[5] = d.h; o[6] = d.w; o[7] = pc.cin_total;
        if (!bf) snprintf(nm, sizeof nm, "conv_direct_f32_kernel");
        else if (pc.k == 3 && pc.stride == 1 && pc.cout == 64 && pc.cin_total == 64 && op.conv2 < 0) snprintf(nm, sizeof nm, "conv64_kernel%s", (op.lin16 >= 0 || op.lin32 >= 0) ? "+1x1" : "");
        else if (op.pair >= 0) { snprintf(nm, sizeof nm, "conv_s2_pair_kernel"); o[2] = pc.cout + net->convs[op.pair].cout; }      // both convs' outputs count
        else snprintf(nm, sizeof nm, "conv_mfma_kernel<%d,%d,%d,%d>", pc.ck, pc.cout, pc.k, pc.stride);
    } else {
        o[0] = op.kind == Op::UPSUM_HEAD ? 5 : 1; o[1] = op.n_terms; o[2] = d.c; o[3] = 0; o[4] = 0; o[5] = d.h; o[6] = d.w; o[7] = d.c;
        snprintf(nm, sizeof nm, op.kind == Op::UPSUM_HEAD ? "upsum_head_kernel" : bf ? "upsum_bf16x8_kernel" : "upsum_kernel<float>");
    }
    if (name) { memset(name, 0, 64); memcpy(name, nm, strlen(nm)); }
}
// one op as the forward pass launches it; the fused last op of the bf16 ball path writes to the lane's scratch outputs
int run_any_op(ttup_wasb* net, const Op& op, int batch, hipStream_t st) {
    if (op.kind == Op::UPSUM_HEAD || op.head) return run_head_op(net, batch, net->heat_scratch, net->argmax_scratch, net->win_scratch, st);
    return run_op(net, op, batch, st);
}
}  // namespace

// Every op on its own: `reps` back-to-back launches of one op between two HIP events on `stream` (inputs warm in the caches).
extern "C" int ttup_wasb_time_ops(ttup_wasb* net, int batch, int reps, int max_ops, float* ms_out, int* info_out, int* n_ops_out, void* stream) {
    TTUP_REQUIRE(net && ms_out && info_out && n_ops_out, TTUP_EINVAL, "ttup_wasb_time_ops: null pointer");
    TTUP_REQUIRE(batch > 0 && batch <= net->micro && reps > 0, TTUP_EINVAL, "ttup_wasb_time_ops: batch must be in [1,%d]", net->micro);
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)net->ops.size();
    TTUP_REQUIRE(n <= max_ops, TTUP_EINVAL, "ttup_wasb_time_ops: %d ops exceed max_ops %d", n, max_ops);
    hipEvent_t e0, e1;
    TTUP_HIP_CHECK(hipEventCreate(&e0));
    TTUP_HIP_CHECK(hipEventCreate(&e1));
    int rc = TTUP_OK;
    net->use_lane(0);
    for (int i = 0; i < n && rc == TTUP_OK; ++i) {
        const Op& op = net->ops[i];
        auto once = [&]() { return run_any_op(net, op, batch, st); };
        rc = once();                       // warm-up launch of this op
        if (rc == TTUP_OK) {
            (void)hipEventRecord(e0, st);
            for (int r = 0; r < reps && rc == TTUP_OK; ++r) rc = once();
            (void)hipEventRecord(e1, st);
            (void)hipEventSynchronize(e1);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e0, e1);
            ms_out[i] = ms / reps;
        }
        op_info(net, i, info_out + 8 * i, nullptr);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *n_ops_out = n;
    return rc;
}

// The whole graph in order, as the forward pass launches it (one micro-batch on lane 0, `stream`), with a HIP event between
// consecutive ops: ms_out[i] = average time from the end of op i-1 to the end of op i over `reps` passes, i.e. the launch
// duration of op i with the cache state it really sees.  This is what bench.py's `roofline` is computed from and what the
// rocprofv3 kernel trace of the same run (TTUP_LANES=1) reports per kernel.  names_out: max_ops x 64 chars.
extern "C" int ttup_wasb_time_graph(ttup_wasb* net, int batch, int reps, int max_ops, float* ms_out, int* info_out, char* names_out,
                                    int* n_ops_out, void* stream) {
    TTUP_REQUIRE(net && ms_out && info_out && n_ops_out, TTUP_EINVAL, "ttup_wasb_time_graph: null pointer");
    TTUP_REQUIRE(batch > 0 && batch <= net->micro && reps > 0, TTUP_EINVAL, "ttup_wasb_time_graph: batch must be in [1,%d]", net->micro);
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)net->ops.size();
    TTUP_REQUIRE(n <= max_ops, TTUP_EINVAL, "ttup_wasb_time_graph: %d ops exceed max_ops %d", n, max_ops);
    std::vector<hipEvent_t> ev(n + 1);
    for (auto& e : ev) TTUP_HIP_CHECK(hipEventCreate(&e));
    std::vector<double> acc(n, 0.0);
    std::vector<std::string> exact(n);          // the device kernel each op launched (kernel_note of its launcher), as rocprofv3 names it
    int rc = TTUP_OK;
    net->use_lane(0);
    for (int r = -1; r < reps && rc == TTUP_OK; ++r) {          // pass -1 = warm-up
        (void)hipEventRecord(ev[0], st);
        for (int i = 0; i < n && rc == TTUP_OK; ++i) {
            const Op& op = net->ops[i];
            kernel_note_reset();
            rc = run_any_op(net, op, batch, st);
            (void)hipEventRecord(ev[i + 1], st);
            if (r < 0) exact[i] = kernel_noted();
        }
        (void)hipEventSynchronize(ev[n]);
        if (r >= 0) for (int i = 0; i < n; ++i) { float ms = 0.f; (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]); acc[i] += ms; }
    }
    for (int i = 0; i < n; ++i) {
        ms_out[i] = (float)(acc[i] / reps);
        char nm[64];
        op_info(net, i, info_out + 8 * i, nm);
        if (names_out) {
            // "<device kernel template-id><+epilogue variant>": the op-level label keeps only its '+...' suffix when the launcher left a note
            std::string full = exact[i].empty() ? std::string(nm) : exact[i] + (strchr(nm, '+') ? strchr(nm, '+') : "");
            memset(names_out + 64 * i, 0, 64);
            memcpy(names_out + 64 * i, full.c_str(), full.size() < 63 ? full.size() : 63);
        }
    }
    for (auto& e : ev) (void)hipEventDestroy(e);
    *n_ops_out = n;
    return rc;
}

// The same launches back to back, `reps` passes between ONE pair of events (no event between the ops: an event record between two
// kernels is a packet of its own on the queue, and the per-op intervals of ttup_wasb_time_graph each include one).  ms_out[0] = the
// average duration of a pass: what one lane of the pipeline spends on a micro-batch.
extern "C" int ttup_wasb_time_replay(ttup_wasb* net, int batch, int reps, float* ms_out, void* stream) {
    TTUP_REQUIRE(net && ms_out, TTUP_EINVAL, "ttup_wasb_time_replay: null pointer");
    TTUP_REQUIRE(batch > 0 && batch <= net->micro && reps > 0, TTUP_EINVAL, "ttup_wasb_time_replay: batch must be in [1,%d]", net->micro);
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e0, e1;
    TTUP_HIP_CHECK(hipEventCreate(&e0));
    TTUP_HIP_CHECK(hipEventCreate(&e1));
    int rc = TTUP_OK;
    net->use_lane(0);
    for (int r = -1; r < reps && rc == TTUP_OK; ++r) {          // pass -1 = warm-up
        if (r == 0) (void)hipEventRecord(e0, st);
        for (const Op& op : net->ops) {
            rc = run_any_op(net, op, batch, st);
            if (rc != TTUP_OK) break;
        }
    }
    (void)hipEventRecord(e1, st);
    (void)hipEventSynchronize(e1);
    float ms = 0.f;
    if (rc == TTUP_OK) { (void)hipEventElapsedTime(&ms, e0, e1); ms_out[0] = ms / reps; }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    return rc;
}
