// The WASB / HRNet CNN as a device-free plan: which op runs where, on tensors of which shapes, with which packed convs.
// Standard library and include/ttup.h only -- this header compiles with a plain host compiler, and tests/helpers/host_wasb_graph.cpp
// runs every switch combination of it on the CPU.  csrc/wasb_net.hip turns a plan into a handle (pack_conv per conv request, one
// allocation per lane and tensor).
// Graph follows balldetection/models/wasb.py: HRNet.forward :445-486, HighResolutionModule.forward :227-245,
// fuse construction :179-222, transitions :362-396, config :514-573, WASBNet.forward :596-608.
//
// What is different from the reference's eager module tree (results unchanged):
//   * BatchNorm (eval) is folded into every conv at create time (csrc/wasb_blob.h);
//   * Bottleneck conv3 (1x1 32->128) and its 1x1 downsample (64->128) + add + ReLU run as ONE two-source
//     1x1 conv with K = 32+64 (the 128-channel pre-activation never touches HBM);
//   * stage-4 fused outputs 1..3 (only consumed when classify_invisible=True, never set by get_model,
//     balldetection/train.py:268) and head channels 0 and 2 (dropped at wasb.py:606) are not computed;
//   * the batch is processed in micro-batches so that intermediate tensors stay near the Infinity Cache.
#pragma once
#include "../../include/ttup.h"
#include <stddef.h>
#include <map>
#include <string>
#include <vector>

namespace ttup {

void set_error(const char* fmt, ...);   // thread-local, returned by ttup_last_error() (api.hip; a host program brings its own)

#ifndef TTUP_REQUIRE          // csrc/common.h has the same text
#define TTUP_REQUIRE(cond, code, ...)                                                         \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            ttup::set_error(__VA_ARGS__);                                                     \
            return code;                                                                      \
        }                                                                                     \
    } while (0)
#endif

// One convolution with eval-mode BatchNorm folded in (scale into the weights, shift into the bias).
struct FoldedConv {
    int cout = 0, cin = 0, k = 1, stride = 1;
    std::vector<float> w;      // [cout][cin][k][k]
    std::vector<float> bias;   // [cout]
};

struct TensorShape { int c = 0, h = 0, w = 0; int extra = 0; };     // (micro + extra, h, w, c)

struct Op {
    enum Kind { CONV, UPSUM, BNECK_TRANS, BB_CHAIN, UPSUM_HEAD, STEM } kind = CONV;
    int chain[4] = {-1, -1, -1, -1}, n_chain = 0;          // BB_CHAIN: packed conv indices
    int conv = -1;            // index into packed convs
    int conv2 = -1, conv3 = -1, dst2 = -1;     // BNECK_TRANS: transition convs and second output; CONV: fused 1x1 follower (conv2) -> dst2
    int src0 = -1, src1 = -1, residual = -1, dst = -1;
    int relu = 0;
    int terms[3] = {-1, -1, -1}, shifts[3] = {0, 0, 0}, n_terms = 0;   // UPSUM
    int res2 = -1, res3 = -1, sh3 = 0;          // CONV (bf16, stride 2): fuse-layer terms folded into the epilogue
    // BB_CHAIN (16 channels, 4 convs) with the consuming fuse-layer sum in its epilogue: terms/shifts/n_terms as for UPSUM,
    // dst2 = the summed output; head = 1: stage-4 output, never stored -- the 1x1 head + argmax partials are computed from it
    // (launched by run_head_op, which knows the output buffers); dst = -1 when the pre-fuse branch tensor has no consumer
    int head = 0;
    int conv1f = -1;                            // STEM: conv1 packed for the frames mode (channel slot f*4 + c)
    // CONV (64 -> 64 3x3, bf16): fuse-layer 1x1 convs on its output riding in its epilogue (packed conv index, output tensor)
    int lin16 = -1, lin16_dst = -1, lin32 = -1, lin32_dst = -1;
    // CONV (3x3 s2 16 -> 32, bf16): a second 3x3 s2 16 -> 16 conv on the same input in the same pass (packed conv, output, ReLU)
    int pair = -1, pair_dst = -1, pair_relu = 0;
};

// The graph switches (README, "knobs"): every net samples them for itself, all together, when it is created (csrc/wasb_net.hip reads
// the environment) -- the tests set them in-process between two handles.
struct GraphSwitches {
    bool fuse = true;              // any fused kernel at all (bf16 nets)
    bool fuse_sum = true;          // the fuse-layer sum / the head in the 16-channel chain's epilogue
    bool fuse_lin = true;          // the 64 -> 16 / 64 -> 32 fuse convs in conv64's epilogue
    bool pair = true;              // the two stride-2 convs of stage 3's fuse layer in one pass
    bool stem = true;              // the fused stem
    bool frames_mode = true;       // the stem reads per-frame records
};

// One pack_conv call: sources a (and b: the second source of a two-source 1x1 conv, or -1) are indices into the blob's folded convs,
// or -- `synth` -- a is an index into the plan's own re-arranged stem convs.  The shape fields are what pack_conv will report; the
// fusion decisions below read them.
struct ConvRequest {
    int a = -1, b = -1; bool synth = false;
    int cin_pad = 0;
    int cout = 0, cin_total = 0, c0 = 0, k = 1, stride = 1;
};

struct GraphPlan {
    int rc = TTUP_OK;                   // != TTUP_OK: the message is in set_error, the rest of the plan is not to be used
    int micro = 1, dtype = TTUP_DTYPE_BF16;
    std::vector<Op> ops;
    std::vector<TensorShape> tensors;
    std::vector<ConvRequest> convs;
    std::vector<FoldedConv> synth;      // the stem's conv1 re-arranged for the frames mode (see stem())
    std::map<std::string, int> taps;
    int t_input = -1, t_out = -1;
    int t_frames = -1;                  // bf16 stem frames mode: (micro + nf - 1, H, W, 4) per-frame pre-processed records
    bool fused_head = false;            // last op computes the heatmap and the argmax partials itself (bf16 path)
    size_t consumed = 0;                // folded convs read in reference order (all but the head conv)

    size_t tensor_bytes(size_t i) const {
        const TensorShape& t = tensors[i];
        return (size_t)(micro + t.extra) * t.h * t.w * t.c * (dtype == TTUP_DTYPE_F32 ? 4 : 2);
    }
    const FoldedConv& source_a(const ConvRequest& r, const std::vector<FoldedConv>& folded) const { return r.synth ? synth[r.a] : folded[r.a]; }
};

const int STAGE_CH[4] = {16, 32, 64, 128};
const int WASB_CONVS = 72;          // arch.hrnet_convs: 71 of the graph + the head conv

struct GraphBuilder {
    GraphPlan& g;
    const std::vector<FoldedConv>& folded;
    const GraphSwitches sw;
    const int in_ch, n_out, H, W;
    const bool fuse;           // bf16 and not TTUP_NO_FUSE: the fused kernels may be used
    size_t cursor = 0;         // next folded conv in reference order

    int new_tensor(int c, int h, int w, int extra = 0) {
        TensorShape t; t.c = c; t.h = h; t.w = w; t.extra = extra;
        g.tensors.push_back(t);
        return (int)g.tensors.size() - 1;
    }
    int next(int cout, int cin, int k, int stride) {          // index of the next folded conv, which must have this shape
        const FoldedConv& f = folded[cursor++];
        if (f.cout != cout || f.cin != cin || f.k != k || f.stride != stride) {
            set_error("wasb blob: conv %zu is %dx%dx%d/s%d, architecture expects %dx%dx%d/s%d", cursor - 1, f.cout, f.cin, f.k, f.stride, cout, cin, k, stride);
            g.rc = TTUP_EFORMAT;
        }
        return (int)cursor - 1;
    }
    int request(int a, int b, int cin_pad, bool synth = false) {
        ConvRequest r; r.a = a; r.b = b; r.synth = synth; r.cin_pad = cin_pad;
        const FoldedConv& fa = g.source_a(r, folded);
        r.cout = fa.cout; r.k = fa.k; r.stride = fa.stride;
        r.c0 = cin_pad > fa.cin ? cin_pad : fa.cin;
        r.cin_total = r.c0 + (b >= 0 ? folded[b].cin : 0);
        g.convs.push_back(r);
        return (int)g.convs.size() - 1;
    }
    Op* writer_of(int t) {          // the op whose `dst` is tensor t
        for (size_t k = g.ops.size(); k-- > 0;) if (g.ops[k].dst == t) return &g.ops[k];
        return nullptr;
    }
    // conv op on tensor `src` -> new tensor
    int conv(int src, int cout, int k, int stride, int relu, int residual = -1) {
        const TensorShape s = g.tensors[src];
        const int pc = request(next(cout, s.c, k, stride), -1, s.c);
        Op op; op.kind = Op::CONV; op.conv = pc; op.src0 = src; op.residual = residual; op.relu = relu;
        op.dst = new_tensor(cout, (s.h + stride - 1) / stride, (s.w + stride - 1) / stride);
        g.ops.push_back(op);
        return op.dst;
    }
    int basic_block(int x) {       // wasb.py:48-64
        const int c = g.tensors[x].c;
        const int t = conv(x, c, 3, 1, 1);
        return conv(t, c, 3, 1, 1, /*residual*/ x);
    }
    Op bb_chain_op(int x, int n_convs, bool need_dst) {      // n_convs/2 BasicBlocks fused (bf16 path); not yet in the op list
        const TensorShape s = g.tensors[x];
        Op op; op.kind = Op::BB_CHAIN; op.src0 = x; op.n_chain = n_convs;
        for (int i = 0; i < n_convs; ++i) op.chain[i] = request(next(s.c, s.c, 3, 1), -1, s.c);
        op.dst = need_dst ? new_tensor(s.c, s.h, s.w) : -1;
        return op;
    }
    int bb_chain(int x, int n_convs) {
        const Op op = bb_chain_op(x, n_convs, true);
        g.ops.push_back(op);
        return op.dst;
    }

    // ---- HighResolutionModule (wasb.py:227-245)
    struct Stage {
        int nb = 0, n_out = 0; bool head_mode = false;
        std::vector<int> xs;                     // branch outputs (xs[0] is -1 when the deferred chain does not store its tensor)
        TensorShape x0;                          // shape of branch 0
        // the full-resolution branch's fuse-layer sum rides in the epilogue of its two-block chain, which is therefore emitted
        // AFTER the lower branches and their 1x1 fuse convs; its weights are still consumed in reference order
        Op deferred; bool has_deferred = false;
        int fuse[4][4][3];                       // folded convs of fuse layer i <- j: one 1x1 (j > i) or i - j stride-2 3x3 convs (j < i)
    };
    // the running sum of output i: `acc` starts at x_0 (i = 0) or at the j = 0 down-chain, the other terms are added at the end
    struct Sum {
        int acc = -1;
        std::vector<int> t, s;                   // further terms and their upsampling shifts, in branch order j (wasb.py:236-243)
        int last_chain_op = -1;                  // index in the op list of the conv that completes the running sum (j = i-1 chain)
    };

    void run_branches(Stage& S) {
        for (int b = 0; b < S.nb; ++b) {
            const int c = g.tensors[S.xs[b]].c;
            if (b == 0 && fuse && sw.fuse_sum && c == 16) {
                S.deferred = bb_chain_op(S.xs[0], 4, /*pre-fuse tensor has consumers*/ S.n_out > 1); S.has_deferred = true; S.xs[0] = S.deferred.dst;
            } else if (fuse && c == 16) S.xs[b] = bb_chain(S.xs[b], 4);                       // both blocks in one kernel
            else if (fuse && c == 32) { S.xs[b] = bb_chain(S.xs[b], 2); S.xs[b] = bb_chain(S.xs[b], 2); }
            else { S.xs[b] = basic_block(S.xs[b]); S.xs[b] = basic_block(S.xs[b]); }
        }
    }
    // reference order of the fuse convs in the state_dict: i major, j minor, chain index k.  Convs of dead fused outputs
    // (i >= n_out) are never requested but are consumed from the cursor all the same.
    void read_fuse_convs(Stage& S) {
        for (int i = 0; i < S.nb; ++i)
            for (int j = 0; j < S.nb; ++j) {
                if (j > i) S.fuse[i][j][0] = next(STAGE_CH[i], STAGE_CH[j], 1, 1);
                else for (int k = 0; k < i - j; ++k) S.fuse[i][j][k] = next(k == i - j - 1 ? STAGE_CH[i] : STAGE_CH[j], STAGE_CH[j], 3, 2);
            }
    }
    // j > i: 1x1 conv + BN at the low resolution, upsampled when summed
    void up_term(Stage& S, int i, int j, Sum& T) {
        const int pc = request(S.fuse[i][j][0], -1, 0);
        const TensorShape sj = g.tensors[S.xs[j]];
        const int dst = new_tensor(STAGE_CH[i], sj.h, sj.w);
        Op* po = fuse ? writer_of(S.xs[j]) : nullptr;
        bool attached = false;
        // 32 -> 16 on the output of a fused 32-channel block: rides in that kernel's epilogue (one MFMA per pixel group)
        if (po && sj.c == 32 && STAGE_CH[i] == 16 && po->kind == Op::BB_CHAIN && po->n_chain == 2 && po->conv2 < 0) {
            po->conv2 = pc; po->dst2 = dst; attached = true;
        }
        // 64 -> 16 / 64 -> 32 on the output of the branch's last 64 -> 64 conv: rides in that conv's epilogue
        if (po && !attached && sj.c == 64 && sw.fuse_lin && po->kind == Op::CONV && po->conv >= 0 && po->conv2 < 0 && po->src1 < 0) {
            const ConvRequest& pp = g.convs[po->conv];
            if (pp.k == 3 && pp.stride == 1 && pp.cout == 64 && pp.cin_total == 64 && pp.c0 == 64) {
                if (STAGE_CH[i] == 16 && po->lin16 < 0) { po->lin16 = pc; po->lin16_dst = dst; attached = true; }
                else if (STAGE_CH[i] == 32 && po->lin32 < 0) { po->lin32 = pc; po->lin32_dst = dst; attached = true; }
            }
        }
        if (!attached) {
            Op op; op.kind = Op::CONV; op.conv = pc; op.src0 = S.xs[j]; op.dst = dst; op.relu = 0;
            g.ops.push_back(op);
        }
        T.t.push_back(dst); T.s.push_back(j - i);
    }
    // the latest 3x3 stride-2 16 -> 32 conv that reads tensor t and has its epilogue and its pair slot free
    Op* pair_partner(int t) {
        for (size_t q = g.ops.size(); q-- > 0;) {
            Op& po = g.ops[q];
            if (po.kind != Op::CONV || po.src0 != t || po.conv < 0) continue;
            const ConvRequest& pp = g.convs[po.conv];
            if (pp.k == 3 && pp.stride == 2 && pp.cout == 32 && pp.cin_total == 16 && po.pair < 0 && po.conv2 < 0 && po.src1 < 0) return &po;
        }
        return nullptr;
    }
    // j < i: chain of stride-2 3x3 convs; the last one adds the running sum
    void down_chain(Stage& S, int i, int j, Sum& T) {
        int cur = S.xs[j];
        for (int k = 0; k < i - j; ++k) {
            const bool last = k + 1 == i - j;
            const FoldedConv& f = folded[S.fuse[i][j][k]];
            const int pc = request(S.fuse[i][j][k], -1, 0);
            const TensorShape sc = g.tensors[cur];
            const int dst = new_tensor(f.cout, (sc.h + 1) / 2, (sc.w + 1) / 2);
            Op op; op.kind = Op::CONV; op.conv = pc; op.src0 = cur; op.dst = dst; op.relu = last ? 0 : 1;
            if (last && T.acc >= 0) op.residual = T.acc;
            // 16 -> 16 on the full-resolution branch while an earlier fuse chain took the same tensor down 16 -> 32: both
            // convs in one pass over it (conv_s2_pair_kernel)
            Op* po = fuse && !last && f.cout == 16 && sc.c == 16 && sw.pair ? pair_partner(cur) : nullptr;
            if (po) { po->pair = pc; po->pair_dst = dst; po->pair_relu = op.relu; }
            else g.ops.push_back(op);
            if (last) T.last_chain_op = (int)g.ops.size() - 1;
            cur = dst;
        }
        T.acc = cur;
    }
    void set_terms(Op& op, const Sum& T) {
        op.n_terms = (int)T.t.size();
        if (T.t.size() > 3) { set_error("fuse: more than 3 upsample terms"); g.rc = TTUP_EINVAL; }
        for (size_t k = 0; k < T.t.size() && k < 3; ++k) { op.terms[k] = T.t[k]; op.shifts[k] = T.s[k]; }
    }
    int finish_sum(Stage& S, int i, const Sum& T) {
        if (i == 0 && S.has_deferred) {
            // y_0 = relu(x_0 + sum_j up(1x1(x_j))) in the epilogue of the branch's block chain
            set_terms(S.deferred, T);
            if (S.head_mode) { S.deferred.head = 1; S.deferred.dst2 = -1; }
            else S.deferred.dst2 = new_tensor(S.x0.c, S.x0.h, S.x0.w);
            g.ops.push_back(S.deferred);
            return S.deferred.dst2;
        }
        // bf16: y_i = relu(chains + x_i + up(...)) finishes in the epilogue of the last chain conv (x_i and one upsampled term
        // fit): the element-wise pass over the branch disappears
        if (fuse && T.last_chain_op >= 0 && T.t.size() <= 2) {
            Op& lc = g.ops[T.last_chain_op];
            lc.res2 = T.t[0];
            if (T.t.size() == 2) { lc.res3 = T.t[1]; lc.sh3 = T.s[1]; }
            lc.relu = 1;
            return lc.dst;
        }
        // y = relu(acc + sum of upsampled / late identity terms)
        const TensorShape xi = i == 0 ? S.x0 : g.tensors[S.xs[i]];
        Op op; op.kind = Op::UPSUM; op.src0 = T.acc; op.dst = new_tensor(xi.c, xi.h, xi.w);
        set_terms(op, T);
        g.ops.push_back(op);
        return op.dst;
    }
    // returns fused outputs 0..n_out-1
    std::vector<int> stage(std::vector<int> xs, int n_out, bool head_mode = false) {
        Stage S; S.nb = (int)xs.size(); S.n_out = n_out; S.head_mode = head_mode; S.x0 = g.tensors[xs[0]]; S.xs = xs;
        run_branches(S);
        read_fuse_convs(S);
        std::vector<int> outs;
        for (int i = 0; i < n_out; ++i) {
            Sum T;
            // emission order: the 1x1 convs of the lower branches (j > i) first, so that a later conv's epilogue can add them
            if (i > 0) { T.t.push_back(S.xs[i]); T.s.push_back(0); }          // x_i joins a sum that a down-chain started: a term with shift 0
            for (int j = i + 1; j < S.nb; ++j) up_term(S, i, j, T);
            for (int j = 0; j < i; ++j) down_chain(S, i, j, T);
            if (i == 0) T.acc = S.xs[0];
            outs.push_back(finish_sum(S, i, T));
        }
        return outs;
    }

    // ---- stem (wasb.py:446-451); returns the second 64-channel tensor, *a1 = Bottleneck conv1's output
    int stem(int* a1) {
        g.t_input = new_tensor(16, H, W);
        if (fuse && sw.stem) {
            // conv1 + conv2 + Bottleneck conv1 in one persistent kernel; the first 64-channel tensor never reaches HBM
            const int i1 = next(64, in_ch, 3, 1);
            const FoldedConv& c1 = folded[i1];
            const int p1 = request(i1, -1, 16);
            // the same conv for the stem's frames mode: input slot f*4 + c holds colour c of frame f (slot 3 of every frame and the
            // slots past the last frame carry zero weights)
            FoldedConv c1f = c1;
            c1f.cin = 16; c1f.w.assign((size_t)64 * 16 * 9, 0.f);
            for (int co = 0; co < 64 && g.rc == TTUP_OK; ++co)
                for (int ci = 0; ci < in_ch; ++ci)
                    for (int t = 0; t < 9; ++t) c1f.w[((size_t)co * 16 + (ci / 3) * 4 + ci % 3) * 9 + t] = c1.w[((size_t)co * in_ch + ci) * 9 + t];
            g.synth.push_back(std::move(c1f));
            int p1f = request(0, -1, 16, true);
            // ... and, for triples, the 4-k-step form of that conv (csrc/conv_stem.h stem_kernel<3, true>): K = 3 tap rows x 40 slots, slot
            // o of a row = pixel dx = o / 12, frame (o % 12) / 4, colour o % 4 (colour 3 and o >= 36: zero weights), packed as a
            // "1x1 conv with 128 inputs" so that k-step s, lane group g, element j holds k = 32 s + 8 g + j
            if (in_ch == 9) {
                FoldedConv c1k = c1;
                c1k.cin = 128; c1k.k = 1; c1k.w.assign((size_t)64 * 128, 0.f);
                for (int co = 0; co < 64 && g.rc == TTUP_OK; ++co)
                    for (int r = 0; r < 3; ++r)
                        for (int o = 0; o < 36; ++o) {
                            const int dx = o / 12, f = (o % 12) / 4, col = o % 4;
                            if (col < 3) c1k.w[(size_t)co * 128 + r * 40 + o] = c1.w[((size_t)co * in_ch + f * 3 + col) * 9 + r * 3 + dx];
                        }
                g.synth.push_back(std::move(c1k));
                p1f = request(1, -1, 0, true);
            }
            Op op; op.kind = Op::STEM; op.conv = p1; op.conv1f = p1f; op.src0 = g.t_input;
            op.conv2 = request(next(64, 64, 3, 1), -1, 0);
            op.conv3 = request(next(32, 64, 1, 1), -1, 0);
            op.dst = new_tensor(64, H, W); g.taps["stem2"] = op.dst;
            op.dst2 = *a1 = new_tensor(32, H, W);
            g.ops.push_back(op);
            // (micro + nf - 1) frames of (H, W, 4) bf16
            if (sw.frames_mode) g.t_frames = new_tensor(4, H, W, in_ch / 3 - 1);
            return op.dst;
        }
        int x;
        {
            Op op; op.conv = request(next(64, in_ch, 3, 1), -1, 16); op.src0 = g.t_input; op.dst = new_tensor(64, H, W); op.relu = 1;
            g.ops.push_back(op);
            x = op.dst; g.taps["stem1"] = x;
        }
        x = conv(x, 64, 3, 1, 1); g.taps["stem2"] = x;
        if (fuse) {       // Bottleneck conv1 (1x1 64->32 + ReLU) rides in the epilogue of stem conv2
            Op& c2 = g.ops.back();
            c2.conv2 = request(next(32, 64, 1, 1), -1, 0);
            c2.dst2 = *a1 = new_tensor(32, H, W);
        } else *a1 = conv(x, 32, 1, 1, 1);
        return x;
    }
    // layer1: Bottleneck(64 -> 32 -> 128) (wasb.py:85-105), conv3 + downsample fused into one two-source 1x1 conv;
    // transition1 (wasb.py:454-459).  bf16: both run in one kernel and the 128-channel tensor stays in LDS.
    std::vector<int> layer1(int x, int a1) {
        std::vector<int> xs(2);
        const int a2 = conv(a1, 32, 3, 1, 1);
        const int c3 = next(128, 32, 1, 1);
        const int ds = next(128, 64, 1, 1);
        const int pc = request(c3, ds, 0);
        if (fuse) {
            Op op; op.kind = Op::BNECK_TRANS; op.conv = pc; op.src0 = a2; op.src1 = x;
            op.conv2 = request(next(16, 128, 3, 1), -1, 0);
            op.conv3 = request(next(32, 128, 3, 2), -1, 0);
            op.dst = xs[0] = new_tensor(16, H, W);
            op.dst2 = xs[1] = new_tensor(32, H / 2, W / 2);
            g.ops.push_back(op);
        } else {
            Op op; op.conv = pc; op.src0 = a2; op.src1 = x; op.dst = new_tensor(128, H, W); op.relu = 1;
            g.ops.push_back(op);
            x = op.dst; g.taps["layer1"] = x;
            xs[0] = conv(x, 16, 3, 1, 1);
            xs[1] = conv(x, 32, 3, 2, 1);
        }
        g.taps["trans1_0"] = xs[0]; g.taps["trans1_1"] = xs[1];
        return xs;
    }
    void build() {
        int a1 = -1;
        const int x = stem(&a1);
        std::vector<int> xs = layer1(x, a1);
        std::vector<int> ys = stage(xs, 2);
        g.taps["stage2_0"] = ys[0]; g.taps["stage2_1"] = ys[1];
        // transition2: new branch from the last output (wasb.py:462-467)
        xs = {ys[0], ys[1], conv(ys[1], 64, 3, 2, 1)};
        ys = stage(xs, 3);
        g.taps["stage3_0"] = ys[0]; g.taps["stage3_1"] = ys[1]; g.taps["stage3_2"] = ys[2];
        xs = {ys[0], ys[1], ys[2], conv(ys[2], 128, 3, 2, 1)};
        const bool head_in_chain = fuse && n_out == 1 && sw.fuse_sum;
        ys = stage(xs, 1, head_in_chain);
        g.t_out = ys[0];
        Op& last = g.ops.back();
        if (head_in_chain && last.kind == Op::BB_CHAIN && last.head) {
            g.fused_head = true;                       // stage-4 output 0 lives only in the registers of the last block chain
        } else if (fuse && n_out == 1 && last.kind == Op::UPSUM && last.dst == ys[0]) {
            last.kind = Op::UPSUM_HEAD;                // stage-4 output 0 is consumed in registers and never stored
            g.fused_head = true;
        } else {
            g.taps["stage4_0"] = ys[0];
        }
        g.consumed = cursor;
    }
};

// H and W are multiples of 8 (ttup_wasb_create checks it)
inline GraphPlan build_graph(const std::vector<FoldedConv>& folded, int in_ch, int n_out, int H, int W, int micro, int dtype, const GraphSwitches& sw) {
    GraphPlan g;
    g.micro = micro; g.dtype = dtype;
    if ((int)folded.size() != WASB_CONVS) { set_error("wasb: %zu folded convs, expected %d", folded.size(), WASB_CONVS); g.rc = TTUP_EFORMAT; return g; }
    GraphBuilder b{g, folded, sw, in_ch, n_out, H, W, dtype == TTUP_DTYPE_BF16 && sw.fuse};
    b.build();
    if (g.rc == TTUP_OK && g.consumed != folded.size() - 1) {
        set_error("wasb: consumed %zu of %zu convs", g.consumed, folded.size() - 1);
        g.rc = TTUP_EFORMAT;
    }
    return g;
}

}  // namespace ttup
