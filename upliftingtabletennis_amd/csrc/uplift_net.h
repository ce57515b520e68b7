// The uplift transformer's handle and weight tables (csrc/uplift.hip builds and runs them; csrc/uplift_grad.hip reads them for the
// training loss and its gradients), and the 1-D launch both units use.
#pragma once
#include "common.h"
#include "uplift_grad_plan.h"
#include <map>
#include <utility>
#include <vector>

namespace ttup {
namespace upl {

// ------------------------------------------------------------------ packed linear layer
struct Linear {
    int n = 0, k = 0;            // out features, in features
    float* w_dev = nullptr;      // MFMA path: [ntile][k/16][64 lanes][4]; small-K path: [n][k] row major
    float* b_dev = nullptr;      // [n] or null
    bool mfma = false;
    // K = 128 layers (all of the 'large' model's transformer layers): the weights split into three bf16 parts, packed per
    // v_mfma_f32_16x16x32_bf16 A fragment: [ntile][k/32][plane][64 lanes][8] (linear_x3_kernel, csrc/uplift_linear.h)
    uint16_t* w3_dev = nullptr;
};

// weight pointers of one layer for stage_x3_kernel (csrc/uplift_stage.h)
struct StageLayerW {
    const uint16_t *w_qkv, *w_proj, *w_fc1, *w_fc2;
    const float *b_qkv, *g1, *b1, *g2, *b2, *bias1, *bias2;
};

// The sequences an attention kernel works on, in a flat [n_seq * S][..] token array
struct SeqView {
    const float* mask;      // additive {0, -inf}; row of sequence seq = seq / mask_div, S entries
    const float2* rope;     // (cos, sin) rows of hd/2; row of token j of sequence seq = (seq / times_div) * times_stride + j - num_cls
    int S, num_cls;         // tokens per sequence; leading tokens that are not rotated (the cls token)
    int mask_div, times_div, times_stride;
    float scale;            // 1 / sqrt(head dim)
};

struct Layer { Linear qkv, proj, fc1, fc2; float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr; };
struct Mlp2 { Linear fc1, fc2; };
struct Head { Linear fc1, fc2, fc3; };
// the variant of get_model a blob holds (hdr[6], hdr[7]; include/ttup.h)
enum { NAME_CONNECT = 0, NAME_MULTI = 1, NAME_SINGLE = 2 };
enum { MODE_DYNAMIC = 0, MODE_STACKED = 1, MODE_ORIGINAL = 2, MODE_FREE = 3 };

// host only: one thread per element, 256 threads a workgroup
template <typename... P, typename... A>
int launch_1d(void (*kernel)(P...), long long n, hipStream_t st, A... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, args...);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

}  // namespace upl
}  // namespace ttup

struct ttup_uplift {
    // (the member types live in ttup::upl)
    typedef ttup::upl::Linear Linear; typedef ttup::upl::Layer Layer; typedef ttup::upl::Mlp2 Mlp2; typedef ttup::upl::Head Head;
    typedef ttup::upl::StageLayerW StageLayerW;
    int D = 0, heads = 0, hd = 0, n_table = 13, max_batch = 0, max_len = 0, chunk = 1;
    int name = ttup::upl::NAME_CONNECT, mode = ttup::upl::MODE_DYNAMIC; bool rot_old = false;
    float *embed_w1t = nullptr, *embed_b1 = nullptr, *embed_w2t = nullptr, *embed_b2 = nullptr;      // 'multistage': embed, weights transposed [K][D]
    float *stacked_wt = nullptr, *stacked_b = nullptr;                                                // 'stacked' / 'originalmethod': ball_embed.fc1 transposed [K][D]
    float2* rope_index = nullptr;          // time_rotation 'old': [max_len][hd/2], row = index of the token in its sequence
    float* pos_rows = nullptr;             // 'singlestage': position head output on all T+1 rows
    std::vector<Layer> pos_layers, layers, second;
    Mlp2 ball_embed, table_embed;
    Head position_head, rotation_head;
    float* cls_dev = nullptr; float* inv_freq_dev = nullptr; float* table_times_dev = nullptr;
    std::vector<StageLayerW> stage_pos, stage_first, stage_second;      // weight pointers of the three stages' layers (stage_x3_kernel); empty = not available
    long long stage_launches = 0;
    long long* stage_stamps = nullptr;          // TTUP_STAGE_STAMPS: the stage kernel's cycle stamps, allocated on first use
    float2 *rope = nullptr, *table_rope = nullptr;      // (cos, sin) tables: [chunk*max_len][hd/2] per forward, [n_table][hd/2] fixed
    std::vector<void*> allocs;
    // 'connectstage' / 'dynamic' only: every record of the blob after inv_freq as plain fp32, in blob order -- the used tensors of
    // grad_layout (csrc/uplift_grad_plan.h) back to back, i.e. the gradient buffer without its hole (csrc/uplift_grad.hip: dX needs W itself)
    float* plain = nullptr; long long plain_floats = 0;
    bool trained = false;          // ttup_uplift_opt_step has changed `plain` (csrc/uplift_opt.hip): the packed weights below no longer match it
    // scratch (sized for `chunk` trajectories of max_len tokens)
    float *x = nullptr, *qkv = nullptr, *att = nullptr, *hid = nullptr, *x2 = nullptr, *tok = nullptr, *ttok = nullptr, *h1 = nullptr;
    float *m1 = nullptr, *m2 = nullptr, *tmask = nullptr, *txy = nullptr;
    int* flags_dev = nullptr;
    // Small batches (a rally or a handful of them: the hub surface, the pipeline's per-clip uplift) are launch-bound -- about
    // eighty kernels of a few microseconds each.  Their forward is captured once per (batch, length) into a hipGraph that works
    // on handle-owned input / output buffers and is replayed with one launch (+ six small copies around it).
    struct GraphEntry { hipGraphExec_t exec = nullptr; int seen = 0; };
    std::map<std::pair<int, int>, GraphEntry> graphs;
    bool graphs_off = false;
    float *g_ball = nullptr, *g_table = nullptr, *g_mask = nullptr, *g_times = nullptr, *g_rot = nullptr, *g_pos = nullptr;
    long long graph_tokens = 0;          // largest batch * len served by a graph
    long long graph_replays = 0;
    ~ttup_uplift() {
        for (auto& kv : graphs) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        for (void* p : allocs) if (p) (void)hipFree(p);
    }
};

namespace ttup {
namespace upl {
// the handle trains: connectstage/dynamic with its plain weights -- the one variant the gradient pass and the optimizer serve
inline bool trains(const ttup_uplift* net) { return net->name == NAME_CONNECT && net->mode == MODE_DYNAMIC && net->plain && net->plain_floats > 0; }
inline GradDims grad_dims(const ttup_uplift* net) {
    return {net->D, net->hd, net->n_table, (int)net->pos_layers.size(), (int)net->layers.size(), (int)net->second.size()};
}
}  // namespace upl
}  // namespace ttup
