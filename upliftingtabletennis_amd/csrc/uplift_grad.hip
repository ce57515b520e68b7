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
#include "uplift_grad_kernels.h"
#include "uplift_grad_attention.h"
#include <math.h>
#include <vector>

using namespace ttup;
using namespace ttup::upl;
using namespace ttup::gemm;

namespace {

constexpr int FLAG_LOCAL = 1;                // transform_mode == 'local'
constexpr int FLAG_CHECK_MASK = 2;           // the reference's mask-format ValueError (model.py:541-546): one read-back and one stream synchronisation

struct Ctx {
    hipStream_t st;
    float* partial;          // scratch of the sliced reductions
};

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
int linear_fwd(const Ctx& c, const float* x, int ldx, const float* W, const float* b, float* out, int ldo, long long M, int N, int K, int flags = 0,
               const float* res = nullptr, int ldr = 0) {
    return gemm<O_ROWS, O_ROWS>(x, ldx, W, K, out, ldo, M, N, K, b, flags, res, ldr, nullptr, 0, 0, c.st);
}
// dx[m][k] = sum_n dy[m][n] W[n][k]   (E_RESID: + res;  E_GATE: where gate > 0)
int linear_dx(const Ctx& c, const float* dy, int ldy, const float* W, float* dx, int ldx, long long M, int N, int K, int flags = 0, const float* res = nullptr,
              int ldr = 0, const float* gate = nullptr, int ldg = 0) {
    return gemm<O_ROWS, O_COLS>(dy, ldy, W, K, dx, ldx, M, K, N, nullptr, flags, res, ldr, gate, ldg, 0, c.st);
}
int reduce_into(const Ctx& c, int slices, long long n, float* out) {
    return launch_1d(reduce_kernel, n, c.st, c.partial, slices, n, out);
}
// g[n] += column sums of z (M rows of leading dimension ldz)
int colsum_into(const Ctx& c, const float* z, long long ldz, long long M, int N, float* g) {
    if (M == 0) return TTUP_OK;
    const int slices = (int)kslices(M);
    hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)((N + 63) / 64), (unsigned)slices), dim3(1024), 0, c.st, z, ldz, M, N, c.partial);
    TTUP_LAUNCH_CHECK();
    return reduce_into(c, slices, N, g);
}
// gW[n][k] += sum_m dy[m][n] x[m][k];  gb[n] += sum_m dy[m][n]
int linear_dw(const Ctx& c, const float* dy, int ldy, const float* x, int ldx, long long M, int N, int K, float* gW, float* gb) {
    if (M == 0) return TTUP_OK;
    if (int rc = gemm<O_COLS, O_COLS>(dy, ldy, x, ldx, c.partial, K, N, K, (int)M, nullptr, 0, nullptr, 0, nullptr, 0, KSLICE, c.st)) return rc;
    if (int rc = reduce_into(c, (int)kslices(M), (long long)N * K, gW)) return rc;
    return gb ? colsum_into(c, dy, ldy, M, N, gb) : TTUP_OK;
}

// ------------------------------------------------------------------ parameters and workspace (the tables: uplift_grad_plan.h)
struct LinP { const float *w, *b; float *gw, *gb; int n, k; };
struct LayerP { LinP qkv, proj, fc1, fc2; const float *g1, *b1, *g2, *b2; float *dg1, *db1, *dg2, *db2; };
struct HeadP { LinP fc1, fc2, fc3; };
struct Params {
    const float* cls; float* dcls;
    LinP ball1, ball2, tab1, tab2;
    std::vector<LayerP> pos, first, second;
    HeadP pos_head, rot_head;
};

// walks the layout's used tensors in step with the plain weights, which hold exactly those, back to back
void map_params(const ttup_uplift* net, const GradLayout& lay, float* grad, Params* P) {
    const float* w = net->plain;
    size_t i = 0;
    auto vec = [&](const float** pw, float** pg) {
        while (!lay.t[i].used) ++i;
        *pw = w; *pg = grad + lay.t[i].offset; w += lay.t[i].count(); ++i;
    };
    auto lin = [&](LinP* L, bool bias = true) {
        vec(&L->w, &L->gw);
        L->n = lay.t[i - 1].n; L->k = lay.t[i - 1].k; L->b = nullptr; L->gb = nullptr;
        if (bias) vec(&L->b, &L->gb);
    };
    auto layer = [&](LayerP* L) {
        lin(&L->qkv); lin(&L->proj, false); lin(&L->fc1); lin(&L->fc2);
        vec(&L->g1, &L->dg1); vec(&L->b1, &L->db1); vec(&L->g2, &L->dg2); vec(&L->b2, &L->db2);
    };
    auto head = [&](HeadP* H) { lin(&H->fc1); lin(&H->fc2); lin(&H->fc3); };
    vec(&P->cls, &P->dcls);
    lin(&P->ball1); lin(&P->ball2); lin(&P->tab1); lin(&P->tab2);
    P->pos.resize(net->pos_layers.size()); P->first.resize(net->layers.size()); P->second.resize(net->second.size());
    for (auto& L : P->pos) layer(&L);
    for (auto& L : P->first) layer(&L);
    head(&P->pos_head);
    for (auto& L : P->second) layer(&L);
    head(&P->rot_head);
}

typedef SavedT<float*> Saved;
typedef StageT<float*> Stage;
typedef PlanT<float*> Plan;
void make_plan(const ttup_uplift* net, int batch, int len, float* base, Plan* p) {
    plan_workspace(grad_dims(net), batch, len, p, [base](long long off, long long, long long) { return base ? base + off : nullptr; });
}
const char* variant_text(const ttup_uplift* net) {
    static const char* names[] = {"connectstage", "multistage", "singlestage"};
    static const char* modes[] = {"dynamic", "stacked", "originalmethod", "free"};
    static thread_local char buf[64];
    snprintf(buf, sizeof buf, "%s/%s", names[net->name % 3], modes[net->mode % 4]);
    return buf;
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
    GRC(linear_fwd(c, p.tA, D, L.qkv.w, L.qkv.b, S.qkv, 3 * D, M, 3 * D, D));
    AttnArgs a = {};
    a.qkv = S.qkv; a.sv = sv; a.out = S.att; a.n_seq = n_seq;
    GRC(run_attention<false>(net, a, c.st));
    GRC(linear_fwd(c, S.att, D, L.proj.w, nullptr, S.x2, D, M, D, D, E_RESID, S.x, D));
    GRC(ln_fwd(c, S.x2, L.g2, L.b2, p.tA, M, D));
    GRC(linear_fwd(c, p.tA, D, L.fc1.w, L.fc1.b, S.hp, D, M, D, D));
    LAUNCH1D(relu_kernel, M * D, S.hp, p.tB, M * D);
    return linear_fwd(c, p.tB, D, L.fc2.w, L.fc2.b, xo, D, M, D, D, E_RESID, S.x2, D);
}
// its backward: dxo (gradient at the layer's output) -> dxi (at its input; may be the same buffer), parameter gradients accumulated
int layer_bwd(const ttup_uplift* net, const Ctx& c, const Plan& p, const LayerP& L, const Saved& S, const float* dxo, float* dxi, const Stage& sg,
              int n_seq, const SeqView& sv) {
    const int D = net->D;
    const long long M = (long long)n_seq * sg.S;
    // fc2
    LAUNCH1D(relu_kernel, M * D, S.hp, p.tA, M * D);
    GRC(linear_dw(c, dxo, D, p.tA, D, M, D, D, L.fc2.gw, L.fc2.gb));
    GRC(linear_dx(c, dxo, D, L.fc2.w, p.tB, D, M, D, D, E_GATE, nullptr, 0, S.hp, D));      // tB = d hp
    // fc1 over LayerNorm 2
    GRC(ln_fwd(c, S.x2, L.g2, L.b2, p.tA, M, D));
    GRC(linear_dw(c, p.tB, D, p.tA, D, M, D, D, L.fc1.gw, L.fc1.gb));
    GRC(linear_dx(c, p.tB, D, L.fc1.w, p.tA, D, M, D, D));                         // tA = d LN2(x2)
    hipLaunchKernelGGL(ln_bwd_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, c.st, S.x2, L.g2, p.tA, dxo, p.tC, p.tE, M, D);      // tC = d x2
    TTUP_LAUNCH_CHECK();
    GRC(colsum_into(c, p.tE, D, M, D, L.dg2));
    GRC(colsum_into(c, p.tA, D, M, D, L.db2));
    // proj
    GRC(linear_dw(c, p.tC, D, S.att, D, M, D, D, L.proj.gw, nullptr));
    GRC(linear_dx(c, p.tC, D, L.proj.w, p.tA, D, M, D, D));                        // tA = d att
    AttnArgs a = {};
    a.qkv = S.qkv; a.sv = sv; a.o = S.att; a.d_o = p.tA; a.dqkv = p.tQ; a.n_seq = n_seq;
    GRC(run_attention<true>(net, a, c.st));
    // qkv over LayerNorm 1
    GRC(ln_fwd(c, S.x, L.g1, L.b1, p.tB, M, D));
    GRC(linear_dw(c, p.tQ, 3 * D, p.tB, D, M, 3 * D, D, L.qkv.gw, L.qkv.gb));
    GRC(linear_dx(c, p.tQ, 3 * D, L.qkv.w, p.tA, D, M, 3 * D, D));                 // tA = d LN1(x)
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
    GRC(linear_fwd(c, x, ldx, H.fc1.w, H.fc1.b, h1, D / 2, M, D / 2, D, E_RELU));
    GRC(linear_fwd(c, h1, D / 2, H.fc2.w, H.fc2.b, h2, D / 4, M, D / 4, D / 2, E_RELU));
    return linear_fwd(c, h2, D / 4, H.fc3.w, H.fc3.b, out, 3, M, 3, D / 4);
}
// d_out (M,3) -> dx (M,D); t1 / t2 are scratch of M*D/2 and M*D/4 floats
int head_bwd(const ttup_uplift* net, const Ctx& c, const HeadP& H, const float* x, int ldx, long long M, const float* h1, const float* h2,
             const float* d_out, float* t1, float* t2, float* dx) {
    const int D = net->D;
    GRC(linear_dw(c, d_out, 3, h2, D / 4, M, 3, D / 4, H.fc3.gw, H.fc3.gb));
    GRC(linear_dx(c, d_out, 3, H.fc3.w, t2, D / 4, M, 3, D / 4, E_GATE, nullptr, 0, h2, D / 4));
    GRC(linear_dw(c, t2, D / 4, h1, D / 2, M, D / 4, D / 2, H.fc2.gw, H.fc2.gb));
    GRC(linear_dx(c, t2, D / 4, H.fc2.w, t1, D / 2, M, D / 4, D / 2, E_GATE, nullptr, 0, h1, D / 2));
    GRC(linear_dw(c, t1, D / 2, x, ldx, M, D / 2, D, H.fc1.gw, H.fc1.gb));
    return linear_dx(c, t1, D / 2, H.fc1.w, dx, D, M, D / 2, D);
}
// the 2 -> D -> D embeddings (model.py:105-158): in (M,2) -> tok, keeping the hidden activation; and back (d_tok is overwritten)
int embed_fwd(const ttup_uplift* net, const Ctx& c, const LinP& f1, const LinP& f2, const float* in, long long M, float* h, float* tok) {
    const int D = net->D;
    GRC(linear_fwd(c, in, 2, f1.w, f1.b, h, D, M, D, 2, E_RELU));
    return linear_fwd(c, h, D, f2.w, f2.b, tok, D, M, D, D);
}
int embed_bwd(const ttup_uplift* net, const Ctx& c, const LinP& f1, const LinP& f2, const float* in, long long M, const float* h, const float* d_tok, float* tmp) {
    const int D = net->D;
    GRC(linear_dw(c, d_tok, D, h, D, M, D, D, f2.gw, f2.gb));
    GRC(linear_dx(c, d_tok, D, f2.w, tmp, D, M, D, D, E_GATE, nullptr, 0, h, D));
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
    TTUP_REQUIRE(trains(net), TTUP_EINVAL, "ttup_uplift_grad_layout: gradients are served for connectstage/dynamic only, this handle holds %s", variant_text(net));
    const GradLayout lay = grad_layout(grad_dims(net));
    for (int i = 0; i < (int)lay.t.size() && i < capacity; ++i) {
        if (offsets_host) offsets_host[i] = lay.t[i].offset;
        if (used_host) used_host[i] = lay.t[i].used;
    }
    *n_floats = lay.total; *n_tensors = (int)lay.t.size();
    return TTUP_OK;
}

extern "C" size_t ttup_uplift_grad_workspace_bytes(ttup_uplift* net, int batch, int len) {
    if (!net || batch <= 0 || len <= 0 || !trains(net)) return 0;
    Plan p;
    make_plan(net, batch, len, nullptr, &p);
    return (size_t)p.total * sizeof(float);
}

extern "C" int ttup_uplift_loss_grad(ttup_uplift* net, const float* ball_dev, const float* table_dev, const float* mask_dev, const float* times_dev,
                                     const float* r_world_dev, const float* rotation_dev, int batch, int len, int flags, void* workspace,
                                     size_t workspace_bytes, float* grad_dev, float* loss_dev, float* rot_dev, float* pos_dev, void* stream) {
    TTUP_REQUIRE(net && ball_dev && table_dev && mask_dev && times_dev && r_world_dev && rotation_dev && workspace && grad_dev && loss_dev && rot_dev && pos_dev,
                 TTUP_EINVAL, "ttup_uplift_loss_grad: null pointer");
    TTUP_REQUIRE(trains(net), TTUP_EINVAL, "ttup_uplift_loss_grad: gradients are served for connectstage/dynamic only, this handle holds %s", variant_text(net));
    TTUP_REQUIRE(batch > 0 && len > 0 && len <= 255, TTUP_EINVAL, "ttup_uplift_loss_grad: batch %d / sequence length %d outside [1,..] x [1,255]", batch, len);
    TTUP_REQUIRE(grad_attention_served(grad_dims(net), len), TTUP_EINVAL, "ttup_uplift_loss_grad: head_dim %d / sequence length %d not served by the attention kernels",
                 net->hd, len);
    TTUP_REQUIRE((flags & ~(FLAG_LOCAL | FLAG_CHECK_MASK)) == 0, TTUP_EINVAL, "ttup_uplift_loss_grad: unknown flag bits %d", flags);
    TTUP_REQUIRE(!(flags & FLAG_LOCAL) || len >= 2, TTUP_EINVAL, "ttup_uplift_loss_grad: transform_mode 'local' needs at least two positions");
    TTUP_REQUIRE(!net->rot_old || len <= net->max_len, TTUP_EINVAL, "ttup_uplift_loss_grad: sequence length %d above the handle's %d", len, net->max_len);
    TTUP_REQUIRE(((size_t)workspace & 15) == 0, TTUP_EINVAL, "ttup_uplift_loss_grad: workspace must be 16-byte aligned");
    Plan p;
    make_plan(net, batch, len, (float*)workspace, &p);
    TTUP_REQUIRE(workspace_bytes >= (size_t)p.total * sizeof(float), TTUP_EINVAL, "ttup_uplift_loss_grad: workspace of %zu bytes, %zu needed", workspace_bytes,
                 (size_t)p.total * sizeof(float));
    const GradLayout lay = grad_layout(grad_dims(net));
    TTUP_REQUIRE(lay.total - lay.hole_len == net->plain_floats, TTUP_EINVAL, "ttup_uplift_loss_grad: the handle's plain weights do not fit the layout");
    Params W;
    map_params(net, lay, grad_dev, &W);
    Ctx c{(hipStream_t)stream, p.partial};
    TTUP_HIP_CHECK(hipMemsetAsync(grad_dev, 0, (size_t)lay.total * sizeof(float), c.st));
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
