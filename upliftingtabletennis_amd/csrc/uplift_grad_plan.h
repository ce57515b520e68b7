// The uplift gradient pass's decisions without a device (csrc/uplift_grad.hip, csrc/uplift_opt.hip): the flat gradient buffer's
// layout, the size of a group of trajectories, the workspace plan and the attention kernels' launch geometry, as functions of plain
// integers.  Standard headers only -- the same source compiles for gfx950 (hipcc) and for the host (g++:
// tests/helpers/host_uplift_grad_plan.cpp checks the layout against arch.uplift_grad_layout, the workspace for alignment, overlap
// and sizing over a sweep of (size, batch, len), and the geometry for every sequence length).
#pragma once
#include <stddef.h>
#include <vector>

namespace ttup {
namespace upl {

constexpr int KSLICE = 512;                  // rows per partial sum of dW / db / dgamma / dbeta / d cls
constexpr long long GROUP_TOKENS = 262144;   // table-stage tokens (n_table + 1 per time step) per group of trajectories

// the connectstage/dynamic model: width, head dim, table keypoints, layers of the table (pos_layers), temporal and spin stages
struct GradDims { int D, hd, n_table, pos_layers, first_layers, second_layers; };

// ------------------------------------------------------------------ the gradient buffer's layout
// The rows a parameter's gradient is summed over, per group: trajectories (G), time steps (G len: ball embedding, temporal stage,
// position head), table keypoints (G n_table), table-stage tokens (G len (n_table + 1)), spin-stage tokens (G (len + 1))
enum GradRows { ROWS_NONE, ROWS_TRAJ, ROWS_TIME, ROWS_KEYPOINT, ROWS_TABLE, ROWS_SPIN };

// One tensor of the state dict in arch.uplift_variant_schema order without the inv_freq buffers: a weight [n][k] or, k = 0, a
// vector of n.  `used` is false for embed.*, which 'connectstage' holds and never reads: no gradient, and no plain weights either.
struct GradTensor {
    int n, k;
    long long offset;          // floats
    bool used;
    GradRows rows;
    long long count() const { return k ? (long long)n * k : n; }
};
struct GradLayout {
    std::vector<GradTensor> t;
    long long total = 0;                       // floats of the gradient buffer
    long long hole_begin = 0, hole_len = 0;    // the embed.* stretch; the plain weights hold total - hole_len floats
};

inline GradLayout grad_layout(const GradDims& d) {
    const int D = d.D;
    GradLayout L;
    auto add = [&](int n, int k, GradRows rows) {
        const GradTensor t{n, k, L.total, rows != ROWS_NONE, rows};
        if (!t.used) {
            if (!L.hole_len) L.hole_begin = t.offset;
            L.hole_len += t.count();
        }
        L.total += t.count();
        L.t.push_back(t);
    };
    auto lin = [&](int n, int k, GradRows rows, bool bias = true) { add(n, k, rows); if (bias) add(n, 0, rows); };
    auto mlp = [&](int din, GradRows rows) { lin(D, din, rows); lin(D, D, rows); };
    auto layer = [&](GradRows rows) {
        lin(3 * D, D, rows); lin(D, D, rows, false); lin(D, D, rows); lin(D, D, rows);          // qkv, proj, mlp1.fc1, mlp1.fc2
        for (int i = 0; i < 4; ++i) add(D, 0, rows);                                            // norm1 weight, bias; norm2 weight, bias
    };
    auto head = [&](GradRows rows) { lin(D / 2, D, rows); lin(D / 4, D / 2, rows); lin(3, D / 4, rows); };
    add(D, 0, ROWS_TRAJ);          // cls_token
    mlp(3, ROWS_NONE);             // embed
    mlp(2, ROWS_TIME);             // ball_embed
    mlp(2, ROWS_KEYPOINT);         // table_embed
    for (int i = 0; i < d.pos_layers; ++i) layer(ROWS_TABLE);
    for (int i = 0; i < d.first_layers; ++i) layer(ROWS_TIME);
    head(ROWS_TIME);               // position head
    for (int i = 0; i < d.second_layers; ++i) layer(ROWS_SPIN);
    head(ROWS_TRAJ);               // rotation head, on the cls rows
    return L;
}

// ------------------------------------------------------------------ groups and the workspace
// trajectories per group: a function of len alone, so that every reduction tree depends on (batch, len) only
inline int group_size(int batch, int len) {
    long long g = GROUP_TOKENS / ((long long)len * 14);
    if (g < 1) g = 1;
    return (int)(g < batch ? g : batch);
}
inline long long kslices(long long rows) { return (rows + KSLICE - 1) / KSLICE; }

// what the forward keeps of one layer (floats per token: 7 D)
template <class T> struct SavedT { T x, qkv, att, x2, hp; };
template <class T> struct StageT { std::vector<SavedT<T>> L; T out; long long tokens; int n_seq, S, num_cls; };
// The workspace of one call.  T is what stands for a buffer: a float* in the pass, an (offset, rows, width) record in the host test.
template <class T> struct PlanT {
    int G = 0;                                   // trajectories per group
    long long n1 = 0, nt = 0, n2 = 0, nk = 0;    // table-stage / temporal / spin tokens and table keypoints of a full group
    long long total = 0;                         // floats
    StageT<T> table, temporal, spin;
    T tA, tB, tC, tE, dX, dY, tQ, partial;
    T ball_h, ball_tok, tab_h, tab_tok, pos_h1, pos_h2, rot_h1, rot_h2;
    T m1, m2, tmask, txy, rope, rot_t, d_rot, d_pos, mask_sum;
    long long rows(GradRows r) const { return r == ROWS_TRAJ ? G : r == ROWS_TIME ? nt : r == ROWS_KEYPOINT ? nk : r == ROWS_TABLE ? n1 : r == ROWS_SPIN ? n2 : 0; }
};

// Cuts the workspace: buffer(offset, rows, width) stands for the rows x width floats at `offset` (a multiple of four floats)
template <class T, class F>
void plan_workspace(const GradDims& d, int batch, int len, PlanT<T>* p, F buffer) {
    const int D = d.D, NT = d.n_table;
    p->G = group_size(batch, len);
    p->nt = (long long)p->G * len; p->n1 = p->nt * (NT + 1); p->n2 = (long long)p->G * (len + 1); p->nk = (long long)p->G * NT;
    long long off = 0;
    auto take = [&](long long rows, long long width) { const T r = buffer(off, rows, width); off += (rows * width + 3) / 4 * 4; return r; };
    auto stage = [&](StageT<T>* s, int layers, long long tokens, long long n_seq, int S, int num_cls) {
        s->tokens = tokens; s->n_seq = (int)n_seq; s->S = S; s->num_cls = num_cls;
        s->L.resize(layers);
        for (auto& L : s->L) { L.x = take(tokens, D); L.qkv = take(tokens, 3 * D); L.att = take(tokens, D); L.x2 = take(tokens, D); L.hp = take(tokens, D); }
        s->out = take(tokens, D);
    };
    stage(&p->table, d.pos_layers, p->n1, p->nt, NT + 1, 1);
    stage(&p->temporal, d.first_layers, p->nt, p->G, len, 0);
    stage(&p->spin, d.second_layers, p->n2, p->G, len + 1, 1);
    // scratch of the layers (the table stage has the most rows), then the gradient streams
    p->tA = take(p->n1, D); p->tB = take(p->n1, D); p->tC = take(p->n1, D); p->tE = take(p->n1, D); p->dX = take(p->n1, D); p->dY = take(p->nt, D);
    p->tQ = take(p->n1, 3 * D);
    p->partial = take(kslices(p->n1), 3LL * D * D);          // the largest sliced product: the table stage's qkv weight
    p->ball_h = take(p->nt, D); p->ball_tok = take(p->nt, D); p->tab_h = take(p->nk, D); p->tab_tok = take(p->nk, D);
    p->pos_h1 = take(p->nt, D / 2); p->pos_h2 = take(p->nt, D / 4); p->rot_h1 = take(p->G, D / 2); p->rot_h2 = take(p->G, D / 4);
    p->m1 = take(p->nt, 1); p->m2 = take(p->n2, 1); p->tmask = take(p->G, NT + 1); p->txy = take(p->nk, 2);
    p->rope = take(p->nt, d.hd); p->rot_t = take(p->G, 3); p->d_rot = take(p->G, 3); p->d_pos = take(p->nt, 3);
    p->mask_sum = take(4, 1);
    p->total = off;
}

// ------------------------------------------------------------------ the attention kernels' launch
// P >= S threads per (sequence, head), P the smallest power of two >= max(16, S); below 64 a workgroup takes 64 / P sequences.
// LDS per sequence: k~ and v (backward: q~ and dO too) of S x hd, (backward) three statistics per row, the mask.
constexpr int ATTN_MAX_THREADS = 256;
constexpr size_t ATTN_MAX_LDS = 160 * 1024;
struct AttnGeom { int P, seqs, threads; size_t lds; bool ok; };
inline AttnGeom attn_geom(int S, int hd, bool bwd) {
    AttnGeom g;
    g.P = 16;
    while (g.P < S && g.P <= ATTN_MAX_THREADS) g.P *= 2;
    g.seqs = g.P >= 64 ? 1 : 64 / g.P;
    g.threads = g.seqs * g.P;
    g.lds = (size_t)g.seqs * ((size_t)(bwd ? 4 : 2) * S * hd + (bwd ? 3 * S : 0) + S) * sizeof(float);
    g.ok = S >= 1 && g.P <= ATTN_MAX_THREADS && g.lds <= ATTN_MAX_LDS && (hd == 8 || hd == 16 || hd == 24 || hd == 32);
    return g;
}
// whether the pass serves sequences of `len` time steps: its three stages run on n_table + 1, len and len + 1 tokens
inline bool grad_attention_served(const GradDims& d, int len) {
    for (int S : {d.n_table + 1, len, len + 1})
        if (S < 1 || !attn_geom(S, d.hd, false).ok || !attn_geom(S, d.hd, true).ok) return false;
    return true;
}

}  // namespace upl
}  // namespace ttup
