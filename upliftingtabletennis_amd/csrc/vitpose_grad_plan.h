// The ViTPose backbone's training pass without a device (csrc/vitpose_grad.hip): the table of the 149 backbone
// tensors (reference key suffix, shape, offset in one flat gradient buffer), the workspace the handle owns -- the activations every
// block keeps for the backward and the scratch both passes share --, the slices of every fixed-order sum, the launch geometry of the
// attention backward and the checks an argument list has to pass: functions of plain integers.  Standard headers, include/ttup.h,
// gemm_modes.h and vitpose_head_plan.h (SLICE_TOKENS) only: the same source compiles for gfx950 (hipcc) and for the host (g++:
// tests/helpers/host_vitpose_grad_plan.cpp).
#pragma once
#include "../../include/ttup.h"
#include "gemm_modes.h"
#include "vitpose_head_plan.h"
#include <stddef.h>
#include <stdio.h>
#include <string>
#include <vector>

namespace ttup {
namespace vgrad {

using namespace ttup::gemm;

constexpr int DIM = 384, HEADS = 12, HD = 32, MLP = 1536, DEPTH = 12, PATCH = 16;
constexpr int MAX_IN_CH = 16;                                   // in_ch * 256 columns of im2col a token: 1..16 input channels
constexpr long long MAX_ROWS = vhead::MAX_ROWS;                 // tokens a handle may be sized for (the head's bound: 2^22)
constexpr int BLOCK_TENSORS = 12, TENSORS = 3 + DEPTH * BLOCK_TENSORS + 2;
static_assert(TENSORS == TTUP_VITPOSE_BACKBONE_TENSORS, "include/ttup.h's pointer structs hold one pointer per table entry");

// ------------------------------------------------------------------ the gradient table
// The backbone's tensors in the reference's state_dict order, behind '<prefix>.backbone.'
enum BlockTensor { T_N1W, T_N1B, T_QKVW, T_QKVB, T_PROJW, T_PROJB, T_N2W, T_N2B, T_FC1W, T_FC1B, T_FC2W, T_FC2B };
enum { T_POS = 0, T_PATCHW = 1, T_PATCHB = 2, T_BLOCK0 = 3, T_LNW = T_BLOCK0 + DEPTH * BLOCK_TENSORS, T_LNB = T_LNW + 1 };
constexpr int block_tensor(int block, int t) { return T_BLOCK0 + block * BLOCK_TENSORS + t; }

struct GradTensor {
    std::string key;          // e.g. "blocks.3.attn.qkv.weight"
    int ndim;
    long long shape[4];
    size_t offset, count;     // floats in the flat gradient buffer
};
struct GradTable {
    std::vector<GradTensor> t;
    size_t total = 0;
};
inline GradTable grad_table(int in_ch, int ntok) {
    GradTable g;
    auto take = [&](const std::string& key, int ndim, long long a, long long b = 1, long long c = 1, long long d = 1) {
        GradTensor t{key, ndim, {a, b, c, d}, g.total, (size_t)(a * b * c * d)};
        g.total += t.count;
        g.t.push_back(t);
    };
    take("pos_embed", 3, 1, ntok + 1, DIM);
    take("patch_embed.proj.weight", 4, DIM, in_ch, PATCH, PATCH);
    take("patch_embed.proj.bias", 1, DIM);
    for (int i = 0; i < DEPTH; ++i) {
        const std::string p = "blocks." + std::to_string(i) + ".";
        take(p + "norm1.weight", 1, DIM); take(p + "norm1.bias", 1, DIM);
        take(p + "attn.qkv.weight", 2, 3 * DIM, DIM); take(p + "attn.qkv.bias", 1, 3 * DIM);
        take(p + "attn.proj.weight", 2, DIM, DIM); take(p + "attn.proj.bias", 1, DIM);
        take(p + "norm2.weight", 1, DIM); take(p + "norm2.bias", 1, DIM);
        take(p + "mlp.fc1.weight", 2, MLP, DIM); take(p + "mlp.fc1.bias", 1, MLP);
        take(p + "mlp.fc2.weight", 2, DIM, MLP); take(p + "mlp.fc2.bias", 1, DIM);
    }
    take("last_norm.weight", 1, DIM); take("last_norm.bias", 1, DIM);
    return g;
}

// ------------------------------------------------------------------ slices
// Every sum over tokens -- d gamma / d beta, the bias gradients, dpos[0] and the k range of the dW products -- is cut every
// SLICE_TOKENS tokens (the head's constant); slices are added in slice order.
using vhead::SLICE_TOKENS;
using vhead::slices;

// ------------------------------------------------------------------ the attention backward's launches
// attn_delta_kernel: one wave per 16 (row, head) pairs of one head, four waves a workgroup: grid (ceil(rows / 64), HEADS).
// attn_bwd_dkv_kernel: one workgroup per (key tile, head, sample) walking ceil(N / AQ) query tiles; attn_bwd_dq_kernel: one
// workgroup per (query tile, head, sample) walking ceil(N / AKV) key tiles.  256 threads each: 16 keys (queries) a wave.
constexpr int AQ = 64, AKV = 64, ASTR = HD + 4;
struct AttnGrid { unsigned x, y, z; int walk; };
constexpr AttnGrid attn_bwd_grid(int ntok, int batch) { return {(unsigned)((ntok + 63) / 64), (unsigned)HEADS, (unsigned)batch, (ntok + 63) / 64}; }
constexpr AttnGrid attn_delta_grid(long long rows) { return {(unsigned)((rows + 63) / 64), (unsigned)HEADS, 1u, 1}; }
constexpr size_t ATTN_BWD_LDS = (size_t)(2 * 64 * ASTR + 2 * 64) * 4;          // two 64 x 32 tiles (row stride 36) + lse and D of a query tile

// ------------------------------------------------------------------ refusals
struct Refusal {
    int rc = TTUP_OK;
    char msg[200] = "";
};
#define VG_PLAN_REQUIRE(cond, ...) do { if (!(cond)) { r.rc = TTUP_EINVAL; snprintf(r.msg, sizeof r.msg, __VA_ARGS__); return r; } } while (0)
inline Refusal check_create(int in_ch, int hp, int wp, int max_batch) {
    Refusal r;
    VG_PLAN_REQUIRE(in_ch >= 1 && in_ch <= MAX_IN_CH, "ttup_vitpose_grad_create: in_ch %d outside 1..%d", in_ch, MAX_IN_CH);
    VG_PLAN_REQUIRE(hp >= 1 && wp >= 1 && max_batch >= 1, "ttup_vitpose_grad_create: grid %dx%d and max_batch %d must be positive", hp, wp, max_batch);
    VG_PLAN_REQUIRE((long long)hp * wp <= MAX_ROWS && (long long)hp * wp * max_batch <= MAX_ROWS, "ttup_vitpose_grad_create: %d x %dx%d tokens, at most %lld",
                    max_batch, hp, wp, MAX_ROWS);
    return r;
}
// scale_len: the floats of drop_scale (0: none given)
inline Refusal check_forward(int max_batch, int batch, long long scale_len) {
    Refusal r;
    VG_PLAN_REQUIRE(batch >= 1 && batch <= max_batch, "ttup_vitpose_grad_forward: batch %d outside 1..%d", batch, max_batch);
    VG_PLAN_REQUIRE(scale_len == 0 || scale_len == (long long)DEPTH * 2 * batch, "ttup_vitpose_grad_forward: drop_scale has %lld floats, (12, 2, %d) has %d",
                    scale_len, batch, DEPTH * 2 * batch);
    return r;
}
// kept_batch: what the last forward ran on (0: none)
inline Refusal check_backward(int kept_batch, int batch) {
    Refusal r;
    VG_PLAN_REQUIRE(kept_batch > 0, "ttup_vitpose_grad_backward: no forward has run on this handle");
    VG_PLAN_REQUIRE(batch == kept_batch, "ttup_vitpose_grad_backward: batch %d, the forward ran batch %d", batch, kept_batch);
    return r;
}
#undef VG_PLAN_REQUIRE

// ------------------------------------------------------------------ the workspace
// One allocation per handle, for T = max_batch * tokens rows.
// Kept by the forward, one slot per block so that nothing is overwritten before the backward reads it (floats a token):
//   X     13 x 384   the residual stream entering block i (X[12]: what last_norm reads)
//   XMID  12 x 384   the stream between the two halves
//   ST1, ST2  12 x 2 each, STL 2   mean and rstd of norm1, norm2, last_norm
//   QKV   12 x 1152, LSE 12 x 12 (m + log l per head), ATT 12 x 384, PRE 12 x 1536 (fc1 before the GELU)
//   COL   in_ch x 256   im2col of the patch embedding (what its dW reads; the images themselves are the caller's)
// = 12 x 3856 + 386 + 256 in_ch floats: 186 632 bytes a token + 1 024 in_ch.  The LN outputs and gelu(fc1) are NOT kept (another
// 12 x (768 + 1536) floats, 110 592 bytes a token): they are recomputed into LN and HID before the product that reads them.
// Scratch, shared by both passes (floats a token): HID, DHID 1536 each; BR (a branch's output; s * g in the backward), LN, G (the
// stream's gradient), DLN (the gradient into an LN output; d att) 384 each; DQKV 1152; DELTA 12: 5 772 floats, 23 088 bytes.
// Sums: SUMS fp64 slices x 2 x 1536; PARTIAL slices x 384 x max(1536, 256 in_ch) floats, the k-slices of one dW product; SCALE
// 24 x max_batch floats.
enum Buf { B_X, B_XMID, B_ST1, B_ST2, B_STL, B_QKV, B_LSE, B_ATT, B_PRE, B_COL, B_HID, B_DHID, B_BR, B_LN, B_G, B_DLN, B_DQKV, B_DELTA, B_SUMS, B_PARTIAL,
           B_SCALE, B_COUNT };
constexpr size_t kept_floats_per_token(int in_ch) { return (size_t)DEPTH * (3 * DIM + 2 * 2 + 3 * DIM + HEADS + MLP) + DIM + 2 + (size_t)in_ch * 256; }
constexpr size_t scratch_floats_per_token() { return (size_t)2 * MLP + 4 * DIM + 3 * DIM + HEADS; }
constexpr size_t partial_cols(int in_ch) { return in_ch * 256 > MLP ? (size_t)in_ch * 256 : (size_t)MLP; }

struct Workspace {
    size_t off[B_COUNT] = {}, bytes[B_COUNT] = {};
    size_t total = 0;
};
// the alignment rules of vitpose_plan.h's plan_buffers: 256 bytes, and 2 MiB for a buffer of 2 MiB or more
constexpr size_t SMALL_ALIGN = 256, LARGE_ALIGN = 2u << 20;
inline Workspace plan_workspace(long long max_rows, int in_ch, int max_batch) {
    const size_t T = (size_t)max_rows, S = (size_t)slices(max_rows);
    Workspace w;
    auto take = [&](int b, size_t bytes) {
        w.bytes[b] = bytes;
        const size_t align = bytes >= LARGE_ALIGN ? LARGE_ALIGN : SMALL_ALIGN;
        w.off[b] = (w.total + align - 1) / align * align;
        w.total = w.off[b] + bytes;
    };
    take(B_X, (DEPTH + 1) * T * DIM * 4); take(B_XMID, DEPTH * T * DIM * 4);
    take(B_ST1, DEPTH * T * 2 * 4); take(B_ST2, DEPTH * T * 2 * 4); take(B_STL, T * 2 * 4);
    take(B_QKV, DEPTH * T * 3 * DIM * 4); take(B_LSE, DEPTH * T * HEADS * 4); take(B_ATT, DEPTH * T * DIM * 4); take(B_PRE, DEPTH * T * MLP * 4);
    take(B_COL, T * in_ch * 256 * 4);
    take(B_HID, T * MLP * 4); take(B_DHID, T * MLP * 4);
    take(B_BR, T * DIM * 4); take(B_LN, T * DIM * 4); take(B_G, T * DIM * 4); take(B_DLN, T * DIM * 4);
    take(B_DQKV, T * 3 * DIM * 4); take(B_DELTA, T * HEADS * 4);
    take(B_SUMS, S * 2 * MLP * 8);
    take(B_PARTIAL, S * DIM * partial_cols(in_ch) * 4);
    take(B_SCALE, (size_t)DEPTH * 2 * max_batch * 4);
    return w;
}

}  // namespace vgrad
}  // namespace ttup
