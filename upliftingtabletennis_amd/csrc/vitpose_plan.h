// The ViTPose detector's decisions without a device (csrc/vitpose.hip): the model constants, the weight blob's tensor table and the
// checks a blob has to pass, the micro-batch rule, the one arena the activations live in, the forward's GEMMs as a table, and the
// taps of the testing seam -- functions of plain integers.  Standard headers, include/ttup.h and gemm_modes.h only: the same source
// compiles for gfx950 (hipcc) and for the host (g++: tests/helpers/host_vitpose_plan.cpp checks the table against
// weights.pack_vitpose_blob, the refusals, the arena for alignment, overlap and sizing, and the taps against vitpose.TAPS).
#pragma once
#include "../../include/ttup.h"
#include "gemm_modes.h"
#include <stdio.h>
#include <string.h>
#include <vector>

namespace ttup {
namespace vit {

using namespace ttup::gemm;

constexpr int DIM = 384, HEADS = 12, HD = 32, MLP = 1536, DEC = 256, DEPTH = 12;
constexpr int STAGES = DEPTH + 2;          // ttup_vitpose_run_stage: 0 the patch embedding, 1..DEPTH the blocks, DEPTH + 1 the head
constexpr char MAGIC[9] = "TTUPVIT1";
constexpr size_t BLOB_HEADER = 8 + 8 * 4;  // magic, eight int32

// ------------------------------------------------------------------ the weight blob (include/ttup.h, weights.pack_vitpose_blob)
// float offsets behind the header; the device copy `weights` and its bf16 rounding `w16` share them
struct BlockOffsets { size_t n1w, n1b, qkvw, qkvb, projw, projb, n2w, n2b, fc1w, fc1b, fc2w, fc2b; };
struct BlobTensor { size_t offset, count; };
struct BlobLayout {
    size_t pos, patch_w, patch_b;
    BlockOffsets blk[DEPTH];
    size_t lnw, lnb, dc_w[2], dc_b[2], fin_w, fin_b;          // deconv l: w[4 phases][DEC][4 * cin], BN folded
    size_t total = 0;                                         // floats
    std::vector<BlobTensor> t;                                // the same tensors in blob order
};

inline BlobLayout blob_layout(int in_ch, int out_ch, int n_pos) {
    BlobLayout L;
    auto take = [&](size_t count) { L.t.push_back({L.total, count}); L.total += count; return L.t.back().offset; };
    L.pos = take((size_t)n_pos * DIM); L.patch_w = take((size_t)DIM * in_ch * 256); L.patch_b = take(DIM);
    for (BlockOffsets& b : L.blk) {
        b.n1w = take(DIM); b.n1b = take(DIM); b.qkvw = take((size_t)3 * DIM * DIM); b.qkvb = take(3 * DIM); b.projw = take((size_t)DIM * DIM); b.projb = take(DIM);
        b.n2w = take(DIM); b.n2b = take(DIM); b.fc1w = take((size_t)MLP * DIM); b.fc1b = take(MLP); b.fc2w = take((size_t)DIM * MLP); b.fc2b = take(DIM);
    }
    L.lnw = take(DIM); L.lnb = take(DIM);
    L.dc_w[0] = take((size_t)4 * DEC * 4 * DIM); L.dc_b[0] = take(DEC); L.dc_w[1] = take((size_t)4 * DEC * 4 * DEC); L.dc_b[1] = take(DEC);
    L.fin_w = take((size_t)out_ch * DEC); L.fin_b = take(out_ch);
    return L;
}

struct Refusal {
    int rc = TTUP_OK;
    char msg[256] = "";          // for ttup_last_error when rc != TTUP_OK
};

// Whether ttup_vitpose_create takes these sizes and this blob: TTUP_EINVAL for the arguments, TTUP_EFORMAT for the blob
inline Refusal check_create(const void* blob, size_t blob_bytes, int height, int width, int max_batch, int micro_batch, int in_ch, int out_ch) {
    Refusal r;
#define VP_PLAN_REQUIRE(cond, code, ...) do { if (!(cond)) { r.rc = code; snprintf(r.msg, sizeof r.msg, __VA_ARGS__); return r; } } while (0)
    VP_PLAN_REQUIRE(height >= 16 && width >= 16 && height % 16 == 0 && width % 16 == 0, TTUP_EINVAL,
                    "ttup_vitpose_create: height and width must be positive multiples of 16 (got %dx%d)", height, width);
    VP_PLAN_REQUIRE(max_batch >= 1 && micro_batch >= 0 && in_ch >= 1 && out_ch >= 1 && out_ch <= 16, TTUP_EINVAL,
                    "ttup_vitpose_create: bad max_batch %d / micro_batch %d / in_ch %d / out_ch %d (1..16)", max_batch, micro_batch, in_ch, out_ch);
    const int ntok = (height / 16) * (width / 16);
    VP_PLAN_REQUIRE(blob_bytes >= BLOB_HEADER && memcmp(blob, MAGIC, 8) == 0, TTUP_EFORMAT, "ttup_vitpose_create: not a ViTPose blob");
    int hdr[8];
    memcpy(hdr, (const char*)blob + 8, sizeof hdr);
    VP_PLAN_REQUIRE(hdr[0] == in_ch && hdr[1] == out_ch, TTUP_EFORMAT, "ttup_vitpose_create: blob has in_ch %d / out_ch %d, asked for %d / %d",
                    hdr[0], hdr[1], in_ch, out_ch);
    VP_PLAN_REQUIRE(hdr[2] == DIM && hdr[3] == DEPTH && hdr[4] == HEADS && hdr[5] == MLP && hdr[6] == DEC, TTUP_EFORMAT,
                    "ttup_vitpose_create: only ViTPose-small (384 / 12 / 12 / 1536 / 256) is built");
    VP_PLAN_REQUIRE(hdr[7] == ntok + 1, TTUP_EFORMAT, "ttup_vitpose_create: pos_embed has %d rows, a %dx%d input needs %d", hdr[7], height, width, ntok + 1);
    const size_t want = BLOB_HEADER + blob_layout(in_ch, out_ch, ntok + 1).total * 4;
    VP_PLAN_REQUIRE(blob_bytes == want, TTUP_EFORMAT, "ttup_vitpose_create: blob has %zu bytes, expected %zu", blob_bytes, want);
#undef VP_PLAN_REQUIRE
    return r;
}

// samples per internal pass: what was asked for, else 8, and never more than max_batch
inline int micro_batch(int max_batch, int requested) {
    const int m = requested ? requested : 8;
    return m < max_batch ? m : max_batch;
}

// ------------------------------------------------------------------ the arena
// B_X .. B_WS are cut from one allocation; x_attn is allocated on first use (run_stage), B_IN is the caller's input
enum Buf { B_X, B_STATS, B_STATS64, B_QKV, B_ATT, B_HID, B_D2, B_HEAT, B_FRAMES, B_WS, B_ARENA, B_XATTN = B_ARENA, B_IN, B_COUNT };

// bytes per element of a buffer: the residual stream, the fp32 statistics, the heatmap and the frame records are fp32 on either path,
// the stored activations bf16 on a bf16 handle (dtype 1)
constexpr size_t elem_size(int buf, int dtype) {
    return buf == B_STATS64 ? 8 : (buf == B_QKV || buf == B_ATT || buf == B_HID || buf == B_D2) && dtype == 1 ? 2 : 4;
}

struct BufferPlan {
    size_t off[B_ARENA] = {}, bytes[B_ARENA] = {};          // bytes 0: the handle has no such buffer
    size_t total = 0;
};

// One micro-batch's activations: stats64 on a bf16 handle only, frames (the fp32 (3, H, W) records of forward_frames: one micro-batch
// of samples spans micro + in_ch / 3 - 1 frames) where a sample is a whole number of frames, refine_bytes of argmax workspace.
// Every buffer starts on a 256-byte boundary, and one of 2 MiB or more on a 2 MiB boundary, where an allocation of its own would put
// it: packed at 256 bytes the forward measured 0.2 - 0.3 % slower.
constexpr size_t SMALL_ALIGN = 256, LARGE_ALIGN = 2u << 20;
inline BufferPlan plan_buffers(int height, int width, int in_ch, int out_ch, int micro, int dtype, size_t refine_bytes) {
    const size_t M = (size_t)micro * (height / 16) * (width / 16);
    BufferPlan p;
    auto take = [&](int b, size_t count) {
        p.bytes[b] = count * elem_size(b, dtype);
        const size_t align = p.bytes[b] >= LARGE_ALIGN ? LARGE_ALIGN : SMALL_ALIGN;
        p.off[b] = (p.total + align - 1) / align * align;
        p.total = p.off[b] + p.bytes[b];
    };
    take(B_X, M * DIM);
    take(B_STATS, M * 2);
    if (dtype == 1) take(B_STATS64, M * 2);
    take(B_QKV, M * 3 * DIM);
    take(B_ATT, M * DIM);
    take(B_HID, M * MLP);
    take(B_D2, M * 16 * DEC);
    take(B_HEAT, M * 16 * out_ch);
    if (in_ch % 3 == 0) take(B_FRAMES, (size_t)(micro + in_ch / 3 - 1) * 3 * height * width);
    take(B_WS, (refine_bytes + 3) / 4);
    return p;
}

// ------------------------------------------------------------------ the forward's GEMMs
// M = m_per_token * batch * tokens rows; the output has out_per_token rows of N per token (a deconvolution phase writes every
// second pixel of every second row of a map twice the size of its input).  K 0: in_ch * 256.  Where bf16_out, a bf16 handle stores
// the output as bf16.  An E_RESID GEMM adds its own output buffer (the residual stream).
enum GemmId { G_PATCH, G_QKV, G_PROJ, G_FC1, G_FC2, G_LAST_NORM, G_DECONV1, G_DECONV2, G_COUNT };
struct GemmSpec { int am, m_per_token, N, K, flags, in, out, out_per_token; bool bf16_out; };
constexpr GemmSpec GEMMS[G_COUNT] = {
    {A_PATCH, 1, DIM, 0, E_POS, B_IN, B_X, 1, false},          // A_PATCH_FRAMES in forward_frames
    {A_LN, 1, 3 * DIM, DIM, 0, B_X, B_QKV, 1, true},
    {A_DENSE, 1, DIM, DIM, E_RESID, B_ATT, B_X, 1, false},
    {A_LN, 1, MLP, DIM, E_GELU, B_X, B_HID, 1, true},
    {A_DENSE, 1, DIM, MLP, E_RESID, B_HID, B_X, 1, false},
    {A_LN, 1, DIM, DIM, 0, B_X, B_ATT, 1, true},               // last_norm alone (ln_apply): no product, the same operand form
    {A_DECONV, 1, DEC, 4 * DIM, E_RELU, B_ATT, B_HID, 4, true},
    {A_DECONV, 4, DEC, 4 * DEC, E_RELU, B_HID, B_D2, 16, true},
};
constexpr bool gemms_fit_tiles() {
    for (const GemmSpec& g : GEMMS) {
        const int K = g.K ? g.K : 256;          // any in_ch
        if (g.N % BN || K % BK || g.N % gemm16::TN || K % gemm16::TK) return false;
    }
    return true;
}
static_assert(gemms_fit_tiles(), "a ViTPose GEMM's N or K is not a whole number of tiles of gemm_kernel or gemm_bf16_kernel");

// ------------------------------------------------------------------ the taps of ttup_vitpose_read_tap
// written by stages first..last; `cols` per token (0: the heatmap, 16 * out_ch); bf16 on a bf16 handle as its buffer is
struct Tap { const char* name; int first, last, buf, cols; };
constexpr Tap TAPS[] = {
    {"x_attn", 1, DEPTH, B_XATTN, DIM}, {"x", 0, DEPTH, B_X, DIM}, {"qkv", 1, DEPTH, B_QKV, 3 * DIM}, {"att", 1, DEPTH, B_ATT, DIM},
    {"hid", 1, DEPTH, B_HID, MLP}, {"ln", DEPTH + 1, DEPTH + 1, B_ATT, DIM}, {"d1", DEPTH + 1, DEPTH + 1, B_HID, 4 * DEC},
    {"d2", DEPTH + 1, DEPTH + 1, B_D2, 16 * DEC}, {"heat", DEPTH + 1, DEPTH + 1, B_HEAT, 0},
};

}  // namespace vit
}  // namespace ttup
