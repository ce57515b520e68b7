// Fused BasicBlock chains: one 3x3 conv of a chain (bb_conv), the one-block chain and the run-time-epilogue two-block chain.
#pragma once
#include "conv_dev.h"
#include "conv.h"

namespace ttup {

// ------------------------------------------------------------------ fused BasicBlock chains
// One or two BasicBlocks (wasb.py:48-64: conv3x3+BN+ReLU, conv3x3+BN, +x, ReLU) of one HRNet branch in ONE kernel.
// The input tile with a halo of 2 pixels per block is staged once; every intermediate (rounded to bf16 exactly like the unfused
// path, and zeroed outside the image so that each conv sees its own zero padding) lives in LDS; only the final
// TH x TW tile is written.  HBM traffic per block chain: one read + one write of the tensor instead of 5 passes per block.
// Each wave keeps the conv's A fragments (weights) in registers and walks 16-pixel groups of the output region
// (linear pixel index, so ragged region widths waste nothing).
struct BBArgs {
    const bf16_t* x = nullptr; bf16_t* y = nullptr;
    const bf16_t* w[4] = {}; const float* bias[4] = {};
    int H = 0, W = 0, tiles_x = 0, tiles_per_img = 0, total_tiles = 0;
    // optional 1x1 follower on the chain output (C=32 -> 16, BN folded, no ReLU: the fuse-layer conv of wasb.py:189-205 that
    // feeds the higher-resolution branch): one extra MFMA per 16-pixel group on the bf16 pairs just packed
    const bf16_t* wf = nullptr; const float* bf = nullptr; bf16_t* yf = nullptr;
    // C=16 two-block chain at full resolution: the fuse-layer sum that consumes the branch (wasb.py:236-243) rides in the last
    // conv's epilogue: ysum = relu(y + sum_k up(st[k], 2^ssh[k])).  With `heat` set the sum is the stage-4 output: it is not
    // stored at all, the 1x1 head (final_layers[0] channel 1, wasb.py:484,606) is applied to it in registers and the workgroup
    // leaves its argmax partial (pv/pi[map * nblk + tile]); y itself (the pre-fuse branch tensor) is only stored when a.y is set.
    const bf16_t* st[3] = {}; int ssh[3] = {}; int nsum = 0; bf16_t* ysum = nullptr;
    float* heat = nullptr; const float* hw = nullptr; float hbias = 0.f; float* pv = nullptr; long long* pi = nullptr;
};
// the tile's slices of the fuse-layer terms staged in LDS by the chain kernel (element offset of term k, pixels per row); a
// separate by-value struct: writing into the kernel-argument struct would move all of it to scratch memory
struct BBTermLds { const bf16_t* s_terms; int toff[3]; int tw[3]; };

// ReLU on the sign bit (one integer max, like relu_pk on bf16 pairs): negative values and -0 become +0, +NaN stays NaN
__device__ __forceinline__ float relu_f32(float v) { const int b = __float_as_int(v); return __int_as_float(b > 0 ? b : 0); }
struct BBBest { float v; long long i; };
__device__ __forceinline__ bool bb_better(float v, long long i, float bv, long long bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn || bn) return vn && (!bn || i < bi);
    return v > bv || (v == bv && i < bi);
}

// (value, index) as one unsigned key: greater key = greater value (NaN greatest, -0 == +0), then lower index (index < 2^31)
__device__ __forceinline__ unsigned long long bb_key(float v, int e) {
    v += 0.0f;                                              // -0 -> +0
    const unsigned bits = __float_as_uint(v);
    unsigned k = bits ^ ((unsigned)((int)bits >> 31) | 0x80000000u);
    if (v != v) k = 0xffffffffu;
    return ((unsigned long long)k << 32) | (unsigned)(~e);
}
__device__ __forceinline__ float bb_key_value(unsigned long long key) {
    const unsigned k = (unsigned)(key >> 32);
    if (k == 0xffffffffu) return __uint_as_float(0x7fc00000u);
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// lane i <- lane i + n of the same 16-lane row (0 where that lane does not exist): DPP row_shl, no LDS traffic
__device__ __forceinline__ unsigned long long bb_dpp_shl(unsigned long long x, int n) {
    unsigned lo = (unsigned)x, hi = (unsigned)(x >> 32);
    switch (n) {
        case 8: lo = __builtin_amdgcn_update_dpp(0, lo, 0x108, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0x108, 0xf, 0xf, false); break;
        case 4: lo = __builtin_amdgcn_update_dpp(0, lo, 0x104, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0x104, 0xf, 0xf, false); break;
        case 2: lo = __builtin_amdgcn_update_dpp(0, lo, 0x102, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0x102, 0xf, 0xf, false); break;
        default: lo = __builtin_amdgcn_update_dpp(0, lo, 0x101, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(0, hi, 0x101, 0xf, 0xf, false); break;
    }
    return ((unsigned long long)hi << 32) | lo;
}

// element offset of 8-channel chunk c8 of the pixel at buffer column x (pix = row*stride + x); C=32 swizzles the chunk
// with bits 1..2 of the column (conflict-free ds_read_b128, see lds_off).  C=16 (32 B per pixel) flips the two chunks with
// bit 2 of the column: the ds_read_b128 fragments of a band group stay conflict-free (columns x and x+8 of a hardware lane group
// carry different chunks either way) and the epilogue's 8-byte stores, 16 lanes at a 32-byte stride, are 2-way instead of 4-way.
// (History of SQ_LDS_BANK_CONFLICT per launch of the two-block chain: 22 % of its LDS cycles before this swizzle, 6.45e6 = 10 %
// with it in round 2, 1.38e7 = 22 % again in round 3 when the ragged strips were packed row-major across aliasing rows, and back
// down with odd row strides + column strip groups in round 4: profiles/r4_pmc_summary.txt.)
template <int C> __device__ __forceinline__ int bb_off(int pix, int x, int c8) {
    if (C == 32) return pix * 32 + ((c8 ^ ((x >> 1) & 3)) << 3);
    return pix * C + ((c8 ^ ((x >> 2) & 1)) << 3);
}

// Weight fragments + bias of one 16-channel conv, loaded by the CALLER: the chain kernel requests the next conv's fragments from
// L2 before the barrier that ends the current conv, so their latency (the first MFMA of a conv needs all of them) hides behind
// the barrier wait instead of following it.
struct BBFrag16 { bf16x8 af[5]; f32x4 bias; };
// A fragment of the 16x16 identity for lanes g >= 2 (row n, columns (g & 1) * 8 .. + 7): the residual add of a block's second
// conv rides in the unused half of its last k-step.  Built once per kernel (it costs ~35 vector instructions).
__device__ __forceinline__ bf16x8 bb_identity_frag(int lane) {
    const int n = lane & 15, g = lane >> 4;
    unsigned short idm[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) idm[j] = (n == (g & 1) * 8 + j) ? 0x3F80 : 0;
    return __builtin_bit_cast(bf16x8, idm);
}
// K order of the 16-channel chain convs (two taps per k-step, first tap on lane groups 0-1, second on 2-3):
//   (0,0)|(0,1)   (1,0)|(1,1)   (2,0)|(2,1)   (0,2)|(1,2)   (2,2)|pad
// so that the pixel fragment of the first three steps depends on the input row only (row y+dy, columns x | x+1): a wave walking
// consecutive output rows reads it once for three rows, and the fourth step's fragment (column x+2 of rows r | r+1) doubles as
// the fifth step of the row two above.  The weights stay in the standard packing (taps 2s | 2s+1 per step): tap t of lane group
// half c8 is at step t/2, lane group 2(t&1) + c8 -- a gather at load time, no second packing.
__device__ __forceinline__ int bb_tap16(int s, int h) {          // tap of k-step s, half h (9 = the zero pad)
    return s < 3 ? 3 * s + h : (s == 3 ? (h ? 5 : 2) : (h ? 9 : 8));
}
__device__ __forceinline__ bf16x8 bb_weight_frag16(const bf16_t* wfrag, int s, int lane) {
    const int i = lane & 15, g = lane >> 4, tap = bb_tap16(s, g >> 1);
    return *(const bf16x8*)(wfrag + ((tap >> 1) * 64 + i + 16 * (2 * (tap & 1) + (g & 1))) * 8);
}
__device__ __forceinline__ void bb_load_frag16(BBFrag16& f, const bf16_t* wfrag, const float* biasp, int lane) {
#pragma unroll
    for (int s = 0; s < 5; ++s) f.af[s] = bb_weight_frag16(wfrag, s, lane);
    f.bias = *(const f32x4*)(biasp + (lane >> 4) * 4);
}

// One 3x3 conv of the chain.  Input buffer: row stride RWI pixels, region origin at (IOFF,IOFF).  Output region RHO x RWO.
// SECOND: second conv of a BasicBlock -> adds the block input (buffer s_res, row stride RWR, origin offset ROFF) and the
// result either overwrites that buffer in place (ORW = RWR, OOFF = ROFF: each pixel is read and written by the same lane)
// or goes to global memory.  A wave owns whole output rows (y = wave, wave+8, ...); the 16-pixel groups of a row are
// unrolled so every LDS address is a per-lane base plus an immediate.
// The last conv of the C=16 chain reads its fuse-sum / head configuration from BBArgs at run time here; the forms the network uses are
// compiled out in csrc/chain16.h (c16_chain_kernel), this one is the fallback for other term layouts and the cross-check of those.
template <int R> struct BBRow { static constexpr int value = R; };
// NWV (C=32 only): waves that share the conv's rows -- `wave` is the wave's index among them (rows wave, wave + NWV, ...).  af32: the C=32
// conv's 18 weight fragments already in registers (a two-group variant kept them there for the life of the workgroup: git show d528471:upliftingtabletennis_amd/csrc/experiments/rejected_kernels.hip.inc).
template <int C, int RWI, int IOFF, int RHO, int RWO, bool SECOND, int RWR, int ROFF, bool GLOBAL_OUT, int ORW, int OOFF, int NWV = 8>
__device__ __forceinline__ void bb_conv(const bf16_t* s_in, bf16_t* s_out, const bf16_t* s_res, const bf16_t* wfrag, const float* biasp,
                                        bf16_t* gout, int gy0, int gx0, int H, int W, int b, int wave, int lane,
                                        const bf16_t* wf = nullptr, const float* bfp = nullptr, bf16_t* yf = nullptr,
                                        const BBArgs* ex = nullptr, BBBest* best = nullptr, const BBFrag16* pre = nullptr,
                                        const BBTermLds* tl = nullptr, bf16x8 idm_pre = bf16x8{}, const bf16x8* af32 = nullptr) {
    constexpr int MT = C / 16;
    constexpr int KSTEPS = (C == 16) ? 5 : 9;
    constexpr int XT = (RWO + 15) / 16;
    static_assert(NWV == 8 || C == 32, "only the 32-channel row loop takes a wave count");
    const int n = lane & 15, g = lane >> 4;
    bf16x8 af[KSTEPS][MT];
    if (C == 32 && af32) {
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
            for (int m = 0; m < MT; ++m) af[s][m] = af32[s * MT + m];
    } else if (C == 16 && pre) {
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) af[s][0] = pre->af[s < 5 ? s : 4];
    } else {
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
            for (int m = 0; m < MT; ++m) af[s][m] = (C == 16) ? bb_weight_frag16(wfrag, s < 5 ? s : 4, lane) : *(const bf16x8*)(wfrag + ((s * MT + m) * 64 + lane) * 8);
    }
    // C=16, second conv of a block: the unused tenth tap of the last k-step (lanes g >= 2, zero weights) carries the block
    // input through an identity matrix, so the residual add happens inside the MFMA (exact: bf16 * 1.0 into the fp32 sum)
    constexpr bool RES_MFMA = SECOND && C == 16;
    if (RES_MFMA && g >= 2) af[KSTEPS - 1][0] = pre ? idm_pre : bb_identity_frag(lane);      // (by value: a field of *pre would pin the struct in memory)
    f32x4 bias[MT];
    if (C == 16 && pre) bias[0] = pre->bias;
    else {
#pragma unroll
        for (int m = 0; m < MT; ++m) bias[m] = *(const f32x4*)(biasp + g * 4 * MT + m * 4);
    }
    int koff[KSTEPS];                     // C=32: per-lane tap/channel offset of every k-step (elements); k-step s = tap (s/3, s%3)
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
        const int dy = s / 3, dx = s % 3;
        // the column swizzle depends only on (n + dx + IOFF) mod 8: 16-pixel groups start at multiples of 16
        koff[s] = (dy * RWI + dx) * C + ((g ^ (((n + dx + IOFF) >> 1) & 3)) << 3);
    }
    // lane's pixel in the last (possibly ragged) group is clamped so that reads stay inside the buffer
    constexpr int XLAST = (XT - 1) * 16;
    const int nl = (XLAST + n < RWO) ? n : (RWO - 1 - XLAST);
    // lane's first output channel inside its pixel record (chunk g for C=32, chunk g>>1 + half g&1 for C=16; swizzled like bb_off)
    const int res_ch = (C == 32) ? ((g ^ (((n + ROFF) >> 1) & 3)) << 3) : ((((g >> 1) ^ (((n + ROFF) >> 2) & 1)) << 3) + (g & 1) * 4);
    const int out_ch = (C == 32) ? ((g ^ (((n + OOFF) >> 1) & 3)) << 3) : ((((g >> 1) ^ (((n + OOFF) >> 2) & 1)) << 3) + (g & 1) * 4);
    // zero padding of the next conv: outputs outside the image must be 0; only border tiles have any (wave-uniform test)
    const bool interior = gy0 >= 0 && gy0 + RHO <= H && gx0 >= 0 && gx0 + RWO <= W;
    constexpr bool CAN_FOLLOW = GLOBAL_OUT && C == 32;
    bf16x8 af_f = {};
    f32x4 bias_f = {0.f, 0.f, 0.f, 0.f};
    if (CAN_FOLLOW && yf) { af_f = *(const bf16x8*)(wf + lane * 8); bias_f = *(const f32x4*)(bfp + g * 4); }
    constexpr bool CAN_SUM = GLOBAL_OUT && C == 16;
    f32x4 hw4 = {0.f, 0.f, 0.f, 0.f};
    if (CAN_SUM && ex && ex->heat) hw4 = *(const f32x4*)(ex->hw + g * 4);
    // C=16: a wave owns a BAND of consecutive output rows (pixel fragments shared between them, see bb_tap16); C=32: rows
    // wave, wave+8, ... (two output tiles per fragment read already)
    constexpr bool BAND = (C == 16);
    constexpr int RB = (RHO + 7) / 8;
    const int yb = BAND ? wave * RB : wave;      // the wave's first row
    // C=32: per-lane fragment addresses of the wave's FIRST row, one per k-step (full groups / clamped last group); the row loop is
    // fully unrolled, so the rows that follow are compile-time offsets (LDS instruction immediates) from them instead of a
    // dozen address registers that each need an add per row.  (C=16 sets up its band addresses below.)
    const bf16_t* pk0[KSTEPS];
    const bf16_t* pkl[KSTEPS];
    {
        const bf16_t* row0 = s_in + ((wave + IOFF) * RWI + IOFF) * C;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) { pk0[s] = row0 + n * C + koff[s]; pkl[s] = row0 + (XLAST + nl) * C + koff[s]; }
    }
    constexpr int ROWSTEP = NWV * RWI * C;
    bf16_t* const so0 = GLOBAL_OUT ? nullptr : s_out + ((yb + OOFF) * ORW + n + OOFF) * C + out_ch;      // lane's output slot in the wave's first row
    // global stores: wave-uniform row base (scalar registers) + the lane's byte offset inside a 16-pixel group (one register for C-channel
    // records, one for 16-channel records) + the group as an immediate -- instead of a 64-bit per-lane address chain per store
    const unsigned st_c = (unsigned)((n * C + g * 4 * MT) * 2), st_16 = (unsigned)((n * 16 + g * 4) * 2);
    // epilogue of one 16-pixel group of row y (orow = its row offset from the wave's first row): bias/ReLU/rounding, zero padding
    // of the next conv, stores, and whatever rides in the last conv's epilogue
    auto epi = [&](int xt, int orow, int y, const f32x4 (&accx)[MT]) __attribute__((always_inline)) {
        const int gy = gy0 + y;
        const bool row_in = gy >= 0 && gy < H;
        const int x = xt * 16 + n;
        const bool valid = !(xt == XT - 1 && x >= RWO);       // ragged last group: computed (the follower MFMA needs the whole wave), not stored
        float v[4 * MT];
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[m * 4 + r] = accx[m][r];
        if (SECOND && !RES_MFMA) {       // + block input; the lane's 4*MT channels start at g*4*MT
            const bf16_t* rp = s_res + ((yb + ROFF) * RWR + n + ROFF) * C + res_ch + (orow * RWR + xt * 16) * C;
            add_bf16x8(v, *(const u32x4*)rp);
        }
        unsigned pk[2 * MT];
#pragma unroll
        for (int i = 0; i < 2 * MT; ++i) pk[i] = relu_pk(pack2(v[2 * i], v[2 * i + 1]));
        const int gx = gx0 + x;
        bool inside = true;
        if (!interior) {
            inside = row_in && gx >= 0 && gx < W;
#pragma unroll
            for (int i = 0; i < 2 * MT; ++i) pk[i] = inside ? pk[i] : 0u;
        }
        const size_t rowpix = (size_t)(b * H + gy) * W + gx0;          // (wave-uniform) first pixel of the region's row in the image
        if (GLOBAL_OUT) {
            if (inside && valid && gout) {
                char* o = (char*)(gout + rowpix * C) + (opaque_u32(st_c) + (unsigned)(xt * 16 * C * 2));
                if (C == 16) *(u32x2*)o = u32x2{pk[0], pk[1]};
                else *(u32x4*)o = u32x4{pk[0], pk[1], pk[2], pk[3]};
            }
            if constexpr (CAN_SUM) {
                if (ex && (ex->nsum > 0 || ex->heat)) {
                    // fuse-layer sum on the rounded block output, exactly what the element-wise pass read back from memory
                    float ys[4] = {bf16_to_f32((bf16_t)(pk[0] & 0xffff)), bf16_to_f32((bf16_t)(pk[0] >> 16)),
                                   bf16_to_f32((bf16_t)(pk[1] & 0xffff)), bf16_to_f32((bf16_t)(pk[1] >> 16))};
                    // stage-4 tail: neither the branch tensor nor the sum is stored, so neither is rounded to bf16 -- the head
                    // sees the fp32 values (two roundings fewer right in front of the heatmap: a smaller bf16-path error)
                    const bool exact_tail = ex->heat && !gout && !ex->ysum;
                    if (exact_tail) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) ys[r] = v[r] > 0.f ? v[r] : 0.f;
                    }
                    const bool live = inside && valid;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (k >= ex->nsum) continue;
                        // the tile's slice of term k sits in LDS (staged during the previous conv): no memory round trip here
                        const int sh = ex->ssh[k];
                        const u32x2 tv = *(const u32x2*)(tl->s_terms + tl->toff[k] + ((((gy0 + y) >> sh) - (gy0 >> sh)) * tl->tw[k] + ((gx >> sh) - (gx0 >> sh))) * 16 + g * 4);
                        ys[0] += bf16_to_f32((bf16_t)(tv.x & 0xffff)); ys[1] += bf16_to_f32((bf16_t)(tv.x >> 16));
                        ys[2] += bf16_to_f32((bf16_t)(tv.y & 0xffff)); ys[3] += bf16_to_f32((bf16_t)(tv.y >> 16));
                    }
                    const unsigned q0 = relu_pk(pack2(ys[0], ys[1])), q1 = relu_pk(pack2(ys[2], ys[3]));
                    if (ex->ysum && live) *(u32x2*)(ex->ysum + ((size_t)(b * H + gy) * W + gx) * 16 + g * 4) = u32x2{q0, q1};
                    if (ex->heat) {
                        // head on the bf16-rounded sum: this lane's 4 channels, then across the 4 lane groups of the pixel
                        float hy[4] = {bf16_to_f32((bf16_t)(q0 & 0xffff)), bf16_to_f32((bf16_t)(q0 >> 16)),
                                       bf16_to_f32((bf16_t)(q1 & 0xffff)), bf16_to_f32((bf16_t)(q1 >> 16))};
                        if (exact_tail) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) hy[r] = ys[r] > 0.f ? ys[r] : 0.f;
                        }
                        float part = hy[0] * hw4[0];
                        part = fmaf(hy[1], hw4[1], part);
                        part = fmaf(hy[2], hw4[2], part);
                        part = fmaf(hy[3], hw4[3], part);
                        part += __shfl_xor(part, 16, 64);
                        part += __shfl_xor(part, 32, 64);
                        const float hv = part + ex->hbias;
                        if (live && g == 0) {
                            const long long e = (long long)gy * W + gx;
                            ex->heat[(size_t)b * H * W + e] = hv;
                            if (bb_better(hv, e, best->v, best->i)) { best->v = hv; best->i = e; }
                        }
                    }
                }
            }
            if constexpr (CAN_FOLLOW) {
                if (yf) {          // lane (n, g) holds channels 8g..8g+7 of its pixel = k-group g of the follower's only k-step
                    const u32x4 bq = u32x4{pk[0], pk[1], pk[2], pk[3]};
                    const f32x4 cf = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af_f, __builtin_bit_cast(bf16x8, bq), bias_f, 0, 0, 0);
                    if (inside && valid) *(u32x2*)((char*)(yf + rowpix * 16) + (opaque_u32(st_16) + (unsigned)(xt * 16 * 32))) = u32x2{pack2(cf[0], cf[1]), pack2(cf[2], cf[3])};
                }
            }
        } else if (valid) {
            bf16_t* o = so0 + (orow * ORW + xt * 16) * C;
            if (C == 16) *(u32x2*)o = u32x2{pk[0], pk[1]};
            else *(u32x4*)o = u32x4{pk[0], pk[1], pk[2], pk[3]};
        }
    };
    if constexpr (!BAND) {
        // (the run-time epilogue form, MODE 0 with the fuse sum, is a cross-check path and stays rolled: unrolled it spills)
        constexpr int ROW_UNROLL = (RHO + NWV - 1) / NWV;
#pragma unroll ROW_UNROLL
        for (int yj = 0; yj < (RHO + NWV - 1) / NWV; ++yj) {
            const int y = wave + NWV * yj;
            if (y >= RHO) break;
            f32x4 acc[XT][MT];
#pragma unroll
            for (int xt = 0; xt < XT; ++xt)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[xt][m] = bias[m];
            // pipelined (see conv64_tile_mfma): the pixel fragments of k-step s+1 are requested before the MFMAs of step s
            bf16x8 bfr[2][XT];
            auto load_step = [&](int s, bf16x8 (&bf)[XT]) __attribute__((always_inline)) {
#pragma unroll
                for (int xt = 0; xt < XT; ++xt)
                    bf[xt] = (xt < XT - 1) ? *(const bf16x8*)(pk0[s] + yj * ROWSTEP + xt * 16 * C) : *(const bf16x8*)(pkl[s] + yj * ROWSTEP);
            };
            load_step(0, bfr[0]);
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) {
                if (s + 1 < KSTEPS) load_step(s + 1, bfr[(s + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int xt = 0; xt < XT; ++xt)
#pragma unroll
                    for (int m = 0; m < MT; ++m) acc[xt][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[s][m], bfr[s & 1][xt], acc[xt][m], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int xt = 0; xt < XT; ++xt) epi(xt, NWV * yj, y, acc[xt]);
        }
    } else {
        const int h = g >> 1, c8 = g & 1;
        constexpr int RS = RWI * C;                                   // one input row (elements)
        constexpr bool RAGGED = RWO % 16 != 0;
        // element offset of the lane's 8-channel chunk of the pixel dx columns right of output pixel nn (swizzle as in bb_off)
        auto lane_off = [&](int nn, int dx) { return (nn + dx) * C + ((c8 ^ (((nn + dx + IOFF) >> 2) & 1)) << 3); };
        const bf16_t* rowb = s_in + ((yb + IOFF) * RWI + IOFF) * C;
        const bf16_t* pA = rowb + lane_off(n, h);                      // steps 0-2: row r + dy, column x | x+1
        const bf16_t* pAl = rowb + XLAST * C + lane_off(nl, h);
        const bf16_t* pC = rowb + h * RS + lane_off(n, 2);             // step 3: column x+2 of rows r | r+1
        const bf16_t* pCl = rowb + XLAST * C + h * RS + lane_off(nl, 2);
        // step 4: pixel (r+2, x+2) on the first half; second half: the block input at the output pixel (second conv of a block,
        // identity weights) or the same pixel again (zero weights)
        const bf16_t* pD = rowb + 2 * RS + lane_off(n, 2);
        const bf16_t* pDl = rowb + XLAST * C + 2 * RS + lane_off(nl, 2);
        int dstep = RS;
        if (RES_MFMA && h) {
            const bf16_t* rr = s_res + ((yb + ROFF) * RWR + ROFF) * C;
            pD = rr + n * C + ((c8 ^ (((n + ROFF) >> 2) & 1)) << 3);
            pDl = rr + (XLAST + nl) * C + ((c8 ^ (((nl + ROFF) >> 2) & 1)) << 3);
            dstep = RWR * C;
        }
        // Rows of the band one after the other, the row's XT column groups as independent accumulator chains (as in the 32-channel
        // form).  Per row and group: ONE new fragment for steps 0-2 (row r+2; rows r and r+1 are still in registers from the rows
        // before) plus the fragments of steps 3 and 4 -- three LDS reads for five MFMAs instead of five.
        // Ragged region widths (38 / 36 / 34 px = two full 16-pixel groups + 6 / 4 / 2 px): the band walks the FULL groups only; the
        // leftover strip (RHO rows x RX columns) is packed 16 pixels at a time into "strip groups" whose lanes sit in different rows
        // -- 12 / 7 / 4 groups instead of 30 / 28 / 26 two-thirds-empty ones -- and handed to the waves with spare time: the last
        // wave's band is short or empty (RHO is not a multiple of 8), so it takes the first K0 strip groups, the others one or two each.
        // Same k-step order and operands per output pixel as a band group: bit-identical results.
        constexpr bool STRIP = RAGGED && !GLOBAL_OUT;
        constexpr int XTR = STRIP ? XT - 1 : XT;
        if (yb < RHO) {
            bf16x8 fa[XT][RB + 2];
#pragma unroll
            for (int xt = 0; xt < XTR; ++xt) {
                const bf16_t* bA = (RAGGED && xt == XT - 1) ? pAl : pA + xt * 16 * C;
                fa[xt][0] = *(const bf16x8*)bA; fa[xt][1] = *(const bf16x8*)(bA + RS);
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int y = yb + r;
                if (y >= RHO) break;
                bf16x8 f3[XT], f4[XT];
#pragma unroll
                for (int xt = 0; xt < XTR; ++xt) {
                    const bool lastg = RAGGED && xt == XT - 1;
                    fa[xt][r + 2] = *(const bf16x8*)((lastg ? pAl : pA + xt * 16 * C) + (r + 2) * RS);
                    f3[xt] = *(const bf16x8*)((lastg ? pCl : pC + xt * 16 * C) + r * RS);
                    f4[xt] = *(const bf16x8*)((lastg ? pDl : pD + xt * 16 * C) + r * dstep);
                }
                f32x4 acc[XT][1];
#pragma unroll
                for (int xt = 0; xt < XTR; ++xt) acc[xt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0][0], fa[xt][r], bias[0], 0, 0, 0);
#pragma unroll
                for (int xt = 0; xt < XTR; ++xt) acc[xt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[1][0], fa[xt][r + 1], acc[xt][0], 0, 0, 0);
#pragma unroll
                for (int xt = 0; xt < XTR; ++xt) acc[xt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[2][0], fa[xt][r + 2], acc[xt][0], 0, 0, 0);
#pragma unroll
                for (int xt = 0; xt < XTR; ++xt) acc[xt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[3][0], f3[xt], acc[xt][0], 0, 0, 0);
#pragma unroll
                for (int xt = 0; xt < XTR; ++xt) acc[xt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[4][0], f4[xt], acc[xt][0], 0, 0, 0);
#pragma unroll
                for (int xt = 0; xt < XTR; ++xt) epi(xt, r, y, acc[xt]);
            }
        }
        if constexpr (STRIP) {
            // Strip groups are COLUMN groups when the input buffer's row stride is odd (the two-block chain's buffers): 16 consecutive
            // rows of one strip column.  A pixel record is two 16-byte LDS slots and a ds_read_b128 is served in lane groups
            // {0-3,12-15 of one chunk | 4-11 of the other}: with a row stride of 1 (mod 8) pixels the 16 rows land on the 16 slots
            // exactly like the 16 consecutive pixels of a band group -- conflict-free for every tap, and the swizzle terms (a
            // function of the column) become wave-uniform.  Round 3's row-major packing (16 pixels over 3-8 rows of a 6 / 4 / 2-pixel
            // strip, row stride 40 = 0 mod 8: rows aliased on the same banks) doubled the kernel's SQ_LDS_BANK_CONFLICT
            // (6.45e6 -> 1.38e7 per launch); it is kept for even strides (the one-block chain).
            constexpr bool COLG = (RWI & 1) == 1 && (!SECOND || (RWR & 1) == 1);
            constexpr int RX = RWO - XLAST, NSP = RHO * RX;
            constexpr int CG = (RHO + 15) / 16;                          // column groups per strip column
            constexpr int NSG = COLG ? RX * CG : (NSP + 15) / 16;
            constexpr int ROWS7 = RHO - 7 * RB < 0 ? 0 : (RHO - 7 * RB > RB ? RB : RHO - 7 * RB);      // band rows of the last wave
            // a strip group costs about two band groups (five fragment reads instead of three, one dependent MFMA chain, per-lane
            // addresses): the last wave takes as many as fit in HALF of its band's gap (in band-group units), the rest go round
            constexpr int K0 = NSG < RB - ROWS7 ? NSG : RB - ROWS7;
            static_assert(NSG - K0 <= 16, "at most two strip groups per wave after the last wave's share");
            auto strip = [&](int j) __attribute__((always_inline)) {
                int row, col;
                bool valid;
                if constexpr (COLG) {
                    const int cj = j / CG, rg = j - cj * CG;              // wave-uniform
                    // rows dealt evenly over the column's groups (30 rows: 15 + 15, not 16 + 14)
                    constexpr int RPG = (RHO + CG - 1) / CG;
                    const int r0 = rg * RPG;
                    valid = n < RPG && r0 + n < RHO;
                    const int rn = r0 + (n < RPG ? n : RPG - 1);         // idle lanes re-read a neighbour's addresses (identical addresses
                    row = rn < RHO ? rn : RHO - 1;                        // broadcast: no bank conflict) and store nothing
                    col = XLAST + cj;
                } else {
                    const int p = 16 * j + n;
                    valid = p < NSP;
                    const int pc = valid ? p : NSP - 1;                   // lanes past the strip recompute its last pixel and store nothing
                    row = pc / RX; col = XLAST + (pc - row * RX);
                }
                const bf16_t* b0 = s_in + ((row + IOFF) * RWI + IOFF + col) * C;
                const int sw2 = (c8 ^ (((col + 2 + IOFF) >> 2) & 1)) << 3;
                const bf16_t* a0 = b0 + h * C + ((c8 ^ (((col + h + IOFF) >> 2) & 1)) << 3);        // steps 0-2: rows row + dy, column col | col+1
                const bf16_t* a3 = b0 + h * RS + 2 * C + sw2;                                       // step 3: column col+2 of rows row | row+1
                const bf16_t* a4 = b0 + 2 * RS + 2 * C + sw2;                                       // step 4: (row+2, col+2) | block input / pad
                if (RES_MFMA && h) a4 = s_res + ((row + ROFF) * RWR + ROFF + col) * C + ((c8 ^ (((col + ROFF) >> 2) & 1)) << 3);
                f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0][0], *(const bf16x8*)a0, bias[0], 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[1][0], *(const bf16x8*)(a0 + RS), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[2][0], *(const bf16x8*)(a0 + 2 * RS), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[3][0], *(const bf16x8*)a3, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[4][0], *(const bf16x8*)a4, acc, 0, 0, 0);
                unsigned q0 = relu_pk(pack2(acc[0], acc[1])), q1 = relu_pk(pack2(acc[2], acc[3]));
                if (!interior) {                                      // zero padding of the next conv outside the image
                    const int gy = gy0 + row, gx = gx0 + col;
                    const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
                    q0 = inside ? q0 : 0u; q1 = inside ? q1 : 0u;
                }
                if (valid) *(u32x2*)(s_out + ((row + OOFF) * ORW + col + OOFF) * C + ((((g >> 1) ^ (((col + OOFF) >> 2) & 1)) << 3) + (g & 1) * 4)) = u32x2{q0, q1};
            };
            if (wave == 7) {
#pragma unroll
                for (int j = 0; j < K0; ++j) strip(j);
            }
            if (K0 + wave < NSG) strip(K0 + wave);
            if (NSG - K0 > 8 && K0 + 8 + wave < NSG) strip(K0 + 8 + wave);
        }
    }
}

// One BasicBlock per tile.  C=32 is persistent: a workgroup walks tiles, the next tile's input region is prefetched into registers while
// the current one is computed, and the weights of both convs (2 x 18 KB) stay resident in LDS.  C=16 runs one tile per workgroup with
// its 5 weight fragments per conv straight from global memory / L2 (persistent variants measured slower there).
// (NB, the number of blocks, is 1: the parameter stays because the kernel's template-id is the key of the committed traffic profiles.)
template <int C, int NB, int TH, int TW>
__global__ __launch_bounds__(512) void bb_chain_kernel(BBArgs a) {
    static_assert(NB == 1, "one BasicBlock; the two-block chain is bb_chain2_kernel / c16_chain_kernel");
    constexpr int L = 2;
    constexpr int R0H = TH + 2 * L, R0W = TW + 2 * L;
    constexpr int SZ_A = R0H * R0W * C, SZ_B = (R0H - 2) * (R0W - 2) * C;
    constexpr int KSTEPS = (C == 16) ? 5 : 9, MT = C / 16;
    constexpr int W_UNITS = KSTEPS * MT * 64;                    // 16-byte units per conv
    constexpr bool RESIDENT = (C == 32);                         // both convs' weights, their biases and the follower in LDS; otherwise everything from global memory
    constexpr int W_PT = (W_UNITS + 511) / 512;
    constexpr int IN_UNITS = R0H * R0W * (C / 8), IN_PT = (IN_UNITS + 511) / 512;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* bufA = (bf16_t*)smem;              // block input region (later overwritten in place by the block output)
    bf16_t* bufB = bufA + SZ_A;                // intermediate of the current block
    bf16_t* s_wt = bufB + SZ_B;                // RESIDENT: the weights of the two convs
    // RESIDENT: the convs' biases and the follower's fragment + bias live in LDS too (BB_MISC_BYTES behind the weights).  Fetched
    // from global memory inside the tile loop they were loads BEHIND the next tile's prefetch in the in-order vector-memory queue:
    // their wait (s_waitcnt vmcnt(0)) held every conv's first MFMA until the whole prefetch had landed (round 5)
    float* s_misc = (float*)(s_wt + (RESIDENT ? 2 * W_UNITS * 8 : 0));
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: row tests and row addresses on the scalar unit
    const int my_tiles = (a.total_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;

    u32x4 pin[IN_PT];
    // byte offset of each of the thread's units from its tile's first halo pixel: the same for every tile (unused units of the last
    // round point at the first pixel, loaded and never committed)
    unsigned voff[IN_PT];
#pragma unroll
    for (int k = 0; k < IN_PT; ++k) {
        const int u = tid + k * 512;
        const int c8 = u % (C / 8), pix = u / (C / 8);
        voff[k] = u < IN_UNITS ? (unsigned)((((pix / R0W) * a.W + pix % R0W) * C + c8 * 8) * 2) : 0u;
    }
    auto issue_in = [&](int it) {
        const TileAt t = tile_at<TH, TW, L>(xcd_tile(blockIdx.x + it * gridDim.x, a.total_tiles), a.tiles_per_img, a.tiles_x);
        const int b = t.b, gy0 = t.y0, gx0 = t.x0;
        if (gy0 >= 0 && gy0 + R0H <= a.H && gx0 >= 0 && gx0 + R0W <= a.W) {
            // the whole halo region lies inside the image (wave-uniform): a scalar base + the per-lane constants -- no coordinates, no
            // bounds tests, no 64-bit per-lane address arithmetic (round 5: the general form below is ~25 vector instructions per load,
            // issued while the matrix pipe has nothing to do)
            const char* base = (const char*)(a.x + ((size_t)(b * a.H + gy0) * a.W + gx0) * C);
#pragma unroll
            for (int k = 0; k < IN_PT; ++k) pin[k] = *(const u32x4*)(base + opaque_u32(voff[k]));
            return;
        }
#pragma unroll
        for (int k = 0; k < IN_PT; ++k) {
            const int u = tid + k * 512;
            const int c8 = u % (C / 8), pix = u / (C / 8);
            const int gy = gy0 + pix / R0W, gx = gx0 + pix % R0W;
            pin[k] = u32x4{0u, 0u, 0u, 0u};
            if (u < IN_UNITS && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) pin[k] = *(const u32x4*)(a.x + ((size_t)(b * a.H + gy) * a.W + gx) * C + c8 * 8);
        }
    };
    if (RESIDENT) {
        // the first tile and both convs' weights travel together: one round trip before the loop
        if (my_tiles > 0) issue_in(0);
        u32x4 pw2[2][W_PT];
#pragma unroll
        for (int cv = 0; cv < 2; ++cv)
#pragma unroll
            for (int k = 0; k < W_PT; ++k) { const int u = tid + k * 512; pw2[cv][k] = u32x4{0u, 0u, 0u, 0u}; if (u < W_UNITS) pw2[cv][k] = ((const u32x4*)a.w[cv])[u]; }
#pragma unroll
        for (int cv = 0; cv < 2; ++cv)
#pragma unroll
            for (int k = 0; k < W_PT; ++k) { const int u = tid + k * 512; if (u < W_UNITS) ((u32x4*)(s_wt + cv * W_UNITS * 8))[u] = pw2[cv][k]; }
        // floats [0, C) bias of conv 0, [C, 2C) bias of conv 1, [2C, 2C+16) follower bias, then the follower's 64 x 16-byte fragment
        if (tid < C) { s_misc[tid] = a.bias[0][tid]; s_misc[C + tid] = a.bias[1][tid]; }
        if (a.yf) {
            if (tid < 16) s_misc[2 * C + tid] = a.bf[tid];
            if (tid >= 64 && tid < 128) ((u32x4*)(s_misc + 2 * C + 16))[tid - 64] = ((const u32x4*)a.wf)[tid - 64];
        }
    } else {
        if (my_tiles > 0) issue_in(0);
    }

    if (my_tiles <= 0) return;          // (workgroup-uniform)
    if (RESIDENT) prefetch_arrived(pin);          // every path into the loop has the prefetch registers complete (see prefetch_arrived)
    for (int it = 0; it < my_tiles; ++it) {
        const TileAt tile = tile_at<TH, TW>(xcd_tile(blockIdx.x + it * gridDim.x, a.total_tiles), a.tiles_per_img, a.tiles_x);
        const int b = tile.b, oy0 = tile.y0, ox0 = tile.x0;
        __syncthreads();                       // previous tile fully consumed (resident weights visible on the first pass)
#pragma unroll
        for (int k = 0; k < IN_PT; ++k) {
            const int u = tid + k * 512;
            if (u < IN_UNITS) { const int c8 = u % (C / 8), pix = u / (C / 8); *(u32x4*)(bufA + bb_off<C>(pix, pix % R0W, c8)) = pin[k]; }
        }
        __syncthreads();
        if (it + 1 < my_tiles) issue_in(it + 1);
        const bf16_t* w0 = RESIDENT ? s_wt : a.w[0];
        const bf16_t* w1 = RESIDENT ? s_wt + W_UNITS * 8 : a.w[1];
        const float* bias0 = RESIDENT ? s_misc : a.bias[0];
        const float* bias1 = RESIDENT ? s_misc + C : a.bias[1];
        const bf16_t* wfl = RESIDENT ? (const bf16_t*)(s_misc + 2 * C + 16) : a.wf;
        const float* bfl = RESIDENT ? s_misc + 2 * C : a.bf;
        bb_conv<C, R0W, 0, R0H - 2, R0W - 2, false, 1, 0, false, R0W - 2, 0>(bufA, bufB, nullptr, w0, bias0, nullptr, oy0 - 1, ox0 - 1, a.H, a.W, b, wave, lane);
        __syncthreads();
        // the next tile's input (requested before the first conv) is waited for HERE, in front of the second conv's stores
        if (RESIDENT) prefetch_arrived(pin);
        bb_conv<C, R0W - 2, 0, TH, TW, true, R0W, 2, true, 1, 0>(bufB, nullptr, bufA, w1, bias1, a.y, oy0, ox0, a.H, a.W, b, wave, lane, wfl, bfl, a.yf);
    }
}

// One tile per workgroup, weights straight from L2 into registers (lowest register footprint: two workgroups per CU): the C=16 two-block
// chain with its fuse-sum / head epilogue configured at RUN time -- the fallback for term layouts other than HRNet's and the cross-check
// (TTUP_BB2_GENERIC=1) of c16_chain_kernel (csrc/chain16.h), which carries the forms the network uses and superseded this kernel's
// compiled-out variants in round 6.
template <int C, int TH, int TW>
__global__ __launch_bounds__(512, 4) void bb_chain2_kernel(BBArgs a) {       // 4 waves per SIMD = two workgroups per CU: at most 128 VGPRs
    constexpr int L = 4;
    constexpr int R0H = TH + 2 * L, R0W = TW + 2 * L;
    // row strides (pixels) of the two LDS buffers: ODD, so that 16 consecutive rows of one column fall on 16 different 16-byte
    // slots -- the strip groups of bb_conv are column groups (see there); 40 -> 41 and 38 -> 39 pixels cost 2 KB of LDS per workgroup
    constexpr int SA = (R0W & 1) ? R0W : R0W + 1;
    constexpr int SB = ((R0W - 2) & 1) ? R0W - 2 : R0W - 1;
    constexpr int SZ_A = R0H * SA * C;
    constexpr int SZ_B = (R0H - 2) * SB * C;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* bufA = (bf16_t*)smem;
    bf16_t* bufB = bufA + SZ_A;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: row tests and row addresses on the scalar unit
    // 3-D grid (tile column, tile row, image): no division to find the tile
    // (XCD = linear workgroup id % 8 = blockIdx.x % 8 when the row has a multiple of 8 tiles: every XCD then takes a strip of
    // adjacent tile columns through all rows and images instead of every eighth column -- see xcd_tile)
    const int bx = (gridDim.x & 7) == 0 ? (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
    const int b = blockIdx.z, tt = blockIdx.y * a.tiles_x + bx;
    const int oy0 = blockIdx.y * TH, ox0 = bx * TW;
    BBFrag16 fr;
    {
        // all of the thread's loads are issued before the first LDS store: ONE memory round trip for the tile, not one per unit.
        // A thread keeps one 16-byte column unit and walks rows (row lane rl, then every RL-th row): the global and the LDS
        // address of every further row are the first row's plus a constant -- no per-unit division, one bounds test per row.
        constexpr int CU = R0W * (C / 8);                 // 16-byte units per tile row
        constexpr int RL = 512 / CU;                      // row lanes
        constexpr int IN_PT = (R0H + RL - 1) / RL;
        static_assert(RL >= 1, "tile row wider than the workgroup");
        const int cu = tid % CU, rl = tid / CU;
        const int col = cu / (C / 8), c8 = cu % (C / 8);
        const int gx = ox0 - L + col, gyb = oy0 - L + rl;
        const bool col_ok = rl < RL && gx >= 0 && gx < a.W;
        const bf16_t* src = a.x + ((long long)(b * a.H + gyb) * a.W + gx) * C + c8 * 8;      // may point outside for halo rows / columns: only dereferenced when valid
        const long long row_step = (long long)RL * a.W * C;
        u32x4 v[IN_PT];
#pragma unroll
        for (int k = 0; k < IN_PT; ++k) {
            const int gy = gyb + k * RL;
            // branch-free: an invalid unit reads the tensor's first bytes and is zeroed afterwards (a branch around the load
            // would make every load wait for the one before it)
            const bool ok = col_ok && rl + k * RL < R0H && gy >= 0 && gy < a.H;
            const u32x4 t = *(const u32x4*)(ok ? src + k * row_step : a.x);
            v[k] = u32x4{ok ? t.x : 0u, ok ? t.y : 0u, ok ? t.z : 0u, ok ? t.w : 0u};
        }
        bf16_t* dst = bufA + bb_off<C>(rl * SA + col, col, c8);
#pragma unroll
        for (int k = 0; k < IN_PT; ++k)
            if (rl < RL && rl + k * RL < R0H) *(u32x4*)(dst + k * RL * SA * C) = v[k];
    }
    const bf16x8 idm = bb_identity_frag(lane);
    if (C == 16) bb_load_frag16(fr, a.w[0], a.bias[0], lane);          // first conv's fragments: in flight across the barrier
    __syncthreads();
    const BBFrag16* pre = C == 16 ? &fr : nullptr;
    bb_conv<C, SA, 0, R0H - 2, R0W - 2, false, 1, 0, false, SB, 0>(bufA, bufB, nullptr, a.w[0], a.bias[0], nullptr, oy0 - 3, ox0 - 3, a.H, a.W, b, wave, lane,
                                                                            nullptr, nullptr, nullptr, nullptr, nullptr, pre);
    if (C == 16) bb_load_frag16(fr, a.w[1], a.bias[1], lane);          // next conv's fragments: requested BEFORE the barrier
    __syncthreads();
    bb_conv<C, SB, 0, R0H - 4, R0W - 4, true, SA, 2, false, SA, 2>(bufB, bufA, bufA, a.w[1], a.bias[1], nullptr, oy0 - 2, ox0 - 2, a.H, a.W, b, wave, lane,
                                                                            nullptr, nullptr, nullptr, nullptr, nullptr, pre, nullptr, idm);
    if (C == 16) bb_load_frag16(fr, a.w[2], a.bias[2], lane);
    __syncthreads();
    // The fuse-layer terms that the last conv's epilogue adds (1x1-conv'd lower branches at 1/2, 1/4, 1/8 resolution): the tile's
    // slices (12x16 + 6x8 + 3x4 pixels of 16 channels = 8 KB at most) are requested now, travel while conv3 runs, and are parked in
    // the tail of bufB that conv3's 26x34 output leaves free -- the epilogue then reads them from LDS instead of paying a memory
    // round trip per output row.
    constexpr int T_FREE = SZ_B - (TH + 2) * (TW + 2) * C;       // elements of bufB behind conv3's output
    static_assert(C != 16 || (TH % 8 == 0 && TW % 8 == 0), "term slices are aligned to the tile for 8-aligned tiles");
    bf16_t* s_terms = bufB + (TH + 2) * (TW + 2) * C;
    u32x4 treg = u32x4{0u, 0u, 0u, 0u};
    int tunit = -1;
    BBTermLds tlds;
    tlds.s_terms = s_terms;
    if (C == 16) {
        int base = 0;                 // in 16-byte units (two per pixel)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            tlds.toff[k] = 0; tlds.tw[k] = 1;
            if (k < a.nsum) {
                const int sh = a.ssh[k], hk = TH >> sh, wk = TW >> sh;
                tlds.toff[k] = base * 8; tlds.tw[k] = wk;
                const int u = tid - base;
                if (u >= 0 && u < hk * wk * 2) {
                    const int px = u >> 1, ty = (oy0 >> sh) + px / wk, tx = (ox0 >> sh) + px % wk;
                    if (ty < (a.H >> sh) && tx < (a.W >> sh)) treg = *(const u32x4*)(a.st[k] + ((size_t)(b * (a.H >> sh) + ty) * (a.W >> sh) + tx) * 16 + (u & 1) * 8);
                    tunit = tid;
                }
                base += hk * wk * 2;
            }
        }
    }
    bb_conv<C, SA, 2, R0H - 6, R0W - 6, false, 1, 0, false, R0W - 6, 0>(bufA, bufB, nullptr, a.w[2], a.bias[2], nullptr, oy0 - 1, ox0 - 1, a.H, a.W, b, wave, lane,
                                                                            nullptr, nullptr, nullptr, nullptr, nullptr, pre);
    if (C == 16 && tunit >= 0) { static_assert(C != 16 || T_FREE * 2 >= ((TH >> 1) * (TW >> 1) + (TH >> 2) * (TW >> 2) + (TH >> 3) * (TW >> 3)) * 32, "bufB tail holds the term slices"); ((u32x4*)s_terms)[tunit] = treg; }
    if (C == 16) bb_load_frag16(fr, a.w[3], a.bias[3], lane);
    __syncthreads();
    BBBest best; best.v = -INFINITY; best.i = 0x7fffffffffffffffLL;
    bb_conv<C, R0W - 6, 0, TH, TW, true, SA, 4, true, 1, 0>(bufB, nullptr, bufA, a.w[3], a.bias[3], a.y, oy0, ox0, a.H, a.W, b, wave, lane,
                                                                   nullptr, nullptr, nullptr, &a, &best, pre, &tlds, idm);
    if (C == 16 && a.heat) {
        // run-time form: lanes -> wave (shuffles) -> workgroup (through the now idle LDS)
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_down(best.v, off, 64);
            const long long oi = __shfl_down(best.i, off, 64);
            if (bb_better(ov, oi, best.v, best.i)) { best.v = ov; best.i = oi; }
        }
        __syncthreads();                      // every wave is done with bufA / bufB
        float* sv = (float*)smem; long long* si = (long long*)(smem + 64);
        if (lane == 0) { sv[wave] = best.v; si[wave] = best.i; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < 8; ++k) if (bb_better(sv[k], si[k], best.v, best.i)) { best.v = sv[k]; best.i = si[k]; }
            a.pv[(size_t)b * a.tiles_per_img + tt] = best.v;
            a.pi[(size_t)b * a.tiles_per_img + tt] = best.i;
        }
    }
}

// the geometry fields of a chain's arguments for TH x TW tiles
template <int TH, int TW>
static BBArgs bb_tiled(const BBArgs& a, int batch, int h, int w) {
    BBArgs k = a;
    k.H = h; k.W = w; k.tiles_x = cdiv(w, TW); k.tiles_per_img = k.tiles_x * cdiv(h, TH); k.total_tiles = k.tiles_per_img * batch;
    return k;
}

template <int C, int TH, int TW>
static int launch_bb2_t(const BBArgs& a, int batch, int h, int w, hipStream_t st) {
    constexpr int SA = ((TW + 8) & 1) ? TW + 8 : TW + 9, SB = ((TW + 6) & 1) ? TW + 6 : TW + 7;       // odd row strides, as in the kernel
    constexpr size_t SMEM = (size_t)((TH + 8) * SA + (TH + 6) * SB) * C * 2 + 64;       // + one argmax slot per wave
    static_assert(SMEM <= 160 * 1024, "LDS budget");
    static_assert(2 * SMEM <= 160 * 1024 || TH * TW > 24 * 32, "the 24x32 tile runs two workgroups per CU");
    const BBArgs k = bb_tiled<TH, TW>(a, batch, h, w);
    return launch_noted(bb_chain2_kernel<C, TH, TW>, dim3(k.tiles_x, cdiv(h, TH), batch), 512, SMEM, st, k, "bb_chain2_kernel<%d, %d, %d>", C, TH, TW);
}

constexpr int BB_MISC_BYTES = (2 * 32 + 16) * 4 + 1024;      // C=32: the biases and the follower's bias + fragment behind the resident weights (bb_chain_kernel: s_misc)
template <int C, int TH, int TW>
static int launch_bb_t(const BBArgs& a, int batch, int h, int w, hipStream_t st) {
    constexpr int KSTEPS = (C == 16) ? 5 : 9, MT = C / 16;
    constexpr size_t SMEM = (size_t)((TH + 4) * (TW + 4) + (TH + 2) * (TW + 2)) * C * 2 +
                            (C == 16 ? 0 : (size_t)2 * KSTEPS * MT * 1024 + BB_MISC_BYTES);          // C=32: the weights of both convs are LDS-resident
    static_assert(SMEM <= 160 * 1024, "LDS budget");
    const BBArgs k = bb_tiled<TH, TW>(a, batch, h, w);
    const int per_cu = (int)((160 * 1024) / SMEM) > 2 ? 2 : ((int)((160 * 1024) / SMEM) < 1 ? 1 : (int)((160 * 1024) / SMEM));
    const int grid = C == 16 ? k.total_tiles : persistent_grid(k.total_tiles, per_cu);      // C=16: one tile per workgroup
    return launch_noted(bb_chain_kernel<C, 1, TH, TW>, dim3(grid), 512, SMEM, st, k, "bb_chain_kernel<%d, 1, %d, %d>", C, TH, TW);
}

}  // namespace ttup
