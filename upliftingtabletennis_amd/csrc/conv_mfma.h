// The generic implicit-GEMM conv (any of the network's shapes, one K chunk at a time) and the paired stride-2 conv.
#pragma once
#include "conv_dev.h"
#include "conv.h"

namespace ttup {

struct ConvKArgs {
    const bf16_t* src0 = nullptr;
    const bf16_t* src1 = nullptr;
    const bf16_t* wpack = nullptr;
    const float* bias = nullptr;
    const bf16_t* residual = nullptr;
    bf16_t* dst = nullptr;
    int c0 = 0, c1 = 0;        // channels of the two sources
    int nchunk0 = 0, nchunk = 0;  // chunks taken from src0, total chunks
    int H = 0, W = 0, OH = 0, OW = 0;
    int tiles_x = 0, tiles_per_img = 0, total_tiles = 0;
    int relu = 0;
    // fused 1x1 follower (F11): dst11 = relu(W11 . dst + b11), 64 -> 32 channels
    const bf16_t* w11 = nullptr; const float* bias11 = nullptr; bf16_t* dst11 = nullptr;
    // further fuse-layer terms added in the epilogue (wasb.py:236-243): res2 at the output resolution (the branch's own
    // tensor), res3 at 1/2^sh3 of it (a 1x1-conv'd lower branch, nearest-neighbour upsampled), both COUT channels
    const bf16_t* res2 = nullptr; const bf16_t* res3 = nullptr; int sh3 = 0;
    // conv64_kernel: linear 1x1 followers on the tile just produced (the fuse-layer convs 64 -> 16 / 64 -> 32 that feed the
    // higher-resolution branches, wasb.py:189-205: conv + BN, no ReLU)
    const bf16_t* wl16 = nullptr; const float* bl16 = nullptr; bf16_t* dl16 = nullptr;
    const bf16_t* wl32 = nullptr; const float* bl32 = nullptr; bf16_t* dl32 = nullptr;
    // conv_s2_pair_kernel: the second conv on the same input (16 -> 16), its own ReLU flag
    const bf16_t* wpack_b = nullptr; const float* bias_b = nullptr; bf16_t* dst_b = nullptr; int relu_b = 0;
    int xcd = 0;           // conv_mfma_kernel: walk the tiles in the XCD-aware order of xcd_tile (stride-2 convs; see launch_mfma)
};

// Persistent, software-pipelined version: a workgroup walks work items (tile, channel chunk); the global loads of
// item i+1 (halo tile chunk + that chunk's weight fragments) are issued into registers BEFORE the MFMA loop of item i
// and written to LDS after it, so HBM/L2 latency hides behind the matrix work (single LDS buffer, two barriers per item).
// Single-chunk convs keep their weights resident in LDS across all tiles of the workgroup.
template <int CK, int COUT, int KS, int S, int TH, int TW, int NW, bool F11>
__global__ __launch_bounds__(NW * 64) void conv_mfma_kernel(ConvKArgs a) {
    constexpr int NTHR = NW * 64;
    constexpr int MT = COUT / 16;
    constexpr int IH = (TH - 1) * S + KS, IW = (TW - 1) * S + KS;
    constexpr int TAPS = KS * KS;
    constexpr int KSTEPS = (CK == 32) ? TAPS : (TAPS + 1) / 2;
    constexpr int NTW = TW / 16;
    constexpr int NT = TH * NTW / NW;         // N-tiles per wave
    constexpr int PAD = KS / 2;
    constexpr int IN_ELEMS = IH * IW * CK;
    constexpr int W_ELEMS = KSTEPS * MT * 64 * 8;
    constexpr int IN_UNITS = IH * IW * (CK / 8), IN_PT = (IN_UNITS + NTHR - 1) / NTHR;
    constexpr int W_UNITS = W_ELEMS / 8, W_PT = (W_UNITS + NTHR - 1) / NTHR;
    static_assert(TH * NTW % NW == 0, "tile must split over the waves");

    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* s_in = (bf16_t*)smem;
    bf16_t* s_w = s_in + ((IN_ELEMS + 7) & ~7);

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: row tests and row addresses on the scalar unit
    const int n = lane & 15, g = lane >> 4;
    const int nchunk = a.nchunk;
    const int my_tiles = (a.total_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    const int n_items = my_tiles * nchunk;
    const unsigned st_c = (unsigned)((n * COUT + g * 4 * MT) * 2);          // lane's byte offset inside a 16-pixel group of COUT-channel records

    u32x4 pin[IN_PT], pw[W_PT];
    // byte offsets of the thread's units from the tile's first halo pixel in src0 (explained at issue_in of bb_chain_kernel, conv_bb.h).  Register budget: the 128-cout
    // variant sits at 252 of 256 with them and the stride-2 16 -> 64 conv at exactly 128 (two workgroups per CU; at 131 it was one
    // and 20 % slower) -- both only since the wave index is a scalar (readfirstlane) and the epilogue addresses take a scalar base
    unsigned voff[IN_PT];
#pragma unroll
    for (int k = 0; k < IN_PT; ++k) {
        const int u = tid + k * NTHR;
        const int c8 = u % (CK / 8), pix = u / (CK / 8);
        voff[k] = u < IN_UNITS ? (unsigned)((((pix / IW) * a.W + pix % IW) * a.c0 + c8 * 8) * 2) : 0u;
    }
    auto issue = [&](int item) {
        const int tl0 = blockIdx.x + (item / nchunk) * gridDim.x, chunk = item % nchunk;
        const TileAt t = tile_at<TH * S, TW * S, PAD>(a.xcd ? xcd_tile(tl0, a.total_tiles) : tl0, a.tiles_per_img, a.tiles_x);
        const int b = t.b, gy0 = t.y0, gx0 = t.x0;
        const bool first = chunk < a.nchunk0;
        const bf16_t* src = first ? a.src0 : a.src1;
        const int csrc = first ? a.c0 : a.c1;
        const int ch0 = (first ? chunk : chunk - a.nchunk0) * CK;
        if (first && gy0 >= 0 && gy0 + IH <= a.H && gx0 >= 0 && gx0 + IW <= a.W) {          // halo tile inside the image: scalar base + lane constants
            const char* base = (const char*)(a.src0 + ((size_t)(b * a.H + gy0) * a.W + gx0) * a.c0 + ch0);
#pragma unroll
            for (int k = 0; k < IN_PT; ++k) pin[k] = *(const u32x4*)(base + opaque_u32(voff[k]));
        } else {
#pragma unroll
            for (int k = 0; k < IN_PT; ++k) {
                const int u = tid + k * NTHR;
                const int c8 = u % (CK / 8), pix = u / (CK / 8);
                const int gy = gy0 + pix / IW, gx = gx0 + pix % IW;
                pin[k] = u32x4{0u, 0u, 0u, 0u};
                if (u < IN_UNITS && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
                    pin[k] = *(const u32x4*)(src + ((size_t)(b * a.H + gy) * a.W + gx) * csrc + ch0 + c8 * 8);
            }
        }
        if (nchunk > 1 || item == 0) {
            const u32x4* wsrc = (const u32x4*)(a.wpack + (size_t)chunk * W_ELEMS);
#pragma unroll
            for (int k = 0; k < W_PT; ++k) { const int u = tid + k * NTHR; if (u < W_UNITS) pw[k] = wsrc[u]; }
        }
    };
    auto commit = [&](int item) {
#pragma unroll
        for (int k = 0; k < IN_PT; ++k) {
            const int u = tid + k * NTHR;
            if (u < IN_UNITS) { const int c8 = u % (CK / 8), pix = u / (CK / 8); *(u32x4*)(s_in + lds_off<CK, IW>(pix / IW, pix % IW, c8)) = pin[k]; }
        }
        if (nchunk > 1 || item == 0) {
#pragma unroll
            for (int k = 0; k < W_PT; ++k) { const int u = tid + k * NTHR; if (u < W_UNITS) ((u32x4*)s_w)[u] = pw[k]; }
        }
    };

    f32x4 bias[MT];          // seeds the accumulators
#pragma unroll
    for (int m = 0; m < MT; ++m) bias[m] = *(const f32x4*)(a.bias + g * 4 * MT + m * 4);

    // fused follower: its 4 weight fragments (2 k-steps x 2 m-tiles) stay in registers for the whole kernel
    bf16x8 af11[2][2];
    f32x4 bias11[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    if (F11) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int m = 0; m < 2; ++m) af11[k][m] = *(const bf16x8*)(a.w11 + ((k * 2 + m) * 64 + lane) * 8);
#pragma unroll
        for (int m = 0; m < 2; ++m) bias11[m] = *(const f32x4*)(a.bias11 + g * 8 + m * 4);
    }

    // per-lane B-fragment bases: CK=32 -> one per tap column dx (k-step s = dy*KS+dx); CK=16 -> one per k-step (two taps)
    constexpr int NBB = (CK == 32) ? KS : KSTEPS;
    const bf16_t* bB[NBB];
#pragma unroll
    for (int k = 0; k < NBB; ++k) {
        int dy = 0, dx = k, c8 = g;
        if (CK != 32) {
            int tap = 2 * k + (g >> 1);
            if (tap > TAPS - 1) tap = TAPS - 1;     // padded k-group: weights are zero
            dy = tap / KS; dx = tap % KS; c8 = g & 1;
        }
        bB[k] = s_in + lds_off<CK, IW>(dy, n * S + dx, c8);
    }

    f32x4 acc[MT][NT];
    if (n_items <= 0) return;          // (workgroup-uniform)
    issue(0);
    prefetch_arrived(pin); prefetch_arrived(pw);          // every path into the loop has the prefetch registers complete (see prefetch_arrived)
    for (int item = 0; item < n_items; ++item) {
        const int chunk = item % nchunk;
        if (item > 0) __syncthreads();          // every wave finished reading the previous item's LDS image
        commit(item);
        __syncthreads();
        if (item + 1 < n_items) issue(item + 1);
        if (chunk == 0) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[m][t] = bias[m];
        }
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            bf16x8 af[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) af[m] = *(const bf16x8*)(s_w + ((s * MT + m) * 64 + lane) * 8);
            // lane-dependent part of the pixel-fragment address (tap column + channel chunk + swizzle) is precomputed in
            // bB[]; the N-tile / tap-row part below is a compile-time immediate
            const bf16_t* bp = (CK == 32) ? bB[s % KS] : bB[s];
            const int dyc = (CK == 32) ? s / KS : 0;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int nt = wave * NT + t;        // wave-uniform
                const int r = nt / NTW, cg = nt % NTW;
                const bf16x8 bfr = *(const bf16x8*)(bp + ((r * S + dyc) * IW + cg * 16 * S) * CK);
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m], bfr, acc[m][t], 0, 0, 0);
                }
            }
        }
        // (no prefetch_arrived in front of the epilogue here: this kernel runs two to four workgroups per CU, another workgroup's MFMAs
        // cover a store drain at the top of the next item, and the HBM-bound 32 -> 32 conv at full resolution measured 4 % SLOWER with
        // the wait moved in front of its stores -- 0.204 against 0.196 ms, round 5)
        if (chunk != nchunk - 1) continue;
        // ---- epilogue: lane holds couts [g*4*MT, (g+1)*4*MT) of pixel n of each of its N-tiles
        const int tl0 = blockIdx.x + (item / nchunk) * gridDim.x;
        const TileAt tile = tile_at<TH, TW>(a.xcd ? xcd_tile(tl0, a.total_tiles) : tl0, a.tiles_per_img, a.tiles_x);
        const int b = tile.b, oy0 = tile.y0, ox0 = tile.x0;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int nt = wave * NT + t;
            const int oy = oy0 + nt / NTW, ox = ox0 + (nt % NTW) * 16 + n;
            if (oy >= a.OH || ox >= a.OW) continue;
            // element offset of the lane's first output channel: a wave-uniform part (scalar registers) + the lane constant -- the
            // loads and stores below then take a scalar base and a 32-bit lane offset instead of a 64-bit per-lane address chain
            const size_t ou = ((size_t)(b * a.OH + oy) * a.OW + ox0 + (nt % NTW) * 16) * COUT;
            const unsigned lc = opaque_u32(st_c);
            auto at = [&](const bf16_t* base) { return (bf16_t*)((char*)const_cast<bf16_t*>(base + ou) + lc); };
            float v[4 * MT];
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[m * 4 + r] = acc[m][t][r];
            // the terms are REQUESTED together and added in the reference's order (residual, res2, res3): a load issued behind the
            // previous term's wait costs one memory round trip per term
            // (wide outputs keep the one-term-at-a-time form: 3 x MT x 2 more registers do not fit beside 8 m-tiles of accumulators)
            constexpr int TM = MT <= 4 ? MT : 1;
            u32x2 tv[3][TM];
            auto load_term = [&](int k, const bf16_t* base) {
#pragma unroll
                for (int m = 0; m < TM; ++m) tv[k][m] = ((const u32x2*)base)[m];
            };
            auto add_term = [&](int k, const bf16_t* base) {
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const u32x2 rv = MT <= 4 ? tv[k][m < TM ? m : 0] : ((const u32x2*)base)[m];
                    v[m * 4 + 0] += bf16_to_f32((bf16_t)(rv.x & 0xffff));
                    v[m * 4 + 1] += bf16_to_f32((bf16_t)(rv.x >> 16));
                    v[m * 4 + 2] += bf16_to_f32((bf16_t)(rv.y & 0xffff));
                    v[m * 4 + 3] += bf16_to_f32((bf16_t)(rv.y >> 16));
                }
            };
            const bf16_t* t3 = a.res3 ? a.res3 + ((size_t)(b * (a.OH >> a.sh3) + (oy >> a.sh3)) * (a.OW >> a.sh3) + (ox >> a.sh3)) * COUT + g * 4 * MT : nullptr;
            if (MT <= 4) {
                if (a.residual) load_term(0, at(a.residual));
                if (a.res2) load_term(1, at(a.res2));
                if (a.res3) load_term(2, t3);
            }
            if (a.residual) add_term(0, at(a.residual));
            if (a.res2) add_term(1, at(a.res2));
            if (a.res3) add_term(2, t3);
            unsigned pk[2 * MT];
#pragma unroll
            for (int i = 0; i < 2 * MT; ++i) pk[i] = pack2(v[2 * i], v[2 * i + 1]);
            if (a.relu) {
#pragma unroll
                for (int i = 0; i < 2 * MT; ++i) pk[i] = relu_pk(pk[i]);
            }
            if (MT == 1) {
                *(u32x2*)at(a.dst) = u32x2{pk[0], pk[1]};
            } else {
#pragma unroll
                for (int q = 0; q < MT / 2; ++q) *(u32x4*)(at(a.dst) + q * 8) = u32x4{pk[4 * q], pk[4 * q + 1], pk[4 * q + 2], pk[4 * q + 3]};
            }
        }
        if (F11) {
            // ---- fused 1x1 follower on the tile just produced (Bottleneck conv1, wasb.py:88-90): the bf16 tile goes through
            // LDS (pixel-major, 128 B per pixel, chunks XOR-swizzled by the pixel index) and comes back as the B operand
            static_assert(!F11 || (COUT == 64 && TH * TW * 64 <= IN_ELEMS + W_ELEMS), "follower needs a 64-channel tile that fits the staging area");
            bf16_t* s_t = s_in;
            __syncthreads();                       // every wave is done with the staging area
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int nt = wave * NT + t;
                const int p = (nt / NTW) * TW + (nt % NTW) * 16 + n;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    u32x4 pk;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const unsigned w = pack2(acc[2 * q + (i >> 1)][t][2 * (i & 1)], acc[2 * q + (i >> 1)][t][2 * (i & 1) + 1]);
                        pk[i] = a.relu ? relu_pk(w) : w;
                    }
                    *(u32x4*)(s_t + p * 64 + (((2 * g + q) ^ (p & 7)) << 3)) = pk;
                }
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int nt = wave * NT + t;
                const int p = (nt / NTW) * TW + (nt % NTW) * 16 + n;
                f32x4 c11[2] = {bias11[0], bias11[1]};
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const bf16x8 bfr = *(const bf16x8*)(s_t + p * 64 + (((4 * k + g) ^ (p & 7)) << 3));
#pragma unroll
                    for (int m = 0; m < 2; ++m) c11[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af11[k][m], bfr, c11[m], 0, 0, 0);
                }
                const int oy = oy0 + nt / NTW, ox = ox0 + (nt % NTW) * 16 + n;
                if (oy >= a.OH || ox >= a.OW) continue;
                *(u32x4*)(a.dst11 + ((size_t)(b * a.OH + oy) * a.OW + ox) * 32 + g * 8) = pack8(c11[0], c11[1], true);
            }
        }
    }
}

// ------------------------------------------------------------------ two stride-2 convs on one input
// Stage 3's fuse layer takes the full-resolution 16-channel branch down twice: 3x3 s2 16 -> 32 (the term of the half-resolution
// output, wasb.py:207-222 with i=1: conv + BN, the running fuse sum and ReLU in the epilogue) and 3x3 s2 16 -> 16 + ReLU (first
// conv of the chain towards the quarter resolution, i=2).  Both are HBM-bound on that 230-MB tensor (8 frames); here ONE
// workgroup pass stages the halo tile once and runs both: one read of the branch instead of two.  Same arithmetic per output
// as conv_mfma_kernel<16, COUT, 3, 2, 4, 32, 8> (same k-steps, same epilogue order).
__global__ __launch_bounds__(512) void conv_s2_pair_kernel(ConvKArgs a) {
    constexpr int CK = 16, KS = 3, S = 2, TH = 4, TW = 32, MTA = 2, MTB = 1;
    constexpr int IH = (TH - 1) * S + KS, IW = (TW - 1) * S + KS;
    constexpr int KSTEPS = 5, PAD = 1;
    constexpr int IN_ELEMS = IH * IW * CK;
    constexpr int IN_UNITS = IH * IW * (CK / 8), IN_PT = (IN_UNITS + 511) / 512;
    constexpr int WA_UNITS = KSTEPS * MTA * 64, WB_UNITS = KSTEPS * MTB * 64;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* s_in = (bf16_t*)smem;
    bf16_t* s_wa = s_in + ((IN_ELEMS + 7) & ~7);
    bf16_t* s_wb = s_wa + WA_UNITS * 8;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, g = lane >> 4;
    const int my_tiles = (a.total_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    StageRegs<WA_UNITS> wa; StageRegs<WB_UNITS> wb;
    stage_load_512<WA_UNITS>(wa, a.wpack, tid);
    stage_load_512<WB_UNITS>(wb, a.wpack_b, tid);
    u32x4 pin[IN_PT];
    unsigned pin_ok = 0u;
    auto issue = [&](int it) {
        const TileAt t = tile_at<TH * S, TW * S, PAD>(xcd_tile(blockIdx.x + it * gridDim.x, a.total_tiles), a.tiles_per_img, a.tiles_x);
        const int b = t.b, gy0 = t.y0, gx0 = t.x0;
#pragma unroll
        for (int k = 0; k < IN_PT; ++k) {
            const int u = tid + k * 512;
            const int c8 = u % (CK / 8), pix = u / (CK / 8);
            const int gy = gy0 + pix / IW, gx = gx0 + pix % IW;
            const bool ok = u < IN_UNITS && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            pin[k] = *(const u32x4*)(ok ? a.src0 + ((size_t)(b * a.H + gy) * a.W + gx) * CK + c8 * 8 : a.src0);      // branch-free: the loads go out together
            pin_ok = ok ? pin_ok | (1u << k) : pin_ok & ~(1u << k);       // zeroed when the unit is written to LDS: a select HERE would wait for the load at once (no prefetch)
        }
    };
    if (my_tiles <= 0) return;          // (workgroup-uniform)
    issue(0);
    stage_store_512<WA_UNITS>(s_wa, wa, tid);
    stage_store_512<WB_UNITS>(s_wb, wb, tid);
    f32x4 bias_a[MTA], bias_b;
#pragma unroll
    for (int m = 0; m < MTA; ++m) bias_a[m] = *(const f32x4*)(a.bias + g * 4 * MTA + m * 4);
    bias_b = *(const f32x4*)(a.bias_b + g * 4);
    // per-lane fragment bases, one per k-step (taps 2s | 2s+1 on lane groups 0-1 | 2-3; the tenth tap is a zero pad)
    const bf16_t* bB[KSTEPS];
#pragma unroll
    for (int k = 0; k < KSTEPS; ++k) {
        int tap = 2 * k + (g >> 1);
        if (tap > 8) tap = 8;
        bB[k] = s_in + lds_off<CK, IW>(tap / KS, n * S + tap % KS, g & 1);
    }
    // the wave's 16-pixel group of the 4x32 tile: row wave / 2, column half wave % 2
    const int r = wave >> 1, cg = wave & 1;
    prefetch_arrived(pin);          // every path into the loop has the prefetch registers complete (see prefetch_arrived)
    for (int it = 0; it < my_tiles; ++it) {
        if (it > 0) __syncthreads();            // every wave finished reading the previous tile
#pragma unroll
        for (int k = 0; k < IN_PT; ++k) {
            const int u = tid + k * 512;
            const bool okk = (pin_ok >> k) & 1u;
            if (u < IN_UNITS) { const int c8 = u % (CK / 8), pix = u / (CK / 8); *(u32x4*)(s_in + lds_off<CK, IW>(pix / IW, pix % IW, c8)) = u32x4{okk ? pin[k].x : 0u, okk ? pin[k].y : 0u, okk ? pin[k].z : 0u, okk ? pin[k].w : 0u}; }
        }
        __syncthreads();
        if (it + 1 < my_tiles) issue(it + 1);
        f32x4 acc_a[MTA] = {bias_a[0], bias_a[1]}, acc_b = bias_b;
#pragma unroll
        for (int s5 = 0; s5 < KSTEPS; ++s5) {
            const bf16x8 bfr = *(const bf16x8*)(bB[s5] + ((r * S) * IW + cg * 16 * S) * CK);
#pragma unroll
            for (int m = 0; m < MTA; ++m) acc_a[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(s_wa + ((s5 * MTA + m) * 64 + lane) * 8), bfr, acc_a[m], 0, 0, 0);
            acc_b = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)(s_wb + (s5 * 64 + lane) * 8), bfr, acc_b, 0, 0, 0);
        }
        prefetch_arrived(pin);          // the next tile's input is waited for in front of this tile's stores
        const int tl = xcd_tile(blockIdx.x + it * gridDim.x, a.total_tiles);
        const int b = tl / a.tiles_per_img, tt = tl % a.tiles_per_img;
        const int oy = (tt / a.tiles_x) * TH + r, ox = (tt % a.tiles_x) * TW + cg * 16 + n;
        if (oy >= a.OH || ox >= a.OW) continue;
        const size_t opix = (size_t)(b * a.OH + oy) * a.OW + ox;
        {   // first conv: 32 outputs, lane holds couts g*8 .. g*8+7; fuse-layer terms in conv_mfma_kernel's order
            const size_t o = opix * 32 + g * 8;
            float v[8];
#pragma unroll
            for (int m = 0; m < MTA; ++m)
#pragma unroll
                for (int q = 0; q < 4; ++q) v[m * 4 + q] = acc_a[m][q];
            auto add_term = [&](const bf16_t* base) { add_bf16x8(v, *(const u32x4*)base); };
            if (a.residual) add_term(a.residual + o);
            if (a.res2) add_term(a.res2 + o);
            if (a.res3) add_term(a.res3 + ((size_t)(b * (a.OH >> a.sh3) + (oy >> a.sh3)) * (a.OW >> a.sh3) + (ox >> a.sh3)) * 32 + g * 8);
            *(u32x4*)(a.dst + o) = pack8(v, a.relu);
        }
        {   // second conv: 16 outputs, lane holds couts g*4 .. g*4+3
            const unsigned w0 = pack2(acc_b[0], acc_b[1]), w1 = pack2(acc_b[2], acc_b[3]);
            *(u32x2*)(a.dst_b + opix * 16 + g * 4) = u32x2{a.relu_b ? relu_pk(w0) : w0, a.relu_b ? relu_pk(w1) : w1};
        }
    }
}

// ------------------------------------------------------------------ launch
template <int CK, int COUT, int KS, int S, int TH, int TW, int NW, bool F11 = false>
static int launch_mfma(const PackedConv& p, const ConvLaunch& l, hipStream_t st) {
    constexpr int MT = COUT / 16;
    constexpr int IH = (TH - 1) * S + KS, IW = (TW - 1) * S + KS;
    constexpr int KSTEPS = (CK == 32) ? KS * KS : (KS * KS + 1) / 2;
    constexpr size_t SMEM = (size_t)(((IH * IW * CK + 7) & ~7) + KSTEPS * MT * 64 * 8) * 2;
    static_assert(SMEM <= 160 * 1024, "LDS budget");
    ConvKArgs a;
    a.src0 = (const bf16_t*)l.src0; a.src1 = (const bf16_t*)l.src1; a.wpack = (const bf16_t*)p.w_dev; a.bias = p.bias_dev;
    a.residual = (const bf16_t*)l.residual; a.dst = (bf16_t*)l.dst;
    a.c0 = p.c0; a.c1 = p.cin_total - p.c0; a.nchunk0 = p.c0 / CK; a.nchunk = p.cin_total / CK;
    a.H = l.h; a.W = l.w; a.OH = (l.h + S - 1) / S; a.OW = (l.w + S - 1) / S;
    a.tiles_x = cdiv(a.OW, TW); a.tiles_per_img = a.tiles_x * cdiv(a.OH, TH); a.total_tiles = a.tiles_per_img * l.batch;
    a.relu = l.relu;
    a.res2 = (const bf16_t*)l.res2; a.res3 = (const bf16_t*)l.res3; a.sh3 = l.sh3;
    if (F11) {
        TTUP_REQUIRE(l.follow && l.follow->cout == 32 && l.follow->cin_total == 64 && l.follow->k == 1 && l.follow->ck == 32 && l.dst2, TTUP_EINVAL, "conv: bad fused 1x1 follower");
        a.w11 = (const bf16_t*)l.follow->w_dev; a.bias11 = l.follow->bias_dev; a.dst11 = (bf16_t*)l.dst2;
    }
    // XCD-aware tile order for the stride-2 convs (env TTUP_S2_XCD=0/1 overrides; the stride-1 full-resolution conv is 5-10 % slower with it)
    static const int s2_xcd = (int)env_ll("TTUP_S2_XCD", 0);
    a.xcd = (S == 2) ? s2_xcd : 0;
    // persistent grid: as many workgroups as can be resident (LDS-limited), each walks its share of the tiles
    const int per_cu = (int)((160 * 1024) / SMEM) > 4 ? 4 : ((int)((160 * 1024) / SMEM) < 1 ? 1 : (int)((160 * 1024) / SMEM));
    return launch_noted(conv_mfma_kernel<CK, COUT, KS, S, TH, TW, NW, F11>, dim3(persistent_grid(a.total_tiles, per_cu)), NW * 64, SMEM, st, a,
                        "conv_mfma_kernel<%d, %d, %d, %d, %d, %d, %d, %s>", CK, COUT, KS, S, TH, TW, NW, F11 ? "true" : "false");
}

// the paired form: 3x3 s2 16 -> 32 (p, with its fuse-layer terms) and 3x3 s2 16 -> 16 (l.pair) on one input
static int launch_s2_pair(const PackedConv& p, const ConvLaunch& l, hipStream_t st) {
    const PackedConv& q = *l.pair;
    TTUP_REQUIRE(p.k == 3 && p.stride == 2 && p.ck == 16 && p.cin_total == 16 && p.cout == 32 && q.k == 3 && q.stride == 2 && q.ck == 16 &&
                 q.cin_total == 16 && q.cout == 16 && l.pair_dst && !l.src1, TTUP_EINVAL, "conv: the paired form is 3x3 s2 16 -> 32 with 3x3 s2 16 -> 16");
    ConvKArgs a;
    a.src0 = (const bf16_t*)l.src0; a.wpack = (const bf16_t*)p.w_dev; a.bias = p.bias_dev; a.residual = (const bf16_t*)l.residual; a.dst = (bf16_t*)l.dst;
    a.res2 = (const bf16_t*)l.res2; a.res3 = (const bf16_t*)l.res3; a.sh3 = l.sh3; a.relu = l.relu;
    a.wpack_b = (const bf16_t*)q.w_dev; a.bias_b = q.bias_dev; a.dst_b = (bf16_t*)l.pair_dst; a.relu_b = l.pair_relu;
    a.H = l.h; a.W = l.w; a.OH = (l.h + 1) / 2; a.OW = (l.w + 1) / 2;
    a.tiles_x = cdiv(a.OW, 32); a.tiles_per_img = a.tiles_x * cdiv(a.OH, 4); a.total_tiles = a.tiles_per_img * l.batch;
    constexpr size_t SMEM = (size_t)(((9 * 65 * 16 + 7) & ~7) + 5 * 3 * 64 * 8) * 2;
    return launch_noted(conv_s2_pair_kernel, dim3(persistent_grid(a.total_tiles, 4)), 512, SMEM, st, a, "conv_s2_pair_kernel");
}

template <int CK, int KS, int S, int TH, int TW>
static int dispatch_cout(const PackedConv& p, const ConvLaunch& l, hipStream_t st) {
    // the stride-2 32 -> 64 conv alone is faster with four-wave workgroups (0.107 against 0.113 ms for its two launches, round 5: twice the
    // workgroups per CU behind its 52-KB staging); every other variant is 5-26 % slower that way
    if constexpr (CK == 32 && S == 2) {
        if (p.cout == 64) return launch_mfma<CK, 64, KS, S, TH, TW, 4>(p, l, st);
    }
    switch (p.cout) {
        case 16: return launch_mfma<CK, 16, KS, S, TH, TW, 8>(p, l, st);
        case 32: return launch_mfma<CK, 32, KS, S, TH, TW, 8>(p, l, st);
        case 64: return launch_mfma<CK, 64, KS, S, TH, TW, 8>(p, l, st);
        case 128: return launch_mfma<CK, 128, KS, S, TH, TW, 8>(p, l, st);
    }
    set_error("conv: cout %d unsupported", p.cout);
    return TTUP_EINVAL;
}

}  // namespace ttup
