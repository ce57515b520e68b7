// The fused Bottleneck tail + transition1.
#pragma once
#include "conv_dev.h"
#include "conv.h"

namespace ttup {

// ------------------------------------------------------------------ fused Bottleneck tail + transition1
// One workgroup (8 waves) produces an 8x32 tile of transition1[0] (3x3 s1 128->16) and the matching 4x16 tile of
// transition1[1] (3x3 s2 128->32) without the 128-channel layer1 tensor ever leaving the CU:
//   phase 1  layer1 = relu(conv3(A2) + downsample(T2) + b) on the 10x34 halo tile (1x1, K = 32+64, 128 couts),
//            rounded to bf16 into LDS exactly as the unfused path rounds it into HBM;
//   phase 2a 3x3 s1 over the LDS tile -> B0;   phase 2b 3x3 s2 over the same tile -> B1.
// Reference: wasb.py:96-105 (conv3/bn3 + downsample + add + relu), :454-459 (transition1).
struct FusedArgs {
    const bf16_t* a2 = nullptr; const bf16_t* t2 = nullptr;       // (B,H,W,32), (B,H,W,64)
    const bf16_t* w1 = nullptr; const float* b1 = nullptr;        // two-source 1x1 -> 128 (3 chunks)
    const bf16_t* w5 = nullptr; const float* b5 = nullptr;        // 3x3 s1 128 -> 16 (4 chunks x 9 steps)
    const bf16_t* w6 = nullptr; const float* b6 = nullptr;        // 3x3 s2 128 -> 32 (4 chunks x 9 steps x 2 m-tiles)
    bf16_t* b0 = nullptr; bf16_t* b1o = nullptr;
    int H = 0, W = 0, tiles_x = 0, tiles_per_img = 0, total_tiles = 0;
};

__device__ __forceinline__ int l1_off(int pix, int c8) { return pix * 128 + ((c8 ^ (pix & 15)) << 3); }
__device__ __forceinline__ int st_off(int pix, int c8) { return pix * 32 + ((c8 ^ ((4 - ((pix >> 2) & 3)) & 3)) << 3); }

// No weight traffic inside the tile loop: W1 and W5 stay in LDS for the life of the workgroup; the 3x3/s2 conv (phase 2b)
// is split over K instead of over output rows -- wave (cc, m) keeps the nine W6 fragments of its 32-channel chunk cc and
// m-tile m in REGISTERS for all tiles and accumulates partial sums for all four output rows (four independent MFMA
// chains); the partials meet in LDS (in the L1 tile's storage once every wave is done reading it) and wave (m, r)
// reduces row r.  Four barriers per tile.  The fp32 summation order of phase 2b (four partial sums) differs from the
// layer-wise kernel's, everything else is the same arithmetic.
__global__ __launch_bounds__(512) void bneck_trans_kernel(FusedArgs a) {
    constexpr int IH = 10, IW = 34, NPIX = IH * IW;            // 340 halo pixels
    constexpr int NT1 = 22;
    constexpr int W1_U = 3 * 8 * 64, W5_U = 4 * 9 * 64;         // 16-byte units
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* s_l1 = (bf16_t*)smem;                               // [340][128]  87,040 B  (phase-2b partial sums alias its first 32 KB)
    bf16_t* s_w1 = s_l1 + NPIX * 128;                           // 24,576 B resident
    bf16_t* s_w5 = s_w1 + W1_U * 8;                             // 36,864 B resident
    float* s_b1 = (float*)(s_w5 + W5_U * 8);                    // 512 B
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;          // (as a scalar -- readfirstlane -- the wave-dependent loops become branches: measured +3 ... 5 %)
    const int n = lane & 15, g = lane >> 4;
    StageRegs<W1_U> w1regs; StageRegs<W5_U> w5regs;
    stage_load_512<W1_U>(w1regs, a.w1, tid);            // stored to LDS after the first tile's loads have been issued (below)
    stage_load_512<W5_U>(w5regs, a.w5, tid);
    const float b1v = tid < 128 ? a.b1[tid] : 0.f;
    const int cc = wave & 3, m6 = wave >> 2;
    bf16x8 af6[9];
#pragma unroll
    for (int s9 = 0; s9 < 9; ++s9) af6[s9] = *(const bf16x8*)(a.w6 + (((cc * 9 + s9) * 2 + m6) * 64 + lane) * 8);
    const f32x4 bias6 = *(const f32x4*)(a.b6 + g * 8 + m6 * 4);
    const f32x4 b5 = *(const f32x4*)(a.b5 + g * 4);
    const int my_tiles = (a.total_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;

    u32x4 pb[3][3];
    bool p_in[3];
    // the lane's three halo pixels as (row << 8 | column), one register each, unpacked inside issue_pix behind an opaque copy: left to
    // itself the compiler hoists the six quotients / remainders out of the tile loop and, at 256 registers, spills them -- and a
    // spill's reload inside issue_pix is a scratch load whose s_waitcnt vmcnt(0) drains the stores in front of it
    unsigned pyx[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        int pix = (wave + 8 * t) * 16 + n;
        pix = pix < NPIX ? pix : NPIX - 1;
        pyx[t] = (unsigned)((pix / IW) << 8 | (pix % IW));
    }
    // byte offset of the lane's 16-byte unit of pixel group t from the tile's first halo pixel in the 32-channel source (twice that, plus
    // 64 per chunk, in the 64-channel one): the same for every tile (explained at issue_in of bb_chain_kernel, conv_bb.h)
    unsigned poff[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) poff[t] = (unsigned)(((pyx[t] >> 8) * a.W + (pyx[t] & 255u)) * 64 + g * 16);
    auto issue_pix = [&](int it) {
        const TileAt t = tile_at<8, 32, 1>(xcd_tile(blockIdx.x + it * gridDim.x, a.total_tiles), a.tiles_per_img, a.tiles_x);
        const int b = t.b, gy0 = t.y0, gx0 = t.x0;
        if (gy0 >= 0 && gy0 + IH <= a.H && gx0 >= 0 && gx0 + IW <= a.W) {          // halo tile inside the image: scalar bases + lane constants
            const size_t gp0 = (size_t)(b * a.H + gy0) * a.W + gx0;
            const char* base_a = (const char*)(a.a2 + gp0 * 32);
            const char* base_t = (const char*)(a.t2 + gp0 * 64);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                p_in[t] = wave + 8 * t < NT1;          // (groups past the tile: clamped to its last pixel, loaded and never used)
                const unsigned o = opaque_u32(poff[t]), o2 = o * 2u - (unsigned)(g * 16);
                pb[t][0] = *(const u32x4*)(base_a + o);
                pb[t][1] = *(const u32x4*)(base_t + o2);
                pb[t][2] = *(const u32x4*)(base_t + o2 + 64);
            }
            return;
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int j = wave + 8 * t;
            unsigned q = pyx[t];
            asm volatile("" : "+v"(q));
            const int gy = gy0 + (int)(q >> 8), gx = gx0 + (int)(q & 255u);
            p_in[t] = j < NT1 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            const size_t gp = (size_t)(b * a.H + gy) * a.W + gx;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                pb[t][c] = u32x4{0u, 0u, 0u, 0u};
                if (p_in[t]) pb[t][c] = (c == 0) ? *(const u32x4*)(a.a2 + gp * 32 + g * 8) : *(const u32x4*)(a.t2 + gp * 64 + (c - 1) * 32 + g * 8);
            }
        }
    };
    if (my_tiles <= 0) return;          // (workgroup-uniform; the launcher never starts more workgroups than tiles)
    issue_pix(0);
    stage_store_512<W1_U>(s_w1, w1regs, tid);
    stage_store_512<W5_U>(s_w5, w5regs, tid);
    if (tid < 128) s_b1[tid] = b1v;
    // every path into the tile loop has the prefetch registers COMPLETE (here: the first tile's; inside the loop: prefetch_arrived in
    // front of phase 2a's stores) -- a path on which they might be pending would put an s_waitcnt vmcnt(0) at the top of every tile
    prefetch_arrived(pb[0]); prefetch_arrived(pb[1]); prefetch_arrived(pb[2]);

    for (int it = 0; it < my_tiles; ++it) {
        const TileAt tile = tile_at<8, 32>(xcd_tile(blockIdx.x + it * gridDim.x, a.total_tiles), a.tiles_per_img, a.tiles_x);
        const int b = tile.b, oy0 = tile.y0, ox0 = tile.x0;
        __syncthreads();            // previous tile's reduction has read its partial sums (weights visible on the first pass)
        // ---------------- phase 1: layer1 halo tile.  Output-channel pairs outermost: a weight fragment read from LDS serves all
        // (up to three) pixel groups of the wave -- 24 fragment reads per wave and tile instead of 72 (the kernel is LDS-bound);
        // every accumulator still sums its three K chunks in the same order
        // (pipelined like conv64_tile_mfma: the two weight fragments of step (q, chunk) + 1 -- and the next pair's bias -- are requested
        // before the MFMAs of step (q, chunk))
        bf16x8 afp[2][2];
        f32x4 bqp[2][2];
        auto load_w1 = [&](int st, bf16x8 (&a2)[2]) __attribute__((always_inline)) {          // st = q * 3 + chunk
            const int q = st / 3, chunk = st % 3;
            a2[0] = *(const bf16x8*)(s_w1 + ((chunk * 8 + 2 * q) * 64 + lane) * 8);
            a2[1] = *(const bf16x8*)(s_w1 + ((chunk * 8 + 2 * q + 1) * 64 + lane) * 8);
        };
        auto load_bq = [&](int q, f32x4 (&b2)[2]) __attribute__((always_inline)) {
            b2[0] = *(const f32x4*)(s_b1 + g * 32 + q * 8); b2[1] = *(const f32x4*)(s_b1 + g * 32 + q * 8 + 4);
        };
        load_w1(0, afp[0]);
        load_bq(0, bqp[0]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 acc[3][2];
            const f32x4 bq0 = bqp[q & 1][0], bq1 = bqp[q & 1][1];
#pragma unroll
            for (int t = 0; t < 3; ++t) { acc[t][0] = bq0; acc[t][1] = bq1; }
#pragma unroll
            for (int chunk = 0; chunk < 3; ++chunk) {
                const int st = q * 3 + chunk;
                if (st + 1 < 12) load_w1(st + 1, afp[(st + 1) & 1]);
                if (chunk == 0 && q + 1 < 4) load_bq(q + 1, bqp[(q + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                const bf16x8 af0 = afp[st & 1][0], af1 = afp[st & 1][1];
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    if (wave + 8 * t >= NT1) continue;             // wave-uniform: waves 6 and 7 own two groups
                    const bf16x8 bfr = __builtin_bit_cast(bf16x8, pb[t][chunk]);
                    acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af0, bfr, acc[t][0], 0, 0, 0);
                    acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af1, bfr, acc[t][1], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int j = wave + 8 * t, pix = j * 16 + n;
                if (j >= NT1 || pix >= NPIX) continue;
                const bool inside = p_in[t];
                u32x4 pk;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const unsigned w = relu_pk(pack2(acc[t][i >> 1][2 * (i & 1)], acc[t][i >> 1][2 * (i & 1) + 1]));
                    pk[i] = inside ? w : 0u;          // (a wave-uniform "interior tile" branch around these selects measured +1 % here, -2 % in the stem)
                }
                *(u32x4*)(s_l1 + l1_off(pix, g * 4 + q)) = pk;
            }
        }
        __syncthreads();
        if (it + 1 < my_tiles) issue_pix(it + 1);               // next tile's pixel fragments: in flight during phases 2a and 2b
        // ---------------- phase 2a: 3x3 s1 128 -> 16 on the LDS tile.  A wave owns two VERTICALLY adjacent 16-pixel groups
        // (rows 2q, 2q+1 of column half ch): the four input rows they touch are read once per (chunk, tap column) and
        // shared by both outputs -- 4 fragment reads instead of 6.
        {
            const int q2 = wave >> 1, ch = wave & 1;
            f32x4 acc[2] = {b5, b5};
            // pipelined like conv64_tile_mfma: the seven fragments of (chunk, tap column) group j+1 are requested before the six MFMAs
            // of group j, and a scheduling barrier keeps the requests there (same k order per accumulator): phase 2a 5.2 k -> 4.7 k cycles,
            // the kernel -3 % (round 5).  It needs 28 more registers than the plain loop: with the 48 swizzled fragment addresses hoisted out
            // of the tile loop the kernel spilled lane constants of issue_pix, whose reloads (scratch loads) put an s_waitcnt vmcnt(0)
            // behind the tile's stores -- hence the opaque column below
            bf16x8 brow[2][4], af[2][3];
            // Swizzled fragment addresses from NINE lane constants instead of 48: pixel P0 + rr * 34 + dx has (pixel & 15) = (P0 + t) & 15
            // with t = 2 rr + dx (34 = 2 mod 16), and chunk (4 c + g) ^ (pixel & 15) = (g ^ (pixel & 15)) ^ (c << 2): the byte address is
            // (bt[t] ^ (c << 6)) + (rr * 34 + dx) * 256 with bt[t] = P0 * 256 + ((g ^ ((P0 + t) & 15)) << 4) -- one v_xor per read, the
            // rest an instruction immediate.  (Written out through l1_off the compiler either hoists 48 addresses out of the tile loop,
            // which spills, or recomputes each with five integer instructions: +240 vector instructions per tile in a kernel whose
            // vector issue port is as busy as its matrix pipe.)
            unsigned bt[9];
            {
                const int P0 = (2 * q2) * IW + ch * 16 + n;
#pragma unroll
                for (int t = 0; t < 9; ++t) bt[t] = (unsigned)(P0 * 256) + (unsigned)(((g ^ ((P0 + t) & 15)) & 15) << 4);
            }
            auto load_group = [&](int j, bf16x8 (&br)[4], bf16x8 (&a3)[3]) __attribute__((always_inline)) {
                const int c = j / 3, dx = j % 3;
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) br[rr] = *(const bf16x8*)((const char*)s_l1 + (bt[2 * rr + dx] ^ (unsigned)(c << 6)) + (rr * IW + dx) * 256);
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) a3[dy] = *(const bf16x8*)(s_w5 + ((c * 9 + dy * 3 + dx) * 64 + lane) * 8);
            };
            load_group(0, brow[0], af[0]);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                if (j + 1 < 12) load_group(j + 1, brow[(j + 1) & 1], af[(j + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[j & 1][dy], brow[j & 1][dy], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[j & 1][dy], brow[j & 1][dy + 1], acc[1], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int oy = oy0 + 2 * q2 + t, ox = ox0 + ch * 16 + n;
                if (oy < a.H && ox < a.W)
                    *(u32x2*)(a.b0 + ((size_t)(b * a.H + oy) * a.W + ox) * 16 + g * 4) =
                        u32x2{relu_pk(pack2(acc[t][0], acc[t][1])), relu_pk(pack2(acc[t][2], acc[t][3]))};
            }
        }
        // ---------------- phase 2b: 3x3 s2 128 -> 32, K-chunk cc / m-tile m6 of all four output rows
        f32x4 part[4];
        {
            const f32x4 seed = cc == 0 ? bias6 : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < 4; ++r) part[r] = seed;
#pragma unroll
            for (int s9 = 0; s9 < 9; ++s9) {
                const int dy = s9 / 3, dx = s9 % 3;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int pix = (2 * r + dy) * IW + 2 * n + dx;
                    const bf16x8 bfr = *(const bf16x8*)(s_l1 + l1_off(pix, cc * 4 + g));
                    part[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af6[s9], bfr, part[r], 0, 0, 0);
                }
            }
        }
        __syncthreads();            // every wave is done reading the L1 tile: its storage now carries the partial sums
        {
            float* s_part = (float*)s_l1;
#pragma unroll
            for (int r = 0; r < 4; ++r) *(f32x4*)(s_part + (((m6 * 4 + cc) * 4 + r) * 64 + lane) * 4) = part[r];
        }
        __syncthreads();
        {
            const float* s_part = (const float*)s_l1;
            const int mr = wave >> 2, rr = wave & 3;            // this wave reduces m-tile mr, output row rr
            f32x4 v = *(const f32x4*)(s_part + (((mr * 4 + 0) * 4 + rr) * 64 + lane) * 4);
#pragma unroll
            for (int c = 1; c < 4; ++c) v += *(const f32x4*)(s_part + (((mr * 4 + c) * 4 + rr) * 64 + lane) * 4);
            const int OH = (a.H + 1) >> 1, OW = (a.W + 1) >> 1;
            const int oy = (oy0 >> 1) + rr, ox = (ox0 >> 1) + n;
            // The next tile's pixel fragments (requested at the start of phase 2a) are waited for HERE, in front of the tile's LAST stores:
            // at the top of the next tile, behind them, the wait is an s_waitcnt vmcnt(0) that drains those stores as well
            // (prefetch_arrived; unconditional: behind a branch the compiler would wait again at the top).  Not earlier: under load a
            // read takes ~5 k cycles to come back (phase stamps, round 5: phase 2a lasted 5.2 k cycles with or without its MFMAs and LDS
            // reads while the wait stood at its end) -- phases 2a, 2b and the two barriers together cover that, phase 2a alone does not.
            prefetch_arrived(pb[0]); prefetch_arrived(pb[1]); prefetch_arrived(pb[2]);
            if (oy < OH && ox < OW)
                *(u32x2*)(a.b1o + ((size_t)(b * OH + oy) * OW + ox) * 32 + g * 8 + mr * 4) = u32x2{relu_pk(pack2(v[0], v[1])), relu_pk(pack2(v[2], v[3]))};
        }
    }
}

}  // namespace ttup
