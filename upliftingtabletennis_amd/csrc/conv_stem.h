// The fused stem: conv1 + conv2 + Bottleneck conv1 in one persistent kernel.
#pragma once
#include "conv64.h"

namespace ttup {

// ------------------------------------------------------------------ fused stem: conv1 + conv2 (+ Bottleneck conv1)
// Persistent workgroups (8 waves) keep ALL weights of the stem in LDS (conv1 20 KB + conv2 73.7 KB) and walk 8x32 tiles:
//   X0 halo tile (12x36 px, 16 ch, register-prefetched one tile ahead) -> conv1 3x3 9(16)->64 +ReLU on the 10x34 halo
//   region, kept in LDS as bf16 (never written to HBM) -> conv2 3x3 64->64 +ReLU straight from LDS (18 k-steps without a
//   barrier) -> T2 tile to HBM and, still in registers, into the 1x1 64->32 follower (Bottleneck conv1) -> A1 tile to HBM.
// Reference: wasb.py:446-451 (stem), :88-90 (Bottleneck conv1).  Intermediates are rounded to bf16 where the layer-wise
// path stores them, so results are bit-identical.
struct StemArgs {
    const bf16_t* x0 = nullptr;       // (B,H,W,16), or in frames mode (NF > 0) the pre-processed frames (B+NF-1,H,W,4): sample b = frames b..b+NF-1
    const bf16_t* w1 = nullptr; const float* b1 = nullptr;      // conv1: CK=16 packing, 5 k-steps x 4 m-tiles
    const bf16_t* w2 = nullptr; const float* b2 = nullptr;      // conv2: CK=32 packing, 2 chunks x 9 k-steps x 4 m-tiles
    const bf16_t* w3 = nullptr; const float* b3 = nullptr;      // follower 1x1 64->32: 2 k-steps x 2 m-tiles
    bf16_t* t2 = nullptr; bf16_t* a1 = nullptr;
    int H = 0, W = 0, tiles_x = 0, tiles_per_img = 0, total_tiles = 0;
};

// NF = 0: X0 comes as (B,H,W,16) records.  NF = 1 / 3 (frames mode): every frame is pre-processed ONCE into a 4-channel record
// (3 colours + 0) and a sample's X0 pixel is assembled in LDS from the NF frames it spans (slot f*4 + c; conv1's weights are
// packed in that channel order): the 16-channel per-triple tensor -- 3 copies of every frame plus 7 zero channels -- is never
// written or read (28.8 -> 7.2 MB of pre-processing output per frame, 28.8 -> 21.6 MB of stem input).
// K4 (NF = 3 only, round 5): conv1 in FOUR k-steps instead of five.  The X0 pixel record is the three frames' (B, G, R, 0) slots back to
// back -- 12 slots, 24 bytes -- so the three pixels under a tap row are 36 CONTIGUOUS slots of LDS: conv1's K dimension becomes
// 3 tap rows x 40 slots (36 + 4 that carry zero weights) = 120 -> 128 = 4 k-steps of 32, a fragment = 8 consecutive slots of one row
// (two 8-byte LDS reads: the records are 8-byte aligned).  The 16-slot records (each frame's 4 slots + 4 zero slots, two taps per
// k-step) need 5 k-steps for the 81 real products: 20 % of conv1's MFMAs and 4 KB of its weights gone.  Weights: StemArgs::w1 packed
// as a "1x1 conv with 128 inputs" in that slot order (csrc/wasb_graph.h).  Another fp32 summation order than the 5-step form (and
// than the layer-wise conv): results agree to bf16 rounding flips, like the other fused kernels (tests/test_gpu_parity.py).
template <int NF, bool K4 = false>
__global__ __launch_bounds__(512) void stem_kernel(StemArgs a) {
    static_assert(!K4 || NF == 3, "the 4-step conv1 is the three-frame form");
    constexpr int XH = 12, XW = 36, TH1 = 10, TW1 = 34, NP1 = TH1 * TW1;       // X0 region, conv1 output region
    constexpr int KS1 = K4 ? 4 : 5;                                              // conv1 k-steps
    constexpr int XS = K4 ? 12 : 16;                                             // slots per X0 pixel record
    constexpr int W1_U = KS1 * 4 * 64, W2_U = 2 * 9 * 4 * 64;                    // 16-byte units
    constexpr int X_UNITS = NF ? XH * XW * NF : XH * XW * 2;                    // 8-byte (frames mode) or 16-byte units
    constexpr int X_PT = (X_UNITS + 511) / 512;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* s_w1 = (bf16_t*)smem;                     // 20,480 B (16,384 B with K4)
    bf16_t* s_w2 = s_w1 + W1_U * 8;                   // 73,728 B
    bf16_t* s_t1 = s_w2 + W2_U * 8;                   // [2 chunks][340 px][32 ch]  43,520 B
    bf16_t* s_x = s_t1 + 2 * NP1 * 32;                // [432 px][16 slots] 13,824 B; K4: [432 px][12 slots] + 16 B of pad (the last fragment of the last pixel reads 4 slots past it)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;          // (as a scalar -- readfirstlane -- the wave-dependent loops become branches: measured +3 ... 5 %)
    const int n = lane & 15, g = lane >> 4;
    StageRegs<W1_U> w1regs; StageRegs<W2_U> w2regs;
    stage_load_512<W1_U>(w1regs, a.w1, tid);            // stored to LDS after the first tile's loads have been issued (below)
    stage_load_512<W2_U>(w2regs, a.w2, tid);
    // Follower weights with the K order permuted to the conv2 accumulator layout (follower_frag): the T2 tile never goes through LDS
    bf16x8 af3[2][2];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int m = 0; m < 2; ++m) af3[k][m] = follower_frag<2>(a.w3, k, m, n, g);
    // biases seed the accumulators (lane's channels g*16.. for the 64-channel convs, g*8.. for the follower)
    f32x4 b1[4], b2[4], b3[2];
#pragma unroll
    for (int m = 0; m < 4; ++m) { b1[m] = *(const f32x4*)(a.b1 + g * 16 + m * 4); b2[m] = *(const f32x4*)(a.b2 + g * 16 + m * 4); }
#pragma unroll
    for (int m = 0; m < 2; ++m) b3[m] = *(const f32x4*)(a.b3 + g * 8 + m * 4);
    // conv1 per-lane tap offsets inside the X0 tile (CK=16: k-step s covers taps 2s and 2s+1)
    int koff1[KS1];
#pragma unroll
    for (int s5 = 0; s5 < KS1; ++s5) {
        if (K4) {          // k = 32 s + 8 g + j = 40 * (tap row) + slot: fragment (s, g) = slots o0 .. o0+7 of row r; k >= 120 carries zero weights (any valid address)
            const int kk0 = 32 * s5 + 8 * g, r = kk0 / 40, o0 = kk0 % 40;
            koff1[s5] = r < 3 ? r * XW * XS + o0 : 0;
        } else {
            int tap = 2 * s5 + (g >> 1); tap = tap > 8 ? 8 : tap; koff1[s5] = ((tap / 3) * XW + tap % 3) * 16 + (g & 1) * 8;
        }
    }
    // conv2 per-lane fragment bases inside one chunk plane of the T1 tile, one per tap column
    const bf16_t* bB[3];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) bB[dx] = s_t1 + lds_off<32, TW1>(0, n + dx, g);

    const int my_tiles = (a.total_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    u32x4 px[NF ? 1 : 2];
    u32x2 pf[NF ? X_PT : 1];
    if (NF) {         // slots no frame writes (the fourth record of a triple, three of four for a single frame; K4: the pad behind the tile) stay zero
        for (int u = tid; u < (K4 ? (XH * XW * XS * 2 + 16) / 16 : XH * XW * 2); u += 512) ((u32x4*)s_x)[u] = u32x4{0u, 0u, 0u, 0u};
        __syncthreads();
    }
    // NF: byte offsets of the thread's (pixel, frame) records from the tile's first halo pixel in the triple's first frame (explained at issue_in of bb_chain_kernel, conv_bb.h)
    unsigned xoff[NF ? X_PT : 1];
    if constexpr (NF != 0) {
#pragma unroll
        for (int k = 0; k < X_PT; ++k) {
            const int u = tid + k * 512;
            const int f = u % (NF ? NF : 1), pix = u / (NF ? NF : 1);
            xoff[k] = u < X_UNITS ? (unsigned)(((f * a.H + pix / XW) * a.W + pix % XW) * 8) : 0u;
        }
    }
    auto issue = [&](int it) {
        const TileAt t = tile_at<8, 32, 2>(xcd_tile(blockIdx.x + it * gridDim.x, a.total_tiles), a.tiles_per_img, a.tiles_x);
        const int b = t.b, gy0 = t.y0, gx0 = t.x0;
        if (NF) {
            if (gy0 >= 0 && gy0 + XH <= a.H && gx0 >= 0 && gx0 + XW <= a.W) {          // halo tile inside the image: scalar base + lane constants
                const char* base = (const char*)(a.x0 + (((size_t)b * a.H + gy0) * a.W + gx0) * 4);
#pragma unroll
                for (int k = 0; k < X_PT; ++k) pf[k] = *(const u32x2*)(base + opaque_u32(xoff[k]));
                return;
            }
#pragma unroll
            for (int k = 0; k < X_PT; ++k) {
                const int u = tid + k * 512;
                const int f = u % (NF ? NF : 1), pix = u / (NF ? NF : 1);
                const int gy = gy0 + pix / XW, gx = gx0 + pix % XW;
                pf[k] = u32x2{0u, 0u};
                if (u < X_UNITS && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
                    pf[k] = *(const u32x2*)(a.x0 + (((size_t)(b + f) * a.H + gy) * a.W + gx) * 4);
            }
            return;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int u = tid + k * 512;
            const int c8 = u & 1, pix = u >> 1;
            const int gy = gy0 + pix / XW, gx = gx0 + pix % XW;
            px[k & (NF ? 0 : 1)] = u32x4{0u, 0u, 0u, 0u};
            if (u < X_UNITS && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
                px[k & (NF ? 0 : 1)] = *(const u32x4*)(a.x0 + ((size_t)(b * a.H + gy) * a.W + gx) * 16 + c8 * 8);
        }
    };
    // The X0 tile of tile it+1 is committed to LDS in the MIDDLE of iteration it: behind the barrier that ends conv1 (the last
    // reader of the X0 buffer) and BEFORE conv2's epilogue issues its stores, and the loads of tile it+2 are requested right there.
    // Committed at the loop top -- behind the epilogue -- the wait for the prefetched loads was an s_waitcnt vmcnt(0) that also
    // drained the T2 / A1 stores just issued (the counter retires in order, and the compiler cannot count stores that sit behind
    // a branch): 2.7 k of the tile's 11.9 k cycles with every wave of the CU parked (round 5).
    auto commit = [&]() {
        if (NF) {
#pragma unroll
            for (int k = 0; k < X_PT; ++k) {
                const int u = tid + k * 512;
                if (u < X_UNITS) *(u32x2*)(s_x + (u / (NF ? NF : 1)) * XS + (u % (NF ? NF : 1)) * 4) = pf[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) { const int u = tid + k * 512; if (u < X_UNITS) ((u32x4*)s_x)[u] = px[k & (NF ? 0 : 1)]; }
        }
    };
    // T2 tile to HBM; follower A1 = relu(W3 . T2 + b3), 64 -> 32, straight from the packed registers
    auto epilogue = [&](const f32x4 (&acc)[4][2], int b, int oy0, int ox0) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int r = 2 * (wave >> 1) + t, cg = wave & 1;
            const int oy = oy0 + r, ox = ox0 + cg * 16 + n;
            const bool ok = oy < a.H && ox < a.W;
            u32x4 pk[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                pk[q] = pack8(acc[2 * q][t], acc[2 * q + 1][t], true);
                if (ok) *(u32x4*)(a.t2 + ((size_t)(b * a.H + oy) * a.W + ox) * 64 + g * 16 + q * 8) = pk[q];
            }
            f32x4 c3[2] = {b3[0], b3[1]};
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int m = 0; m < 2; ++m) c3[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af3[k][m], __builtin_bit_cast(bf16x8, pk[k]), c3[m], 0, 0, 0);
            if (ok) *(u32x4*)(a.a1 + ((size_t)(b * a.H + oy) * a.W + ox) * 32 + g * 8) = pack8(c3[0], c3[1], true);
        }
    };
    constexpr bool STAGGER = K4;
    const bool late = __builtin_amdgcn_readfirstlane(wave) >= 4;
    f32x4 acc[4][2];
    int eb = 0, eoy0 = 0, eox0 = 0;
    bool pending = false;
    if (my_tiles <= 0) return;          // (workgroup-uniform; the launcher never starts more workgroups than tiles)
    issue(0);
    stage_store_512<W1_U>(s_w1, w1regs, tid);
    stage_store_512<W2_U>(s_w2, w2regs, tid);
    commit();                           // unconditional: its wait retires every older load (biases, follower fragments) on every path into the loop
    if (my_tiles > 1) issue(1);
    for (int it = 0; it < my_tiles; ++it) {
        const TileAt tile = tile_at<8, 32>(xcd_tile(blockIdx.x + it * gridDim.x, a.total_tiles), a.tiles_per_img, a.tiles_x);
        const int b = tile.b, oy0 = tile.y0, ox0 = tile.x0;
        const bool t1_inside = oy0 >= 1 && oy0 + 9 <= a.H && ox0 >= 1 && ox0 + 33 <= a.W;          // the whole 10x34 conv1 region lies inside the image
        // ONE barrier covers "X0 tile complete" (committed in the middle of the previous iteration) and "previous conv2 done reading
        // the T1 tile" (and the weights on the first pass)
        __syncthreads();
        // ---------------- conv1 on the 10x34 region (22 groups of 16 pixels, linear pixel index)
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int j = wave + 8 * t;
            if (j >= 22) continue;
            const int p = j * 16 + n, pc = p < NP1 ? p : NP1 - 1;
            const int y = pc / TW1, x = pc % TW1;
            const bf16_t* xb = s_x + (y * XW + x) * XS;
            f32x4 acc[4] = {b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
            for (int s5 = 0; s5 < KS1; ++s5) {
                bf16x8 bfr;
                if (K4) {          // 8-byte aligned: two ds_read_b64
                    const u32x2 lo = *(const u32x2*)(xb + koff1[s5]), hi = *(const u32x2*)(xb + koff1[s5] + 4);
                    bfr = __builtin_bit_cast(bf16x8, u32x4{lo.x, lo.y, hi.x, hi.y});
                } else bfr = *(const bf16x8*)(xb + koff1[s5]);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const bf16x8 af = *(const bf16x8*)(s_w1 + ((s5 * 4 + m) * 64 + lane) * 8);
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr, acc[m], 0, 0, 0);
                }
            }
            if (p < NP1) {
                // conv2's zero padding: conv1 outputs outside the image are zeros.  Only border tiles have any (wave-uniform test on the
                // scalar unit): interior tiles skip the per-lane position test and the eight selects per pixel group (round 5: the
                // vector issue port is what these kernels run out of)
                const int gy = oy0 - 1 + y, gx = ox0 - 1 + x;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    u32x4 pk = pack8(acc[2 * q], acc[2 * q + 1], true);
                    if (!t1_inside) {
                        const bool inside = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
#pragma unroll
                        for (int i = 0; i < 4; ++i) pk[i] = inside ? pk[i] : 0u;
                    }
                    // lane's channels g*16 + q*8 .. +7  ->  chunk plane (g>>1), 16-byte chunk (g&1)*2+q
                    *(u32x4*)(s_t1 + (g >> 1) * (NP1 * 32) + lds_off<32, TW1>(y, x, (g & 1) * 2 + q)) = pk;
                }
            }
        }
        __syncthreads();
        commit();                                        // conv1 was the X0 buffer's last reader; unconditional (see conv64_kernel): on the last tile a stale image nobody reads
        if (it + 2 < my_tiles) issue(it + 2);
        // ---------------- conv2 on the 8x32 tile, both 32-channel planes straight from LDS
        // STAGGER (waves 4-7, the second wave of every SIMD): the epilogue of a tile is deferred to the start of the NEXT tile's conv2
        // phase, so it runs under the partner wave's MFMA loop instead of beside the partner's own epilogue (both waves of a SIMD
        // otherwise leave the matrix pipe idle together); the accumulators stay in registers across the tile boundary
        if (STAGGER && late && pending) epilogue(acc, eb, eoy0, eox0);
#pragma unroll
        for (int m = 0; m < 4; ++m) { acc[m][0] = b2[m]; acc[m][1] = b2[m]; }
        static_assert(TW1 == 34 && NP1 == 340, "conv64_tile_mfma's tile");
        conv64_tile_mfma(acc, bB, s_w2, wave, lane);
        if (STAGGER && late) { eb = b; eoy0 = oy0; eox0 = ox0; pending = true; }
        else epilogue(acc, b, oy0, ox0);
    }
    if (STAGGER && late && pending) epilogue(acc, eb, eoy0, eox0);
}

}  // namespace ttup
