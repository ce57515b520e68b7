// The uplift forward's fused layer halves on split-bf16 operands: the MLP block (two forms), the qkv block, the short-sequence attention block.
// Private to csrc/uplift.hip, which includes it after uplift_x3.h inside its no-packed-fp32 region; no other unit may include it.
#pragma once

namespace {

// The token-local half of SimpleStaticLayer.forward (model.py:295-298) in ONE kernel, D = 128:
//     x2 = proj(att) + x;   hid = relu(fc1(LN(x2)));   x = fc2(hid) + x2
// Three chained 128 x 128 GEMMs (split-bf16 operands as in linear_x3_kernel) on a tile of 64 tokens; x2 stays in the registers of
// the lanes that produced it (the three GEMMs share one tiling, so the residual of the last one is already in place), LN(x2) and hid
// go through LDS, nothing but `att` and `x` is read and nothing but `x` written: 1.5 KB of HBM traffic per token instead of the
// 4.1 KB of the three separate launches (proj -> x2, fc1 -> hid, fc2 -> x), which at B = 10 000 trajectories are HBM-bound.
struct MlpArgs {
    const float* att; float* x; long long M;
    const uint16_t* w_proj; const uint16_t* w_fc1; const uint16_t* w_fc2;
    const float* g2; const float* b2; const float* bias1; const float* bias2;
};
__global__ __launch_bounds__(256) void mlp_block_x3_kernel(MlpArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t xh[];      // [3][BM][128] split planes, then float s2[BM][132]
    constexpr int BM = 64, K = 128, PLANE = BM * K, KS = K / 32, NTW = 2;
    static_assert(K == X3_K, "the uplift_x3.h blocks are written for 128-wide rows");
    float* s2 = (float*)(xh + 3 * PLANE);                              // [BM][128] fp32, 16-byte chunks XOR-swizzled with the row's low 4 bits
    // (512-byte rows alias on the banks: the swizzle spreads the 8 rows of a ds_write_b128 lane group over 8 chunks; 80 KB per
    // 64-token workgroup = two per CU, 160 KB per 128-token workgroup)
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6, wn = wave & 3, wm = wave >> 2;
    const long long m0 = (long long)ttup_bid_x() * BM;
    const int q = lane >> 4, c = lane & 15;
    const int grp = tid >> 4, l16 = tid & 15;
    auto gemm = [&](const uint16_t* __restrict__ w3, f32x4 (&acc)[NTW][4]) __attribute__((always_inline)) {
        const uint16_t* xw = xh + (wm * 64 + c) * K;
        bf16x8 wa[3][NTW];
#pragma unroll
        for (int t = 0; t < NTW; ++t)
#pragma unroll
            for (int p = 0; p < 3; ++p) wa[p][t] = *(const bf16x8*)(w3 + ((((size_t)(wn + 4 * t) * KS) * 3 + p) * 64 + lane) * 8);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            bf16x8 xb[3][4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int p = 0; p < 3; ++p) xb[p][mt] = *(const bf16x8*)(xw + p * PLANE + mt * 16 * K + (((4 * s + q) ^ c) << 3));
            bf16x8 wn_[3][NTW];
            const int sn = s + 1 < KS ? s + 1 : s;
#pragma unroll
            for (int t = 0; t < NTW; ++t)
#pragma unroll
                for (int p = 0; p < 3; ++p) wn_[p][t] = *(const bf16x8*)(w3 + ((((size_t)(wn + 4 * t) * KS + sn) * 3 + p) * 64 + lane) * 8);
#pragma unroll
            for (int j = 0; j < 6; ++j)
#pragma unroll
                for (int t = 0; t < NTW; ++t)
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
                        acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[x3::PA[j]][t], xb[x3::PB[j]][mt], acc[t][mt], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < NTW; ++t)
#pragma unroll
                for (int p = 0; p < 3; ++p) wa[p][t] = wn_[p][t];
        }
    };
    // ---- 1. att rows -> split planes
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = grp + i * 16;
        const long long m = m0 + r;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const f32x4 lo = m < a.M ? *(const f32x4*)(a.att + m * K + 8 * l16) : z, hi = m < a.M ? *(const f32x4*)(a.att + m * K + 8 * l16 + 4) : z;
        x3_split_store<PLANE>(xh, r, l16, lo, hi);
    }
    __syncthreads();
    // ---- 2. x2 = proj(att) + x   (kept in registers; a copy goes to LDS for the LayerNorm)
    f32x4 x2[NTW][4];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) x2[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    gemm(a.w_proj, x2);
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
        const int n = (wn + 4 * t) * 16 + 4 * q;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int r = wm * 64 + mt * 16 + c;
            const long long m = m0 + r;
            if (m < a.M) x2[t][mt] += *(const f32x4*)(a.x + m * K + n);
            *(f32x4*)x3_f32(s2, r, n) = x2[t][mt];
        }
    }
    __syncthreads();              // every wave is done reading the att planes; x2 rows are complete in s2
    // ---- 3. LN(x2) -> split planes
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = grp + i * 16;
        f32x4 v[2] = {*(const f32x4*)x3_f32(s2, r, 8 * l16), *(const f32x4*)x3_f32(s2, r, 8 * l16 + 4)};
        float sum = ((v[0][0] + v[0][1]) + (v[0][2] + v[0][3])) + ((v[1][0] + v[1][1]) + (v[1][2] + v[1][3]));
        sum = row16_sum(sum);
        const float mean = sum / (float)K;
        float var = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[u][e] - mean; var = fmaf(d, d, var); }
        var = row16_sum(var);
        const float rstd = 1.0f / sqrtf(var / (float)K + 1e-5f);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const f32x4 g = *(const f32x4*)(a.g2 + 8 * l16 + 4 * u), bt = *(const f32x4*)(a.b2 + 8 * l16 + 4 * u);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[u][e] = (v[u][e] - mean) * rstd * g[e] + bt[e];
        }
        x3_split_store<PLANE>(xh, r, l16, v[0], v[1]);
    }
    __syncthreads();
    // ---- 4. hid = relu(fc1(LN(x2)) + b1) -> split planes (through s2: a lane holds 4 outputs of a token, a chunk is 8)
    {
        f32x4 acc[NTW][4];
#pragma unroll
        for (int t = 0; t < NTW; ++t)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        gemm(a.w_fc1, acc);
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
            const int n = (wn + 4 * t) * 16 + 4 * q;
            const f32x4 b4 = *(const f32x4*)(a.bias1 + n);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                f32x4 v = acc[t][mt] + b4;
                v = relu4(v);
                *(f32x4*)x3_f32(s2, wm * 64 + mt * 16 + c, n) = v;          // (s2's LayerNorm input has been consumed: barrier above)
            }
        }
    }
    __syncthreads();              // GEMM 2 has read its planes; hid rows are complete in s2
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = grp + i * 16;
        x3_split_store<PLANE>(xh, r, l16, *(const f32x4*)x3_f32(s2, r, 8 * l16), *(const f32x4*)x3_f32(s2, r, 8 * l16 + 4));
    }
    __syncthreads();
    // ---- 5. x = fc2(hid) + b2 + x2
    {
        f32x4 acc[NTW][4];
#pragma unroll
        for (int t = 0; t < NTW; ++t)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        gemm(a.w_fc2, acc);
#pragma unroll
        for (int t = 0; t < NTW; ++t) {
            const int n = (wn + 4 * t) * 16 + 4 * q;
            const f32x4 b4 = *(const f32x4*)(a.bias2 + n);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const long long m = m0 + wm * 64 + mt * 16 + c;
                if (m < a.M) *(f32x4*)(a.x + m * K + n) = (acc[t][mt] + b4) + x2[t][mt];
            }
        }
    }
}

// The same block in the form of stage_x3_kernel's MLP half (round 4, after that kernel turned out twice as fast per tile): 8 waves on
// a 64-token tile, wave w owns output features 16 w .. 16 w + 15 of all 64 rows in each of the three GEMMs (no weight fragment is
// fetched twice by a workgroup), its 12 KB weight tile of the NEXT GEMM is requested before the current one starts and stays in
// flight across the LDS phases (LDS-only barriers, loads pinned with scheduling barriers), LayerNorm row sums on DPP.  80 KB of LDS:
// two workgroups per CU, whose phases interleave.  Arithmetic identical to mlp_block_x3_kernel (same split, same order per output).
__global__ __launch_bounds__(512) void mlp_block8_x3_kernel(MlpArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t xh[];      // [3][64][128] split planes | float s2[64][128] (swizzled)
    constexpr int BM = 64, K = 128, PLANE = BM * K, KS = K / 32;
    static_assert(K == X3_K, "the uplift_x3.h blocks are written for 128-wide rows");
    float* s2 = (float*)(xh + 3 * PLANE);
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)ttup_bid_x() * BM;
    const int q = lane >> 4, c = lane & 15;
    const int grp = tid >> 4, l16 = tid & 15;
    const int n = wave * 16 + 4 * q;
    auto load_tile = [&](const uint16_t* __restrict__ w3, bf16x8 (&w)[3][KS]) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int p = 0; p < 3; ++p) w[p][s] = *(const bf16x8*)(w3 + ((((size_t)wave * KS + s) * 3 + p) * 64 + lane) * 8);
        __builtin_amdgcn_sched_barrier(0);
    };
    // ---- small operands first (the memory counter retires in order), then the first weight tile, then the att rows
    f32x4 xr[4], lg[2], lb[2];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const long long m = m0 + mt * 16 + c;
        xr[mt] = m < a.M ? *(const f32x4*)(a.x + m * K + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) { lg[u] = *(const f32x4*)(a.g2 + 8 * l16 + 4 * u); lb[u] = *(const f32x4*)(a.b2 + 8 * l16 + 4 * u); }
    const f32x4 bias1 = *(const f32x4*)(a.bias1 + n), bias2 = *(const f32x4*)(a.bias2 + n);
    f32x4 at[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long m = m0 + grp + 32 * i;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        at[i][0] = m < a.M ? *(const f32x4*)(a.att + m * K + 8 * l16) : z;
        at[i][1] = m < a.M ? *(const f32x4*)(a.att + m * K + 8 * l16 + 4) : z;
    }
    bf16x8 wnext[3][KS];
    load_tile(a.w_proj, wnext);
#pragma unroll
    for (int i = 0; i < 2; ++i) x3_split_store<PLANE>(xh, grp + 32 * i, l16, at[i][0], at[i][1]);
    stage_barrier();
    // ---- x2 = proj(att) + x
    f32x4 x2[4];
    {
        bf16x8 wc[3][KS];
        x3_take(wc, wnext);
        load_tile(a.w_fc1, wnext);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) x2[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        x3_gemm64<PLANE>(xh, c, q, wc, x2);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            x2[mt] += xr[mt];
            *(f32x4*)x3_f32(s2, mt * 16 + c, n) = x2[mt];
        }
    }
    stage_barrier();
    // ---- LN(x2) -> split planes
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = grp + 32 * i;
        f32x4 v[2] = {*(const f32x4*)x3_f32(s2, r, 8 * l16), *(const f32x4*)x3_f32(s2, r, 8 * l16 + 4)};
        float sum = ((v[0][0] + v[0][1]) + (v[0][2] + v[0][3])) + ((v[1][0] + v[1][1]) + (v[1][2] + v[1][3]));
        sum = row16_sum(sum);
        const float mean = sum / (float)K;
        float var = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[u][e] - mean; var = fmaf(d, d, var); }
        var = row16_sum(var);
        const float rstd = 1.0f / sqrtf(var / (float)K + 1e-5f);
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[u][e] = (v[u][e] - mean) * rstd * lg[u][e] + lb[u][e];
        x3_split_store<PLANE>(xh, r, l16, v[0], v[1]);
    }
    stage_barrier();
    // ---- hid = relu(fc1(LN(x2)) + b1) -> s2 -> split planes
    {
        bf16x8 wc[3][KS];
        x3_take(wc, wnext);
        load_tile(a.w_fc2, wnext);
        f32x4 acc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        x3_gemm64<PLANE>(xh, c, q, wc, acc);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            f32x4 v = acc[mt] + bias1;
            v = relu4(v);
            *(f32x4*)x3_f32(s2, mt * 16 + c, n) = v;
        }
    }
    stage_barrier();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = grp + 32 * i;
        x3_split_store<PLANE>(xh, r, l16, *(const f32x4*)x3_f32(s2, r, 8 * l16), *(const f32x4*)x3_f32(s2, r, 8 * l16 + 4));
    }
    stage_barrier();
    // ---- x = fc2(hid) + b2 + x2
    {
        f32x4 acc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        x3_gemm64<PLANE>(xh, c, q, wnext, acc);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const long long m = m0 + mt * 16 + c;
            if (m < a.M) *(f32x4*)(a.x + m * K + n) = (acc[mt] + bias2) + x2[mt];
        }
    }
}

// qkv = LN(x) Wqkv^T + b for D = 128 (384 outputs), the stage kernel's steps 1-2 with the result written to memory: 8 waves on a
// 64-token tile, wave w computes the q, k and v tiles w, 8 + w, 16 + w (all 64 rows each), weight tiles requested one GEMM ahead.
// Used instead of linear_x3_kernel<true, 3, *> for launches of at most 256 tiles (the hub surface, the pipeline's per-clip uplift),
// where one workgroup's latency is what counts.
struct QkvArgs { const float* x; float* qkv; long long M; const uint16_t* w_qkv; const float* b_qkv; const float* g1; const float* b1; };
__global__ __launch_bounds__(512) void qkv_block8_x3_kernel(QkvArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t xh[];      // [3][64][128] split planes
    constexpr int BM = 64, K = 128, PLANE = BM * K, KS = K / 32;
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const long long m0 = (long long)ttup_bid_x() * BM;
    const int q = lane >> 4, c = lane & 15;
    const int grp = tid >> 4, l16 = tid & 15;
    auto load_tile = [&](int nt, bf16x8 (&w)[3][KS]) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int p = 0; p < 3; ++p) w[p][s] = *(const bf16x8*)(a.w_qkv + ((((size_t)nt * KS + s) * 3 + p) * 64 + lane) * 8);
        __builtin_amdgcn_sched_barrier(0);
    };
    // ---- LN(x) rows -> split planes (16 lanes per row, rows grp and grp + 32)
    f32x4 xv[2][2], lg[2], lb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long long m = m0 + grp + 32 * i;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        xv[i][0] = m < a.M ? *(const f32x4*)(a.x + m * K + 8 * l16) : z;
        xv[i][1] = m < a.M ? *(const f32x4*)(a.x + m * K + 8 * l16 + 4) : z;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) { lg[u] = *(const f32x4*)(a.g1 + 8 * l16 + 4 * u); lb[u] = *(const f32x4*)(a.b1 + 8 * l16 + 4 * u); }
    bf16x8 wnext[3][KS];
    load_tile(wave, wnext);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = grp + 32 * i;
        f32x4 (&v)[2] = xv[i];
        float sum = ((v[0][0] + v[0][1]) + (v[0][2] + v[0][3])) + ((v[1][0] + v[1][1]) + (v[1][2] + v[1][3]));
        sum = row16_sum(sum);
        const float mean = sum / (float)K;
        float var = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[u][e] - mean; var = fmaf(d, d, var); }
        var = row16_sum(var);
        const float rstd = 1.0f / sqrtf(var / (float)K + 1e-5f);
        u32x4 p0, p1, p2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float x0 = (v[j >> 1][2 * (j & 1)] - mean) * rstd * lg[j >> 1][2 * (j & 1)] + lb[j >> 1][2 * (j & 1)];
            const float x1 = (v[j >> 1][2 * (j & 1) + 1] - mean) * rstd * lg[j >> 1][2 * (j & 1) + 1] + lb[j >> 1][2 * (j & 1) + 1];
            const unsigned q0 = ux3_pack2(x0, x1);
            const float r0 = x0 - __uint_as_float(q0 << 16), r1 = x1 - __uint_as_float(q0 & 0xffff0000u);
            const unsigned q1 = ux3_pack2(r0, r1);
            const float s0 = r0 - __uint_as_float(q1 << 16), s1 = r1 - __uint_as_float(q1 & 0xffff0000u);
            p0[j] = q0; p1[j] = q1; p2[j] = ux3_pack2(s0, s1);
        }
        uint16_t* d = xh + r * K + ((l16 ^ (r & 15)) << 3);
        *(u32x4*)d = p0; *(u32x4*)(d + PLANE) = p1; *(u32x4*)(d + 2 * PLANE) = p2;
    }
    stage_barrier();
    // ---- the wave's q, k, v tiles
    const uint16_t* xw = xh + c * K;
#pragma unroll
    for (int jp = 0; jp < 3; ++jp) {
        bf16x8 wc[3][KS];
        x3_take(wc, wnext);
        const int nn = jp * K + wave * 16 + 4 * q;
        const f32x4 b4 = *(const f32x4*)(a.b_qkv + nn);
        if (jp < 2) load_tile((jp + 1) * 8 + wave, wnext);
        f32x4 acc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            bf16x8 xb[3][4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int p = 0; p < 3; ++p) xb[p][mt] = *(const bf16x8*)(xw + p * PLANE + mt * 16 * K + (((4 * s + q) ^ c) << 3));
#pragma unroll
            for (int j = 0; j < 6; ++j)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wc[x3::PA[j]][s], xb[x3::PB[j]][mt], acc[mt], 0, 0, 0);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const long long m = m0 + mt * 16 + c;
            if (m < a.M) *(f32x4*)(a.qkv + m * (3 * K) + nn) = acc[mt] + b4;
        }
    }
}

// ------------------------------------------------------------------ fused attention half of a layer, short sequences
// att = softmax-attention(RoPE(q), RoPE(k), v) with qkv = LN(x) Wqkv^T + b, for sequences of S <= 16 tokens (the table stage: 14),
// D = 128, 4 heads of 32: ONE kernel instead of the qkv linear + the attention launch, and the 1536 bytes of qkv per token never
// leave the CU (at B = 10 000 trajectories the table stage is 17 M tokens per layer).  A workgroup of 8 waves owns SEQS = 64 / S
// whole sequences (rows beyond SEQS*S idle):
//   1. LN(x) rows -> three split-bf16 planes in LDS; every wave loads the twelve fragments of ITS 16 rows into registers (the plane
//      storage is free after that and is reused for qkv);
//   2. qkv of all four heads by the split-bf16 GEMM of linear_x3_kernel: wave (m-tile w & 3, head pair w >> 2) streams the weight
//      fragments of its 12 n-tiles from L2; bias and RoPE (q, k; not the cls rows) in the epilogue -> LDS [64][4 x (q|k|v)];
//   3. attention on the fp32 matrix pipe, one (sequence, head) per wave at a time: scores^T = K Q^T (8 v_mfma_f32_16x16x4_f32: a lane
//      ends with the scores of ONE query against four keys, so the softmax is in-lane plus two cross-lane steps), P V with the key
//      index permuted so that the probabilities are already where the A operand wants them (8 more MFMAs) -> att.
// (First version: scalar attention, four threads per query row -- VALU-bound on redundant exp() calls, no faster than the two
// separate launches.)
struct AttnBlockArgs {
    const float* x; float* att; long long n_seq;
    const uint16_t* w_qkv; const float* b_qkv; const float* g1; const float* b1;
    SeqView sv;
};
constexpr int ATTN_QS = 196;          // floats per row of the qkv tile: 2 heads x 96 + 4 (784 B = 49 slots of 16 B: consecutive rows fall on consecutive slots)
__global__ __launch_bounds__(512) void attn_block_x3_kernel(AttnBlockArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t xh[];      // [3][64][128] split planes of LN(x); then float qh[64][ATTN_QS], two heads at a time
    // (50 KB: two workgroups per CU; with all four heads in LDS -- 99 KB, one workgroup per CU -- the kernel was latency-bound)
    constexpr int BM = 64, K = 128, PLANE = BM * K, KS = K / 32, HD = 32, QS = ATTN_QS;
    float* qh = (float*)xh;
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const int S = a.sv.S, SEQS = BM / S, ROWS = SEQS * S;
    const long long seq0 = (long long)ttup_bid_x() * SEQS;
    const long long m0 = seq0 * S, M = a.n_seq * S;
    const int q = lane >> 4, c = lane & 15;
    // ---- 1. LN(x) rows -> split planes (16 lanes per row, 32 rows per pass)
    {
        const int grp = tid >> 4, l16 = tid & 15;
        const f32x4 gg[2] = {*(const f32x4*)(a.g1 + 8 * l16), *(const f32x4*)(a.g1 + 8 * l16 + 4)};
        const f32x4 bb[2] = {*(const f32x4*)(a.b1 + 8 * l16), *(const f32x4*)(a.b1 + 8 * l16 + 4)};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = grp + i * 32;
            const long long m = m0 + r;
            const bool ok = r < ROWS && m < M;
            f32x4 v[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) v[u] = ok ? *(const f32x4*)(a.x + m * K + 8 * l16 + 4 * u) : f32x4{0.f, 0.f, 0.f, 0.f};
            float sum = ((v[0][0] + v[0][1]) + (v[0][2] + v[0][3])) + ((v[1][0] + v[1][1]) + (v[1][2] + v[1][3]));
            sum = row16_sum(sum);
            const float mean = sum / (float)K;
            float var = 0.f;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float d = v[u][e] - mean; var = fmaf(d, d, var); }
            var = row16_sum(var);
            const float rstd = 1.0f / sqrtf(var / (float)K + 1e-5f);
            u32x4 p0, p1, p2;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x0 = (v[j >> 1][2 * (j & 1)] - mean) * rstd * gg[j >> 1][2 * (j & 1)] + bb[j >> 1][2 * (j & 1)];
                const float x1 = (v[j >> 1][2 * (j & 1) + 1] - mean) * rstd * gg[j >> 1][2 * (j & 1) + 1] + bb[j >> 1][2 * (j & 1) + 1];
                const unsigned q0 = ux3_pack2(x0, x1);
                const float r0 = x0 - __uint_as_float(q0 << 16), r1 = x1 - __uint_as_float(q0 & 0xffff0000u);
                const unsigned q1 = ux3_pack2(r0, r1);
                const float s0 = r0 - __uint_as_float(q1 << 16), s1 = r1 - __uint_as_float(q1 & 0xffff0000u);
                p0[j] = q0; p1[j] = q1; p2[j] = ux3_pack2(s0, s1);
            }
            uint16_t* d = xh + r * K + ((l16 ^ (r & 15)) << 3);
            *(u32x4*)d = p0; *(u32x4*)(d + PLANE) = p1; *(u32x4*)(d + 2 * PLANE) = p2;
        }
    }
    __syncthreads();
    // ---- 2. qkv of all heads
    const int mt = wave & 3, hp = wave >> 2;
    bf16x8 xb[3][KS];
    {
        const uint16_t* xw = xh + (mt * 16 + c) * K;
#pragma unroll
        for (int sK = 0; sK < KS; ++sK)
#pragma unroll
            for (int p = 0; p < 3; ++p) xb[p][sK] = *(const bf16x8*)(xw + p * PLANE + (((4 * sK + q) ^ c) << 3));
    }
    __syncthreads();              // every wave holds its fragments: the plane storage becomes the qkv tile
    const int grow = mt * 16 + c;                            // the lane's token row in the tile
    const int gsl = grow / S, gjt = grow - gsl * S;
    const long long gseq = seq0 + gsl;
    const bool rot = grow < ROWS && gseq < a.n_seq && gjt >= a.sv.num_cls;
    const float2* rrow = a.sv.rope + ((size_t)((rot ? gseq : 0) / a.sv.times_div) * a.sv.times_stride + (rot ? gjt - a.sv.num_cls : 0)) * (HD / 2);
    for (int rd = 0; rd < 2; ++rd) {                         // two heads per round: wave (m-tile w & 3, head 2 rd + (w >> 2))
        {
            const int h = 2 * rd + hp;
#pragma unroll
            for (int jp = 0; jp < 3; ++jp) {                 // n-tile pairs: q, k, v of the head
                const int nt0 = jp * 8 + 2 * h;
                bf16x8 wa[2][3][KS];
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int sK = 0; sK < KS; ++sK)
#pragma unroll
                        for (int p = 0; p < 3; ++p) wa[e][p][sK] = *(const bf16x8*)(a.w_qkv + ((((size_t)(nt0 + e) * KS + sK) * 3 + p) * 64 + lane) * 8);
                f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int sK = 0; sK < KS; ++sK)
#pragma unroll
                    for (int jj = 0; jj < 6; ++jj)
#pragma unroll
                        for (int e = 0; e < 2; ++e) acc[e] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[e][x3::PA[jj]][sK], xb[x3::PB[jj]][sK], acc[e], 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    f32x4 v = acc[e] + *(const f32x4*)(a.b_qkv + (nt0 + e) * 16 + 4 * q);
                    if (jp < 2 && rot) {                     // RoPE on q and k: dim pairs (e*16 + 4q, +1) and (+2, +3) of the head
                        const f32x4 cs = *(const f32x4*)(rrow + e * 8 + 2 * q);          // (cos, sin) of the two pairs
                        v = f32x4{v[0] * cs[0] - v[1] * cs[1], v[0] * cs[1] + v[1] * cs[0], v[2] * cs[2] - v[3] * cs[3], v[2] * cs[3] + v[3] * cs[2]};
                    }
                    *(f32x4*)(qh + grow * QS + hp * 96 + jp * 32 + e * 16 + 4 * q) = v;
                }
            }
        }
        __syncthreads();
        // ---- 3. attention: task = (sequence sl, head of the round); lane (c, q)
        for (int task = wave; task < SEQS * 2; task += 8) {
        const int sl = task >> 1, h = 2 * rd + (task & 1);
        const long long seq = seq0 + sl;
        if (seq >= a.n_seq) continue;                        // wave-uniform
        const float* base = qh + (sl * S) * QS + (task & 1) * 96;
        const float* mrow = a.sv.mask + (size_t)(seq / a.sv.mask_div) * S;
        // scores^T = K Q^T: A = K (row j = c, dims 8q .. 8q+7), B = Q (column i = c, the same dims); rows past the tile's last
        // sequence belong to nobody and are masked below
        const int jr = sl * S + c < BM ? c : 0;
        const f32x4 k0 = *(const f32x4*)(base + jr * QS + 32 + 8 * q), k1 = *(const f32x4*)(base + jr * QS + 32 + 8 * q + 4);
        const f32x4 q0 = *(const f32x4*)(base + jr * QS + 8 * q), q1 = *(const f32x4*)(base + jr * QS + 8 * q + 4);
        f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(k0[e], q0[e], sc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(k1[e], q1[e], sc, 0, 0, 0);
        // sc[r] = q_i . k_j for query i = c, key j = 4q + r
        const bool row_ok = c < S && mrow[c < S ? c : 0] == 0.f;
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 4 * q + r;
            const bool col_ok = j < S && mrow[j < S ? j : 0] == 0.f;
            sc[r] = col_ok ? sc[r] * a.sv.scale : -INFINITY;
            mx = sc[r] > mx ? sc[r] : mx;
        }
        { const float o = __shfl_xor(mx, 16, 64); mx = o > mx ? o : mx; }
        { const float o = __shfl_xor(mx, 32, 64); mx = o > mx ? o : mx; }
        float pr[4], den = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { pr[r] = (row_ok && sc[r] > -INFINITY) ? __expf(sc[r] - mx) : 0.f; den += pr[r]; }
        den += __shfl_xor(den, 16, 64);
        den += __shfl_xor(den, 32, 64);
        const float inv = den > 0.f ? 1.f / den : 0.f;       // a fully masked query row yields zeros (torch SDPA semantics)
        // the sums are normalised AFTER P V, as in stage_x3_kernel and the attention_mfma kernels (it used to be p * inv before: the
        // one place where this path and the stage kernel rounded differently).  Query 4q + r is lane 4q + r's (its c).
        float invr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) invr[r] = __shfl(inv, 4 * q + r, 64);
        // out = P V, k index (step s, lane group q) <-> key j = 4q + s: the A operand of step s is the lane's own pr[s]
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s2_ = 0; s2_ < 4; ++s2_) {
                const int j = 4 * q + s2_;
                const float vv = (j < S) ? base[j * QS + 64 + dt * 16 + c] : 0.f;
                o = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[s2_], vv, o, 0, 0, 0);
            }
            // o[r] = out[query 4q + r][dim dt*16 + c]
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 4 * q + r;
                if (i < S) a.att[(m0 + sl * S + i) * K + h * HD + dt * 16 + c] = o[r] * invr[r];
            }
        }
        }
        __syncthreads();              // the round's q | k | v are consumed: the next round overwrites them
    }
}

}  // namespace
