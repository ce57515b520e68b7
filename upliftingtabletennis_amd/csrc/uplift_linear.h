// The uplift forward's linear layers: the exact-fp32 MFMA kernel, its split-bf16 form for K = 128, and the tiny-K kernel.
//   linear_kernel   out = [relu](LN?(x) W^T + b) [+ res] on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate).  W is the
//                   A operand (pre-packed per lane on the host), the token tile is the B operand read from LDS, so a lane owns 4
//                   consecutive outputs of one token.
// Private to csrc/uplift.hip, which includes it after uplift_x3.h inside its no-packed-fp32 region; no other unit may include it.
#pragma once

namespace {

struct LinArgs {
    const float* x; int ldx;
    const float* w; const float* bias;
    const float* gamma; const float* beta;      // LayerNorm (null = none)
    const float* res; int ldr;
    float* out; int ldo;
    int M, N, K, relu;
};

// K permutation shared by the packed weights and the LDS image: MFMA k-step s, k-lane q  <->  k = q*(K/4) + s
// Workgroup tile: 64*MH token rows x 64*NTW outputs, 4*MH waves; wave (wm, wn) owns rows wm*64.. and N-tiles wn + 4t.
template <bool LN, int NTW, int MH>
__global__ __launch_bounds__(256 * MH) void linear_kernel(LinArgs a) {
    extern __shared__ __attribute__((aligned(16))) float xs[];      // [4][64*MH][K/4 + 4]
    constexpr int BM = 64 * MH;
    const int K = a.K, KQ = K / 4, RS = KQ + 4, PLANE = BM * RS;
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6, wn = wave & 3, wm = wave >> 2;
    const int m0 = ttup_bid_x() * BM, n0 = ttup_bid_y() * (64 * NTW);
    // ---- stage the token rows (LayerNorm applied on the way in): 16 lanes per row, float4 per lane per 64 features
    {
        const int grp = tid >> 4, l16 = tid & 15;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = grp + i * 16 * MH, m = m0 + r;
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = 4 * (l16 + 16 * u);
                v[u] = (m < a.M && k < K) ? *(const f32x4*)(a.x + (size_t)m * a.ldx + k) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
            if (LN) {
                float sum = 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) sum += (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);
                sum = row16_sum(sum);
                const float mean = sum / (float)K;
                float var = 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (4 * (l16 + 16 * u) >= K) continue;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const float d = v[u][e] - mean; var = fmaf(d, d, var); }
                }
                var = row16_sum(var);
                const float rstd = 1.0f / sqrtf(var / (float)K + 1e-5f);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = 4 * (l16 + 16 * u);
                    if (k >= K) continue;
                    const f32x4 g = *(const f32x4*)(a.gamma + k), bt = *(const f32x4*)(a.beta + k);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[u][e] = (v[u][e] - mean) * rstd * g[e] + bt[e];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = 4 * (l16 + 16 * u);
                if (k < K) *(f32x4*)(xs + (k / KQ) * PLANE + r * RS + (k % KQ)) = v[u];
            }
        }
    }
    __syncthreads();
    const int q = lane >> 4, c = lane & 15;
    f32x4 acc[NTW][4];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntiles = (a.N + 15) / 16;
    int nt_g[NTW]; bool nt_ok[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) { nt_g[t] = n0 / 16 + wn + 4 * t; nt_ok[t] = nt_g[t] < ntiles; }
    const int ks4 = K / 16;
    const float* xw = xs + q * PLANE + (wm * 64 + c) * RS;
    f32x4 wa[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
        wa[t] = nt_ok[t] ? *(const f32x4*)(a.w + (((size_t)nt_g[t] * ks4) * 64 + lane) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s4 = 0; s4 < ks4; ++s4) {
        f32x4 xb[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) xb[mt] = *(const f32x4*)(xw + mt * 16 * RS + s4 * 4);
        f32x4 wn_[NTW];
        const int sn = s4 + 1 < ks4 ? s4 + 1 : s4;
#pragma unroll
        for (int t = 0; t < NTW; ++t)
            wn_[t] = nt_ok[t] ? *(const f32x4*)(a.w + (((size_t)nt_g[t] * ks4 + sn) * 64 + lane) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < NTW; ++t)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[t][j], xb[mt][j], acc[t][mt], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < NTW; ++t) wa[t] = wn_[t];
    }
    // ---- epilogue: lane holds outputs n = nt*16 + 4*q + {0..3} of token m = m0 + wm*64 + mt*16 + c
    const bool vec = (a.N % 4 == 0) && (a.ldo % 4 == 0) && (!a.res || a.ldr % 4 == 0);
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
        if (!nt_ok[t]) continue;
        const int n = nt_g[t] * 16 + 4 * q;
        if (vec) {
            if (n >= a.N) continue;
            const f32x4 b4 = a.bias ? *(const f32x4*)(a.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int m = m0 + wm * 64 + mt * 16 + c;
                if (m >= a.M) continue;
                f32x4 v = acc[t][mt] + b4;
                if (a.relu) v = relu4(v);
                if (a.res) v += *(const f32x4*)(a.res + (size_t)m * a.ldr + n);
                *(f32x4*)(a.out + (size_t)m * a.ldo + n) = v;
            }
            continue;
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int m = m0 + wm * 64 + mt * 16 + c;
            if (m >= a.M) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (n + r >= a.N) continue;
                float v = acc[t][mt][r] + (a.bias ? a.bias[n + r] : 0.f);
                if (a.relu) v = v > 0.f ? v : 0.f;
                if (a.res) v += a.res[(size_t)m * a.ldr + n + r];
                a.out[(size_t)m * a.ldo + n + r] = v;
            }
        }
    }
}

// The same layer on the bf16 matrix pipe with SPLIT operands (the arithmetic of csrc/conv_x3.hip; the shared pieces are in uplift_x3.h): every fp32 weight and every
// (LayerNorm'd) activation is split exactly into three bf16 parts, a product is the sum of six exact partial products (smallest
// first) accumulated in fp32 -- accurate to below one fp32 fma rounding, at 2.7x the peak rate of v_mfma_f32_16x16x4_f32.  K = 128
// only (the transformer layers of the 'large' model: 98 % of the work); TTUP_F32_EXACT=1 keeps the fp32-MFMA kernel.
// LDS image: three planes [64*MH tokens][128] bf16 (256-byte rows), the 16-byte chunk index XOR-swizzled with the token's low four
// bits: the 16 lanes of a ds_read_b128 group (8 tokens of one k chunk, 8 of the next) fall on 16 different chunks.

template <bool LN, int NTW, int MH>
__global__ __launch_bounds__(256 * MH) void linear_x3_kernel(LinArgs a, const uint16_t* __restrict__ w3) {
    extern __shared__ __attribute__((aligned(16))) uint16_t xh[];      // [3][64*MH][128]
    constexpr int BM = 64 * MH, K = 128, PLANE = BM * K;
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6, wn = wave & 3, wm = wave >> 2;
    const int m0 = ttup_bid_x() * BM, n0 = ttup_bid_y() * (64 * NTW);
    // ---- stage the token rows (LayerNorm applied on the way in): 16 lanes per row, two float4 per lane (8 consecutive features)
    {
        const int grp = tid >> 4, l16 = tid & 15;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = grp + i * 16 * MH, m = m0 + r;
            f32x4 v[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) v[u] = m < a.M ? *(const f32x4*)(a.x + (size_t)m * a.ldx + 8 * l16 + 4 * u) : f32x4{0.f, 0.f, 0.f, 0.f};
            if (LN) {
                // (mean / variance with the summation tree of linear_kernel's staging is not required: any order is within the bar;
                // a 16-lane tree over 8 features per lane)
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
                    const f32x4 g = *(const f32x4*)(a.gamma + 8 * l16 + 4 * u), bt = *(const f32x4*)(a.beta + 8 * l16 + 4 * u);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[u][e] = (v[u][e] - mean) * rstd * g[e] + bt[e];
                }
            }
            u32x4 p0, p1, p2;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x0 = v[j >> 1][2 * (j & 1)], x1 = v[j >> 1][2 * (j & 1) + 1];
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
    const int q = lane >> 4, c = lane & 15;
    f32x4 acc[NTW][4];
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntiles = (a.N + 15) / 16;
    int nt_g[NTW]; bool nt_ok[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) { nt_g[t] = n0 / 16 + wn + 4 * t; nt_ok[t] = nt_g[t] < ntiles; }
    constexpr int KS = K / 32;
    // token c of m-tile mt sits in row wm*64 + mt*16 + c: (row & 15) == c, so the swizzle term is the lane's own c
    const uint16_t* xw = xh + (wm * 64 + c) * K;
    bf16x8 wa[3][NTW];
    const bf16x8 zero8 = {};
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
        for (int p = 0; p < 3; ++p) wa[p][t] = nt_ok[t] ? *(const bf16x8*)(w3 + ((((size_t)nt_g[t] * KS) * 3 + p) * 64 + lane) * 8) : zero8;
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
            for (int p = 0; p < 3; ++p) wn_[p][t] = nt_ok[t] ? *(const bf16x8*)(w3 + ((((size_t)nt_g[t] * KS + sn) * 3 + p) * 64 + lane) * 8) : zero8;
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
    // ---- epilogue: lane holds outputs n = nt*16 + 4*q + {0..3} of token m = m0 + wm*64 + mt*16 + c  (N % 4 == 0 for K = 128 layers)
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
        if (!nt_ok[t]) continue;
        const int n = nt_g[t] * 16 + 4 * q;
        if (n >= a.N) continue;
        const f32x4 b4 = a.bias ? *(const f32x4*)(a.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int m = m0 + wm * 64 + mt * 16 + c;
            if (m >= a.M) continue;
            f32x4 v = acc[t][mt] + b4;
            if (a.relu) v = relu4(v);
            if (a.res) v += *(const f32x4*)(a.res + (size_t)m * a.ldr + n);
            *(f32x4*)(a.out + (size_t)m * a.ldo + n) = v;
        }
    }
}

// out[m][n] = relu?(sum_k x[m][k] w[n][k] + b[n]) for tiny K (2 or 3): embedding fc1
__global__ void small_linear_kernel(const float* x, int ldx, const float* w, const float* b, float* out, int ldo, long long M, int N, int K, int relu) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= M * N) return;
    const long long m = i / N; const int n = (int)(i % N);
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(x[m * ldx + k], w[n * K + k], acc);
    acc += b ? b[n] : 0.f;
    if (relu) acc = acc > 0.f ? acc : 0.f;
    out[m * ldo + n] = acc;
}

}  // namespace
