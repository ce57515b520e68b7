// The uplift forward's attention kernels: the scalar one (any head size, any length that fits LDS) and the two fp32 matrix-pipe forms.
//   attention_kernel  per (sequence, head): RoPE(q,k) on load from a per-forward (cos,sin) table, additive {0,-inf} row+column mask,
//                   online softmax in registers; a fully masked query row yields zeros (torch SDPA semantics).  Short sequences (the
//                   14-token table stage) share a wave four at a time.
// Private to csrc/uplift.hip, which includes it after uplift_x3.h inside its no-packed-fp32 region; no other unit may include it.
#pragma once

namespace {

struct AttnArgs {
    const float* qkv;   // [n_seq*S][3D]
    float* out;         // [n_seq*S][D]
    int n_seq, D, heads, hd;
    SeqView sv;
};

// P threads per (sequence, head); a workgroup of ttup_bdim_x() threads serves ttup_bdim_x() / P sequences.  K (rotated) and V
// of each sequence live in LDS, thread i0 owns query rows i0, i0+P, ...
template <int HD, int P>
__global__ __launch_bounds__(128) void attention_kernel(AttnArgs a) {      // at most 128 threads are ever launched: 256 VGPRs, no spills
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int S = a.sv.S, G = ttup_bdim_x() / P;
    const int SEQ = 2 * S * HD + 16;                 // floats per sequence; the +16 words spreads the groups over LDS banks
    float* ms = sm + G * SEQ;                        // [G][S] additive mask
    const int h = ttup_bid_y(), tid = ttup_tid_x();
    const int D3 = 3 * a.D, HV = HD / 4;
    // ---- stage K (RoPE applied) and V, one float4 per thread per step, 128 B rows read by HV consecutive threads
    for (int u = tid; u < G * S * HV; u += ttup_bdim_x()) {
        const int g = u / (S * HV), rem = u - g * (S * HV), j = rem / HV, part = rem - j * HV;
        const int seq = ttup_bid_x() * G + g;
        if (seq >= a.n_seq) continue;
        const float* kp = a.qkv + ((size_t)seq * S + j) * D3 + a.D + h * HD + part * 4;
        f32x4 k = *(const f32x4*)kp;
        const f32x4 v = *(const f32x4*)(kp + a.D);
        if (j >= a.sv.num_cls) {
            const f32x4 cs = *(const f32x4*)(a.sv.rope + ((size_t)(seq / a.sv.times_div) * a.sv.times_stride + (j - a.sv.num_cls)) * (HD / 2) + part * 2);
            k = f32x4{k[0] * cs[0] - k[1] * cs[1], k[0] * cs[1] + k[1] * cs[0], k[2] * cs[2] - k[3] * cs[3], k[2] * cs[3] + k[3] * cs[2]};
        }
        *(f32x4*)(sm + g * SEQ + j * HD + part * 4) = k;
        *(f32x4*)(sm + g * SEQ + S * HD + j * HD + part * 4) = v;
    }
    for (int u = tid; u < G * S; u += ttup_bdim_x()) {
        const int seq = ttup_bid_x() * G + u / S;
        ms[u] = seq < a.n_seq ? a.sv.mask[(size_t)(seq / a.sv.mask_div) * S + (u % S)] : -INFINITY;
    }
    __syncthreads();
    const int g = tid / P, i0 = tid - g * P;
    const int seq = ttup_bid_x() * G + g;
    if (seq >= a.n_seq) return;
    const float* ks = sm + g * SEQ;
    const float* vs = ks + S * HD;
    const float* mg = ms + g * S;
    for (int i = i0; i < S; i += P) {
        f32x4 q[HV];
        const float* qp = a.qkv + ((size_t)seq * S + i) * D3 + h * HD;
#pragma unroll
        for (int d = 0; d < HV; ++d) q[d] = *(const f32x4*)(qp + 4 * d);
        if (i >= a.sv.num_cls) {
            const float2* rp = a.sv.rope + ((size_t)(seq / a.sv.times_div) * a.sv.times_stride + (i - a.sv.num_cls)) * (HD / 2);
#pragma unroll
            for (int d = 0; d < HV; ++d) {
                const f32x4 cs = *(const f32x4*)(rp + 2 * d);
                q[d] = f32x4{q[d][0] * cs[0] - q[d][1] * cs[1], q[d][0] * cs[1] + q[d][1] * cs[0],
                             q[d][2] * cs[2] - q[d][3] * cs[3], q[d][2] * cs[3] + q[d][3] * cs[2]};
            }
        }
        f32x4 o[HV];
#pragma unroll
        for (int d = 0; d < HV; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
        float mx = -INFINITY, den = 0.f;
        if (mg[i] == 0.f) {
            for (int j = 0; j < S; ++j) {
                if (mg[j] != 0.f) continue;             // -inf column
                float s = 0.f;
#pragma unroll
                for (int d = 0; d < HV; ++d) {
                    const f32x4 kk = *(const f32x4*)(ks + j * HD + 4 * d);
                    s = fmaf(q[d][0], kk[0], s); s = fmaf(q[d][1], kk[1], s); s = fmaf(q[d][2], kk[2], s); s = fmaf(q[d][3], kk[3], s);
                }
                s *= a.sv.scale;
                if (s > mx) {
                    const float corr = expf(mx - s);
                    den *= corr;
#pragma unroll
                    for (int d = 0; d < HV; ++d) o[d] *= corr;
                    mx = s;
                }
                const float p = expf(s - mx);
                den += p;
#pragma unroll
                for (int d = 0; d < HV; ++d) {
                    const f32x4 vv = *(const f32x4*)(vs + j * HD + 4 * d);
                    o[d][0] = fmaf(p, vv[0], o[d][0]); o[d][1] = fmaf(p, vv[1], o[d][1]);
                    o[d][2] = fmaf(p, vv[2], o[d][2]); o[d][3] = fmaf(p, vv[3], o[d][3]);
                }
            }
        }
        float* op = a.out + ((size_t)seq * S + i) * a.D + h * HD;
        const float inv = den > 0.f ? 1.f / den : 0.f;
#pragma unroll
        for (int d = 0; d < HV; ++d) *(f32x4*)(op + 4 * d) = o[d] * inv;
    }
}

// ------------------------------------------------------------------ attention on the fp32 matrix pipe, long sequences
// The temporal / spin stages (sequences of T or T+1 tokens, head dim 32).  attention_kernel walks the keys with one thread per query
// row -- 121 dependent exp / fma rounds: 60-70 us for a single rally, 15 % of the time at B = 10 000.  Here a wave owns 16 queries
// of one (sequence, head): K (RoPE applied) and V of the whole sequence are staged in LDS once per workgroup (4 waves = 64 queries);
// per 16-key tile  scores^T = K Q^T  (8 v_mfma_f32_16x16x4_f32: a lane ends with the scores of ONE query against four keys, so the
// row maximum and the denominator are in-lane sums plus two cross-lane steps at the end) in a first pass for the maxima, and again in
// a second pass for p = exp(s - max) and  out += P V  (8 more MFMAs, key index permuted so that p is already the A operand).  The
// normalisation 1 / den goes through 16 floats of LDS (out rows are indexed by 4q + r, den by the lane's own query).
struct AttnMArgs {
    const float* qkv; float* out; SeqView sv; int n_seq;
};
constexpr int ATTM_KS = 36;          // floats per K / V row in LDS (144 B: 16 consecutive rows fall on 16 different 16-byte slots)
__global__ __launch_bounds__(256) void attention_mfma_kernel(AttnMArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];      // K [SP][36] | V [SP][36] | inv [4 waves][16]
    constexpr int HD = 32, D = 128, D3 = 384, KS = ATTM_KS;
    const int S = a.sv.S, KT = (S + 15) / 16, SP = KT * 16;
    float* sk = sm;
    float* sv = sm + SP * KS;
    float* sinv = sv + SP * KS;
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, c = lane & 15;
    const int h = ttup_bid_y(), seq = ttup_bid_z();
    const float* base = a.qkv + (size_t)seq * S * D3 + h * HD;
    const float2* rbase = a.sv.rope + (size_t)(seq / a.sv.times_div) * a.sv.times_stride * (HD / 2);
    const float* mrow = a.sv.mask + (size_t)(seq / a.sv.mask_div) * S;
    // ---- stage K (rotated) and V: 8 threads per row, one float4 each; rows past S are zero
    for (int u = tid; u < SP * 8; u += 256) {
        const int j = u >> 3, part = u & 7;
        f32x4 k = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f};
        if (j < S) {
            k = *(const f32x4*)(base + (size_t)j * D3 + D + part * 4);
            v = *(const f32x4*)(base + (size_t)j * D3 + 2 * D + part * 4);
            if (j >= a.sv.num_cls) {
                const f32x4 cs = *(const f32x4*)(rbase + (size_t)(j - a.sv.num_cls) * (HD / 2) + part * 2);
                k = f32x4{k[0] * cs[0] - k[1] * cs[1], k[0] * cs[1] + k[1] * cs[0], k[2] * cs[2] - k[3] * cs[3], k[2] * cs[3] + k[3] * cs[2]};
            }
        }
        *(f32x4*)(sk + j * KS + part * 4) = k;
        *(f32x4*)(sv + j * KS + part * 4) = v;
    }
    __syncthreads();
    const int qt = ttup_bid_x() * 4 + wave;                   // this wave's tile of 16 queries
    if (qt * 16 >= S) return;                                // (no barrier below: waves are independent from here on)
    const int i = qt * 16 + c;                               // the lane's query
    const bool row_ok = i < S && mrow[i < S ? i : 0] == 0.f;
    // B operand of scores^T: Q[i][8q .. 8q+7], rotated
    f32x4 q0 = {0.f, 0.f, 0.f, 0.f}, q1 = {0.f, 0.f, 0.f, 0.f};
    if (i < S) {
        q0 = *(const f32x4*)(base + (size_t)i * D3 + 8 * q);
        q1 = *(const f32x4*)(base + (size_t)i * D3 + 8 * q + 4);
        if (i >= a.sv.num_cls) {
            const float2* rp = rbase + (size_t)(i - a.sv.num_cls) * (HD / 2) + 4 * q;
            const f32x4 c0 = *(const f32x4*)rp, c1 = *(const f32x4*)(rp + 2);
            q0 = f32x4{q0[0] * c0[0] - q0[1] * c0[1], q0[0] * c0[1] + q0[1] * c0[0], q0[2] * c0[2] - q0[3] * c0[3], q0[2] * c0[3] + q0[3] * c0[2]};
            q1 = f32x4{q1[0] * c1[0] - q1[1] * c1[1], q1[0] * c1[1] + q1[1] * c1[0], q1[2] * c1[2] - q1[3] * c1[3], q1[2] * c1[3] + q1[3] * c1[2]};
        }
    }
    auto scores = [&](int kt) __attribute__((always_inline)) {
        // A operand: K[kt*16 + c][8q .. 8q+7]; result sc[r] = q_i . k_j for j = kt*16 + 4q + r, masked keys -> -inf
        const float* kp = sk + (kt * 16 + c) * KS + 8 * q;
        const f32x4 k0 = *(const f32x4*)kp, k1 = *(const f32x4*)(kp + 4);
        f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(k0[e], q0[e], sc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(k1[e], q1[e], sc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = kt * 16 + 4 * q + r;
            const bool col_ok = j < S && mrow[j < S ? j : 0] == 0.f;
            sc[r] = col_ok ? sc[r] * a.sv.scale : -INFINITY;
        }
        return sc;
    };
    float mx = -INFINITY;
    for (int kt = 0; kt < KT; ++kt) {
        const f32x4 sc = scores(kt);
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = sc[r] > mx ? sc[r] : mx;
    }
    { const float o = __shfl_xor(mx, 16, 64); mx = o > mx ? o : mx; }
    { const float o = __shfl_xor(mx, 32, 64); mx = o > mx ? o : mx; }
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
    for (int kt = 0; kt < KT; ++kt) {
        const f32x4 sc = scores(kt);
        float pr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { pr[r] = (row_ok && sc[r] > -INFINITY) ? __expf(sc[r] - mx) : 0.f; den += pr[r]; }
        // out += P V with k index (step s, lane group q) <-> key kt*16 + 4q + s: the A operand of step s is the lane's own pr[s]
        const float* vp = sv + (kt * 16 + 4 * q) * KS + c;
#pragma unroll
        for (int s2_ = 0; s2_ < 4; ++s2_) {
            o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[s2_], vp[s2_ * KS], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[s2_], vp[s2_ * KS + 16], o1, 0, 0, 0);
        }
    }
    den += __shfl_xor(den, 16, 64);
    den += __shfl_xor(den, 32, 64);
    // o[r] = out[query qt*16 + 4q + r][dim c (o0) / 16 + c (o1)]: the row's 1 / den comes from the lane that owns that query
    if (q == 0) sinv[wave * 16 + c] = den > 0.f ? 1.f / den : 0.f;          // a fully masked query row yields zeros (torch SDPA semantics)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);                    // lgkmcnt(0): the wave's own LDS writes are visible to its reads
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int io = qt * 16 + 4 * q + r;
        if (io >= S) continue;
        const float inv = sinv[wave * 16 + 4 * q + r];
        float* op = a.out + ((size_t)seq * S + io) * D + h * HD;
        op[c] = o0[r] * inv;
        op[16 + c] = o1[r] * inv;
    }
}

// The same attention for sequences of at most 128 tokens (KT <= 8 key tiles: the 121-token trajectories of the headline and of config 3)
// in the form the stage kernel's attention phase arrived at: all score tiles of a query tile are computed ONCE, as independent MFMA
// chains (groups of four key tiles), and stay in registers between the maximum and the exponentials; the mask is two ballots per wave
// instead of a global load per score; V is staged TRANSPOSED ([dim][token], row stride SP + 4) so that the P V operand of four keys is
// one 16-byte read; exponentials on v_exp_f32.  Per output the operation order is attention_mfma_kernel's.  NG = groups of four key tiles.
template <int NG>
__global__ __launch_bounds__(256) void attention_mfma8_kernel(AttnMArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];      // K [SP][36] | V^T [32][SP + 4] | inv [4 waves][16]
    constexpr int HD = 32, D = 128, D3 = 384, KS = ATTM_KS, NK = NG * 4;
    const int S = a.sv.S, KT = (S + 15) / 16, SP = KT * 16, VS = SP + 4;
    float* sk = sm;
    float* svt = sm + SP * KS;
    float* sinv = svt + HD * VS;
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, c = lane & 15;
    const int h = ttup_bid_y(), seq = ttup_bid_z();
    const float* base = a.qkv + (size_t)seq * S * D3 + h * HD;
    const float2* rbase = a.sv.rope + (size_t)(seq / a.sv.times_div) * a.sv.times_stride * (HD / 2);
    const float* mrow = a.sv.mask + (size_t)(seq / a.sv.mask_div) * S;
    // ---- stage K (rotated) and V^T: 8 threads per token, one float4 of each per thread; tokens past S are zero
    for (int u = tid; u < SP * 8; u += 256) {
        const int j = u >> 3, part = u & 7;
        f32x4 k = {0.f, 0.f, 0.f, 0.f}, v = {0.f, 0.f, 0.f, 0.f};
        if (j < S) {
            k = *(const f32x4*)(base + (size_t)j * D3 + D + part * 4);
            v = *(const f32x4*)(base + (size_t)j * D3 + 2 * D + part * 4);
            if (j >= a.sv.num_cls) {
                const f32x4 cs = *(const f32x4*)(rbase + (size_t)(j - a.sv.num_cls) * (HD / 2) + part * 2);
                k = f32x4{k[0] * cs[0] - k[1] * cs[1], k[0] * cs[1] + k[1] * cs[0], k[2] * cs[2] - k[3] * cs[3], k[2] * cs[3] + k[3] * cs[2]};
            }
        }
        *(f32x4*)(sk + j * KS + part * 4) = k;
#pragma unroll
        for (int e = 0; e < 4; ++e) svt[(part * 4 + e) * VS + j] = v[e];
    }
    // bit j of (lo, hi): token j / 64 + j is a valid key and query
    const unsigned long long lo = __builtin_amdgcn_ballot_w64(lane < S && mrow[lane < S ? lane : 0] == 0.f);
    const unsigned long long hi = __builtin_amdgcn_ballot_w64(64 + lane < S && mrow[64 + lane < S ? 64 + lane : 0] == 0.f);
    __syncthreads();
    const int qt = ttup_bid_x() * 4 + wave;                 // this wave's tile of 16 queries
    if (qt * 16 >= S) return;                                // (no barrier below: waves are independent from here on)
    const int i = qt * 16 + c;                               // the lane's query
    const bool row_ok = i < S && (((i < 64 ? lo : hi) >> (i & 63)) & 1);
    f32x4 q0 = {0.f, 0.f, 0.f, 0.f}, q1 = {0.f, 0.f, 0.f, 0.f};
    if (i < S) {
        q0 = *(const f32x4*)(base + (size_t)i * D3 + 8 * q);
        q1 = *(const f32x4*)(base + (size_t)i * D3 + 8 * q + 4);
        if (i >= a.sv.num_cls) {
            const float2* rp = rbase + (size_t)(i - a.sv.num_cls) * (HD / 2) + 4 * q;
            const f32x4 c0 = *(const f32x4*)rp, c1 = *(const f32x4*)(rp + 2);
            q0 = f32x4{q0[0] * c0[0] - q0[1] * c0[1], q0[0] * c0[1] + q0[1] * c0[0], q0[2] * c0[2] - q0[3] * c0[3], q0[2] * c0[3] + q0[3] * c0[2]};
            q1 = f32x4{q1[0] * c1[0] - q1[1] * c1[1], q1[0] * c1[1] + q1[1] * c1[0], q1[2] * c1[2] - q1[3] * c1[3], q1[2] * c1[3] + q1[3] * c1[2]};
        }
    }
    // ---- scores^T = K Q^T for every key tile (tiles past KT repeat the last one and are masked: their bits are 0)
    f32x4 sc[NK];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        f32x4 kk[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int kt = g * 4 + t < KT ? g * 4 + t : KT - 1;
            const float* kp = sk + (kt * 16 + c) * KS + 8 * q;
            kk[t][0] = *(const f32x4*)kp; kk[t][1] = *(const f32x4*)(kp + 4);
            sc[g * 4 + t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < 4; ++t) sc[g * 4 + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kk[t][0][e], q0[e], sc[g * 4 + t], 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int t = 0; t < 4; ++t) sc[g * 4 + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kk[t][1][e], q1[e], sc[g * 4 + t], 0, 0, 0);
    }
    // sc[kt][r] = q_i . k_j for j = kt*16 + 4q + r
    const unsigned long long lo_q = lo >> (4 * q), hi_q = hi >> (4 * q);
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool col_ok = kt < KT && (((kt < 4 ? lo_q : hi_q) >> ((kt & 3) * 16 + r)) & 1);
            sc[kt][r] = col_ok ? sc[kt][r] * a.sv.scale : -INFINITY;
            mx = sc[kt][r] > mx ? sc[kt][r] : mx;
        }
    { const float o = __shfl_xor(mx, 16, 64); mx = o > mx ? o : mx; }
    { const float o = __shfl_xor(mx, 32, 64); mx = o > mx ? o : mx; }
    // ---- p = exp(s - max), out += P V with k index (step s, lane group q) <-> key kt*16 + 4q + s: the A operand is the lane's own p
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
    float den = 0.f;
    const float* vbase = svt + c * VS + 4 * q;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        f32x4 vv[4][2];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int kt = g * 4 + t < KT ? g * 4 + t : KT - 1;
            vv[t][0] = *(const f32x4*)(vbase + kt * 16); vv[t][1] = *(const f32x4*)(vbase + 16 * VS + kt * 16);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float pr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) { pr[r] = (row_ok && sc[g * 4 + t][r] > -INFINITY) ? __expf(sc[g * 4 + t][r] - mx) : 0.f; den += pr[r]; }
#pragma unroll
            for (int s2_ = 0; s2_ < 4; ++s2_) {
                o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[s2_], vv[t][0][s2_], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[s2_], vv[t][1][s2_], o1, 0, 0, 0);
            }
        }
    }
    den += __shfl_xor(den, 16, 64);
    den += __shfl_xor(den, 32, 64);
    if (q == 0) sinv[wave * 16 + c] = den > 0.f ? 1.f / den : 0.f;          // a fully masked query row yields zeros (torch SDPA semantics)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);                    // lgkmcnt(0): the wave's own LDS writes are visible to its reads
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int io = qt * 16 + 4 * q + r;
        if (io >= S) continue;
        const float inv = sinv[wave * 16 + 4 * q + r];
        float* op = a.out + ((size_t)seq * S + io) * D + h * HD;
        op[c] = o0[r] * inv;
        op[16 + c] = o1[r] * inv;
    }
}

}  // namespace
