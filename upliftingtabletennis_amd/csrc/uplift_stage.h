// The uplift forward's stage kernel: ALL layers of a stage in one kernel, sequences of S <= 64 tokens.
// Private to csrc/uplift.hip, which includes it after uplift_x3.h inside its no-packed-fp32 region; no other unit may include it.
#pragma once
#include <type_traits>

namespace {

// A small batch (one rally from the hub surface, the pipeline's per-clip uplift) is a dependent chain of ~80 launches of a few
// microseconds of work each, most of them one workgroup that waits on its weight fetches.  Here a workgroup of 8 waves owns
// SEQS = 64 / S whole sequences (the table stage: four 14-token sequences; the temporal / spin stages of a clip of up to 63 frames:
// one) and runs EVERY layer of the stage on them:
//   * the tokens live in registers between layers (wave w owns output features 16 w .. 16 w + 15 of all 64 rows in every GEMM, so
//     the residuals are already where the next result lands) and pass through LDS only as LayerNorm / operand staging;
//   * per layer  LN -> q | k | v of ALL heads (three 64 x 16 tiles per wave; bias and RoPE in the epilogue) -> attention on the fp32
//     matrix pipe (attention_mfma_kernel's two-pass form over ceil(S/16) key tiles, K and V read from the qkv tile in LDS) ->
//     proj + residual -> LN -> fc1 -> ReLU -> fc2 + residual: the split-bf16 arithmetic of linear_x3_kernel throughout (same
//     split, same accumulation order per output);
//   * a wave's next 12 KB weight tile (16 outputs x 128 inputs x three bf16 planes) is requested one GEMM ahead and stays in
//     flight across the LDS phases in between: the barriers wait on LDS traffic only (stage_barrier), not on the vector-memory
//     counter, which is what made the per-layer kernels (and a first version of this one: 49 us per layer for one workgroup)
//     latency-bound on a single CU's fetches.
// LDS: split planes [3][64][128] bf16 (48 KB; the attention output aliases them) | q | k tile [64][260] fp32 (65 KB; the fp32
// staging of the LayerNorms and of the MLP aliases it) | V transposed [4 heads][32][84] fp32 (42 KB: the P V operand of four keys
// is one 16-byte read; a sequence's tokens start at a multiple of 4) | 16 floats per wave = 155.5 KB.
constexpr int STAGE_MAX_LAYERS = 16;   // the layer table travels in the kernel arguments (scalar loads, pointers known to be global)
struct StageArgs {
    float* x; long long n_seq; StageLayerW layers[STAGE_MAX_LAYERS]; int n_layers;
    SeqView sv;
    // table stage without the assembled token tensor (model.py:374-378 and the gather after the stage): when `table_tok` is set, row 0
    // of sequence (b, t) is read from x[(b*T + t)] (the ball token), row 1 + n from table_tok[b*NT + n], and only row 0 is written back
    // -- to the same place.  14 of 15 token rows of the stage never exist in HBM.
    const float* table_tok; int T, NT;
    long long* stamps;                 // TTUP_STAGE_STAMPS=1: [layer][12] clock values of workgroup 0 / wave 0 at the phase boundaries (else null)
};
constexpr int STAGE_QS = 260;         // floats per row of the q | k tile: 4 heads x 64 + 4 (1040 B = 65 slots of 16 B: consecutive rows fall on consecutive slots)
constexpr int STAGE_VS = 84;          // floats per row of V^T [head][dim][token]: 4 x 84 = 16 (mod 64), so a transposed store of 4 dims x 16 tokens per lane group is conflict-free
constexpr size_t STAGE_LDS = (size_t)3 * 64 * 128 * 2 + (size_t)64 * STAGE_QS * 4 + (size_t)4 * 32 * STAGE_VS * 4 + 8 * 16 * 4;
__global__ __launch_bounds__(512) void stage_x3_kernel(StageArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint16_t xh[];       // split planes
    constexpr int BM = 64, K = 128, PLANE = BM * K, KS = K / 32, HD = 32, QS = STAGE_QS, VS = STAGE_VS;
    static_assert(K == X3_K, "the uplift_x3.h blocks are written for 128-wide rows");
    float* att = (float*)xh;                                          // attention output (fp32, swizzled), while the planes are dead
    float* qh = (float*)(xh + 3 * PLANE);                             // q | k of the four heads: [row][head][q|k][32]
    float* s2 = qh;                                                   // fp32 row staging (swizzled), while the q | k tile is dead
    float* vt = qh + BM * QS;                                         // V^T: [head][dim][sequence sl at column sl*S4 + token]
    float* sinv = vt + 4 * HD * VS;
    const int tid = ttup_tid_x(), lane = tid & 63, wave = tid >> 6;
    const int S = a.sv.S, SEQS = BM / S, ROWS = SEQS * S, QT = (S + 15) >> 4, S4 = (S + 3) & ~3;
    const long long seq0 = (long long)ttup_bid_x() * SEQS;
    const long long m0 = seq0 * S, M = a.n_seq * S;
    const int q = lane >> 4, c = lane & 15;
    const int grp = tid >> 4, l16 = tid & 15;
    const int n = wave * 16 + 4 * q;                                  // the lane's four output features in every 128-wide GEMM
    // LayerNorm of row r of s2 (16 lanes per row, 8 features each) -> split planes
    auto ln_split = [&](int r, const f32x4 (&g)[2], const f32x4 (&bt)[2]) __attribute__((always_inline)) {
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
            for (int e = 0; e < 4; ++e) v[u][e] = (v[u][e] - mean) * rstd * g[u][e] + bt[u][e];
        x3_split_store<PLANE>(xh, r, l16, v[0], v[1]);
    };
    // one 16-output weight tile: 4 k-steps x 3 planes, 16 bytes per lane each
    // (the scheduling barriers pin the twelve requests where they are written: left alone, the scheduler sinks them to their
    // first use -- the next GEMM -- to save registers, which is exactly the exposed latency this kernel exists to hide)
    auto load_tile = [&](const uint16_t* __restrict__ w3, int nt, bf16x8 (&w)[3][KS]) __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int p = 0; p < 3; ++p) w[p][s] = *(const bf16x8*)(w3 + ((((size_t)nt * KS + s) * 3 + p) * 64 + lane) * 8);
        __builtin_amdgcn_sched_barrier(0);
    };
    // acc[mt] += W_tile . planes  (64 tokens x 16 outputs x 128 inputs, six partial products smallest first)
    // ---- the tokens: global -> registers (row mt*16 + c, features n .. n+3)
    f32x4 xr[4];
    bool rot[4]; const float2* rrow[4]; int vcol[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int r = mt * 16 + c;
        const long long m = m0 + r;
        const int sl = r / S, jt = r - sl * S;
        const long long sq = seq0 + sl;
        const float* src = a.x + m * K;
        if (a.table_tok) src = jt == 0 ? a.x + sq * K : a.table_tok + ((sq < a.n_seq ? sq / a.T : 0) * a.NT + jt - 1) * K;
        xr[mt] = (r < ROWS && m < M) ? *(const f32x4*)(src + n) : f32x4{0.f, 0.f, 0.f, 0.f};
        rot[mt] = r < ROWS && sq < a.n_seq && jt >= a.sv.num_cls;
        rrow[mt] = a.sv.rope + ((size_t)((rot[mt] ? sq : 0) / a.sv.times_div) * a.sv.times_stride + (rot[mt] ? jt - a.sv.num_cls : 0)) * (HD / 2);
        vcol[mt] = r < ROWS ? sl * S4 + jt : -1;             // the row's column in V^T (rows of no sequence are not stored)
    }
    for (int i = tid; i < 4 * HD * VS + 8 * 16; i += 512) vt[i] = 0.f;          // V^T and the normalisers: never-written columns must read as finite (0 x NaN)
    // bit r: row r of the tile takes part in attention (its mask entry is 0); every wave computes the same 64 bits
    unsigned long long rowbits;
    {
        const int sl = lane / S, jt = lane - sl * S;
        const long long sq = seq0 + sl;
        rowbits = __builtin_amdgcn_ballot_w64(lane < ROWS && sq < a.n_seq && a.sv.mask[(size_t)((lane < ROWS && sq < a.n_seq ? sq : 0) / a.sv.mask_div) * S + jt] == 0.f);
    }
    bf16x8 wnext[3][KS];
    if (a.n_layers > 0) load_tile(a.layers[0].w_qkv, wave, wnext);
    const int hw = wave >> 1, ew = wave & 1;                 // a wave's q / k / v tile: head hw, dims 16 ew .. 16 ew + 15
    for (int li = 0; li < a.n_layers; ++li) {
        const StageLayerW& L = a.layers[li];
        auto stamp = [&](int i) __attribute__((always_inline)) { if (a.stamps && ttup_bid_x() == 0 && tid == 0) a.stamps[li * 12 + i] = (long long)__builtin_readcyclecounter(); };
        stamp(0);
        // ---- 1. LN(x) -> split planes   (small operands are requested BEFORE the weight tile that is issued next: the memory
        // counter retires in order, so waiting for them then does not wait for the tile)
        f32x4 lg[2], lb[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) { lg[u] = *(const f32x4*)(L.g1 + 8 * l16 + 4 * u); lb[u] = *(const f32x4*)(L.b1 + 8 * l16 + 4 * u); }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) *(f32x4*)x3_f32(s2, mt * 16 + c, n) = xr[mt];
        stage_barrier();
        ln_split(grp, lg, lb);
        ln_split(grp + 32, lg, lb);
        stage_barrier();
        stamp(1);
        // ---- 2. q | k | v: tiles wave, 8 + wave, 16 + wave of the 384 outputs (bias; RoPE on q and k)
#pragma unroll
        for (int jp = 0; jp < 3; ++jp) {
            bf16x8 wc[3][KS];
            x3_take(wc, wnext);
            const f32x4 b4 = *(const f32x4*)(L.b_qkv + jp * K + n);
            f32x4 cs4[4];
            if (jp < 2) {
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) cs4[mt] = *(const f32x4*)(rrow[mt] + ew * 8 + 2 * q);
            }
            if (jp < 2) load_tile(L.w_qkv, (jp + 1) * 8 + wave, wnext); else load_tile(L.w_proj, wave, wnext);
            f32x4 acc[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            x3_gemm64<PLANE>(xh, c, q, wc, acc);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                f32x4 v = acc[mt] + b4;
                if (jp < 2 && rot[mt]) {                     // dim pairs (16 ew + 4q, +1) and (+2, +3) of the head
                    const f32x4 cs = cs4[mt];
                    v = f32x4{v[0] * cs[0] - v[1] * cs[1], v[0] * cs[1] + v[1] * cs[0], v[2] * cs[2] - v[3] * cs[3], v[2] * cs[3] + v[3] * cs[2]};
                }
                if (jp < 2) *(f32x4*)(qh + (mt * 16 + c) * QS + hw * 64 + jp * 32 + ew * 16 + 4 * q) = v;
                else if (vcol[mt] >= 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) vt[(hw * HD + ew * 16 + 4 * q + e) * VS + vcol[mt]] = v[e];
                }
            }
        }
        stamp(2);
        stage_barrier();              // qkv complete; every wave is done with the planes: the attention output goes there
        stamp(3);
        // ---- 3. attention: task = (sequence, head, tile of 16 queries)
        for (int task = wave; task < SEQS * 4 * QT; task += 8) {
            const int qt = task % QT, sh = task / QT, h = sh & 3, sl = sh >> 2;
            const long long seq = seq0 + sl;
            if (seq >= a.n_seq) continue;                    // wave-uniform
            const float* base = qh + (sl * S) * QS + h * 64;
            const float* vbase = vt + (h * HD + c) * VS + sl * S4 + 4 * q;          // V^T[dim c][keys 4q ..] of the sequence; dims 16 + c are 16 rows on
            const int i = qt * 16 + c, ir = i < S ? i : S - 1;
            const unsigned long long seqbits = (rowbits >> (sl * S)) & (S >= 64 ? ~0ull : (1ull << S) - 1);          // bit j: key / query j of this sequence is valid
            const bool row_ok = (seqbits >> (i & 63)) & 1 && i < S;
            const unsigned long long colbits = seqbits >> (4 * q);          // bit kt*16 + r: key kt*16 + 4q + r
            const f32x4 q0 = *(const f32x4*)(base + ir * QS + 8 * q), q1 = *(const f32x4*)(base + ir * QS + 8 * q + 4);
            f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
            float den = 0.f;
            // NKT key tiles at once: their score chains are independent (the matrix pipe stays fed) and the scores stay in
            // registers between the maximum and the exponentials; per chain and per output the operation order is
            // attention_mfma_kernel's
            auto attend = [&](auto nkt_c) __attribute__((always_inline)) {
                constexpr int NKT = decltype(nkt_c)::value;
                f32x4 kk[NKT][2], sc[NKT], vv[NKT][2];
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt) {
                    const int jc = kt * 16 + c, jr = jc < S ? jc : S - 1;
                    const float* kp = base + jr * QS + 32 + 8 * q;
                    kk[kt][0] = *(const f32x4*)kp; kk[kt][1] = *(const f32x4*)(kp + 4);
                    sc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int kt = 0; kt < NKT; ++kt) sc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kk[kt][0][e], q0[e], sc[kt], 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int kt = 0; kt < NKT; ++kt) sc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kk[kt][1][e], q1[e], sc[kt], 0, 0, 0);
                // V^T of keys kt*16 + 4q .. + 3, requested once the K fragments are dead (columns past the sequence hold other tokens,
                // zeros or -- past the array -- the normalisers: their p is 0 and all of it is finite, the storage having been cleared once)
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt) { vv[kt][0] = *(const f32x4*)(vbase + kt * 16); vv[kt][1] = *(const f32x4*)(vbase + kt * 16 + 16 * VS); }
                float mx = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const bool col_ok = (colbits >> (kt * 16 + r)) & 1;
                        sc[kt][r] = col_ok ? sc[kt][r] * a.sv.scale : -INFINITY;
                        mx = sc[kt][r] > mx ? sc[kt][r] : mx;
                    }
                { const float o = __shfl_xor(mx, 16, 64); mx = o > mx ? o : mx; }
                { const float o = __shfl_xor(mx, 32, 64); mx = o > mx ? o : mx; }
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt) {
                    float pr[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) { pr[r] = (row_ok && sc[kt][r] > -INFINITY) ? __expf(sc[kt][r] - mx) : 0.f; den += pr[r]; }          // (v_exp_f32: 1 ulp; sixteen libm expf per task were a third of the attention phase)
                    // out += P V with k index (step s, lane group q) <-> key kt*16 + 4q + s: the A operand of step s is the lane's own pr[s]
#pragma unroll
                    for (int s2_ = 0; s2_ < 4; ++s2_) {
                        o0 = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[s2_], vv[kt][0][s2_], o0, 0, 0, 0);
                        o1 = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[s2_], vv[kt][1][s2_], o1, 0, 0, 0);
                    }
                }
            };
            switch (QT) {
                case 1: attend(std::integral_constant<int, 1>{}); break;
                case 2: attend(std::integral_constant<int, 2>{}); break;
                case 3: attend(std::integral_constant<int, 3>{}); break;
                default: attend(std::integral_constant<int, 4>{}); break;
            }
            den += __shfl_xor(den, 16, 64);
            den += __shfl_xor(den, 32, 64);
            // o[r] = out[query qt*16 + 4q + r][dim c (o0) / 16 + c (o1)]: the row's 1 / den comes from the lane that owns that query
            if (q == 0) sinv[wave * 16 + c] = den > 0.f ? 1.f / den : 0.f;          // a fully masked query row yields zeros (torch SDPA semantics)
            __builtin_amdgcn_wave_barrier();
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int io = qt * 16 + 4 * q + r;
                if (io >= S) continue;
                const float inv = sinv[wave * 16 + 4 * q + r];
                *x3_f32(att, sl * S + io, h * HD + c) = o0[r] * inv;
                *x3_f32(att, sl * S + io, h * HD + 16 + c) = o1[r] * inv;
            }
            __builtin_amdgcn_wave_barrier();
        }
        stamp(4);
        stage_barrier();              // att complete, q | k | v consumed
        stamp(5);
        // ---- 4. att (fp32, in the plane storage) -> split planes, through registers
        {
            f32x4 t[2][2];
#pragma unroll
            for (int i = 0; i < 2; ++i) { t[i][0] = *(const f32x4*)x3_f32(att, grp + 32 * i, 8 * l16); t[i][1] = *(const f32x4*)x3_f32(att, grp + 32 * i, 8 * l16 + 4); }
            stage_barrier();
#pragma unroll
            for (int i = 0; i < 2; ++i) x3_split_store<PLANE>(xh, grp + 32 * i, l16, t[i][0], t[i][1]);
        }
        stage_barrier();
        stamp(6);
        // ---- 5. x2 = proj(att) + x (stays in the lane); a copy goes to s2 for the LayerNorm
        f32x4 x2[4];
        {
            bf16x8 wc[3][KS];
            x3_take(wc, wnext);
#pragma unroll
            for (int u = 0; u < 2; ++u) { lg[u] = *(const f32x4*)(L.g2 + 8 * l16 + 4 * u); lb[u] = *(const f32x4*)(L.b2 + 8 * l16 + 4 * u); }
            load_tile(L.w_fc1, wave, wnext);
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
        stamp(7);
        ln_split(grp, lg, lb);
        ln_split(grp + 32, lg, lb);
        stage_barrier();
        stamp(8);
        // ---- 6. hid = relu(fc1(LN(x2)) + b1) -> s2 -> split planes
        {
            bf16x8 wc[3][KS];
            x3_take(wc, wnext);
            const f32x4 b4 = *(const f32x4*)(L.bias1 + n);
            load_tile(L.w_fc2, wave, wnext);
            f32x4 acc[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            x3_gemm64<PLANE>(xh, c, q, wc, acc);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                f32x4 v = acc[mt] + b4;
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
        stamp(9);
        // ---- 7. x = fc2(hid) + b2 + x2
        {
            bf16x8 wc[3][KS];
            x3_take(wc, wnext);
            const f32x4 b4 = *(const f32x4*)(L.bias2 + n);
            if (li + 1 < a.n_layers) load_tile(a.layers[li + 1].w_qkv, wave, wnext);
            f32x4 acc[4];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            x3_gemm64<PLANE>(xh, c, q, wc, acc);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) xr[mt] = (acc[mt] + b4) + x2[mt];
        }
        stamp(10);
        stage_barrier();              // every wave is done with the planes and with s2
        stamp(11);
    }
    // ---- the tokens: registers -> global
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int r = mt * 16 + c;
        const long long m = m0 + r;
        if (!(r < ROWS && m < M)) continue;
        if (!a.table_tok) *(f32x4*)(a.x + m * K + n) = xr[mt];
        else {
            const int sl = r / S;
            if (r == sl * S) *(f32x4*)(a.x + (seq0 + sl) * K + n) = xr[mt];
        }
    }
}

}  // namespace
