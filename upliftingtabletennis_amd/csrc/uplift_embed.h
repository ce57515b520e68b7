// The uplift forward's own token kernels (the ones the training pass shares are in uplift_tokens.h): cls strip, by-index RoPE table, the two embeddings.
// Private to csrc/uplift.hip, which includes it after uplift_x3.h inside its no-packed-fp32 region; no other unit may include it.
#pragma once

namespace {

// y[b, t] = x[b, 1+t] on rows of 3 floats: the position head of 'singlestage' runs over all T+1 rows of every sequence (model.py:495-497)
__global__ void strip_cls3_kernel(const float* x, float* y, int T, long long total) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= total) return;
    const int c = (int)(i % 3);
    const long long r = i / 3;
    const long long b = r / T; const int t = (int)(r % T);
    y[i] = x[(b * (T + 1) + 1 + t) * 3 + c];
}
// rope[r][i] = (cos, sin)(r * inv_freq[i]): time_rotation 'old' turns by the token's index in the sequence (model.py:73-75)
__global__ void rope_index_kernel(const float* inv_freq, float2* rope, int half, long long total) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= total) return;
    const float f = (float)(i / half) * inv_freq[i % half];
    rope[i] = make_float2(cosf(f), sinf(f));
}
// Modes 'stacked' / 'originalmethod' (model.py:345-353): h[b,t] = relu(fc1([ball[b,t], table[b] flattened])), K = 2 + 13*TW with
// TW = 3 (x, y, visibility) or 2.  The stacked (B,T,K) input is never built: a workgroup serves 32 tokens of ONE trajectory, reduces
// the table columns of fc1 (and the bias) once into LDS, and adds the two ball columns per token.  wt is fc1.weight transposed [K][D].
// PER_TOKEN: every output sums its K products in column order instead, bias last (the order of a plain linear layer over the
// stacked input; TTUP_UPLIFT_STACKED_PER_TOKEN, the cross-check of the summation order).
constexpr int STACKED_TOKENS = 32;
template <bool PER_TOKEN>
__global__ __launch_bounds__(256) void stacked_embed_kernel(const float* __restrict__ ball, const float* __restrict__ table, const float* __restrict__ wt,
                                                            const float* __restrict__ bias, float* __restrict__ out, int T, int D, int TW) {
    __shared__ float tab[39];
    __shared__ float c[256];          // D <= 256 (ttup_uplift_create)
    const int b = ttup_bid_x(), t0 = ttup_bid_y() * STACKED_TOKENS, tid = ttup_tid_x();
    const int KT = 13 * TW;
    if (tid < KT) tab[tid] = table[((size_t)b * 13 + tid / TW) * 3 + tid % TW];
    __syncthreads();
    if (!PER_TOKEN) {
        if (tid < D) {
            float acc = bias[tid];
            for (int k = 0; k < KT; ++k) acc = fmaf(tab[k], wt[(size_t)(2 + k) * D + tid], acc);
            c[tid] = acc;
        }
        __syncthreads();
    }
    const int nt = T - t0 < STACKED_TOKENS ? T - t0 : STACKED_TOKENS;
    for (int i = tid; i < nt * D; i += 256) {
        const int t = t0 + i / D, n = i % D;
        const float* bp = ball + ((size_t)b * T + t) * 2;
        float v;
        if (PER_TOKEN) {
            v = fmaf(bp[1], wt[D + n], bp[0] * wt[n]);
            for (int k = 0; k < KT; ++k) v = fmaf(tab[k], wt[(size_t)(2 + k) * D + n], v);
            v += bias[n];
        } else v = fmaf(bp[1], wt[D + n], fmaf(bp[0], wt[n], c[n]));
        out[((size_t)b * T + t) * D + n] = v > 0.f ? v : 0.f;
    }
}
// 'multistage' (model.py:549-560): x[b, 0] = cls, x[b, 1+t] = embed(pos[b, t]) = fc2(relu(fc1(pos))) with fc1 3 -> D, fc2 D -> D.
// A workgroup serves 16 tokens: the hidden rows go to LDS, then thread (n, half) accumulates 8 tokens of output column n over k
// (w2t = fc2.weight transposed [D][D]: consecutive n read consecutive words, the hidden values are LDS broadcasts).
constexpr int EMBED3_TOKENS = 16;
__global__ __launch_bounds__(256) void embed3_cls_kernel(const float* __restrict__ pos, const float* __restrict__ w1t, const float* __restrict__ b1,
                                                         const float* __restrict__ w2t, const float* __restrict__ b2, const float* __restrict__ cls,
                                                         float* __restrict__ x, int T, int D, long long tokens) {
    __shared__ float h[EMBED3_TOKENS][256];          // D <= 256
    const int tid = ttup_tid_x();
    const long long r0 = (long long)ttup_bid_x() * EMBED3_TOKENS;
    for (int i = tid; i < EMBED3_TOKENS * D; i += 256) {
        const int j = i / D, n = i % D;
        const long long r = r0 + j;
        float v = 0.f;
        if (r < tokens) {
            const float* p = pos + r * 3;
            v = fmaf(p[2], w1t[2 * D + n], fmaf(p[1], w1t[D + n], fmaf(p[0], w1t[n], b1[n])));
            v = v > 0.f ? v : 0.f;
        }
        h[j][n] = v;
    }
    __syncthreads();
    for (int i = tid; i < 2 * D; i += 256) {
        const int n = i % D, j0 = (i / D) * (EMBED3_TOKENS / 2);
        float acc[EMBED3_TOKENS / 2];
#pragma unroll
        for (int j = 0; j < EMBED3_TOKENS / 2; ++j) acc[j] = b2[n];
        for (int k = 0; k < D; ++k) {
            const float w = w2t[(size_t)k * D + n];
#pragma unroll
            for (int j = 0; j < EMBED3_TOKENS / 2; ++j) acc[j] = fmaf(h[j0 + j][k], w, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < EMBED3_TOKENS / 2; ++j) {
            const long long r = r0 + j0 + j;
            if (r < tokens) x[((r / T) * (T + 1) + 1 + r % T) * D + n] = acc[j];
        }
    }
    // the cls rows of the trajectories that START in this tile
    for (int j = 0; j < EMBED3_TOKENS; ++j) {
        const long long r = r0 + j;
        if (r < tokens && r % T == 0)
            for (int n = tid; n < D; n += 256) x[(r / T) * (T + 1) * D + n] = cls[n];
    }
}

}  // namespace
