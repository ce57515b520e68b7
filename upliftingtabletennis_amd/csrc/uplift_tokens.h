// Token plumbing of the uplift transformer shared by the forward (csrc/uplift.hip) and the training pass (csrc/uplift_grad.hip):
// token assembly, masks, the RoPE table, the spin frame change.  The kernels sit in an unnamed namespace: each of the two units
// gets its own copy in its own code object, under the names it had.
#pragma once
#include "common.h"
#include <math.h>

namespace {

using namespace ttup;

// rope[r][i] = (cos, sin)(round(t_r / 0.002) * inv_freq[i]) for every time stamp r           (model.py:62-80)
__global__ void rope_table_kernel(const float* times, const float* inv_freq, float2* rope, int half, long long total) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= total) return;
    const float pos = rintf(times[i / half] / 0.002f);          // round(t / (1/MAX_FPS)), model.py:72
    const float f = pos * inv_freq[i % half];
    rope[i] = make_float2(cosf(f), sinf(f));
}
// x[(b,t), 0] = ball_tok[b,t]; x[(b,t), 1+n] = table_tok[b,n]      (model.py:374-378)
__global__ void assemble_table_kernel(const float* ball_tok, const float* table_tok, float* x, int T, int NT, int D, long long total) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= total) return;
    const int d = (int)(i % D);
    long long r = i / D;
    const int n = (int)(r % (NT + 1)); r /= (NT + 1);      // r = b*T + t
    x[i] = n == 0 ? ball_tok[r * D + d] : table_tok[((r / T) * NT + (n - 1)) * D + d];
}
// y[r] = x[r*stride_tok] rows (token 0 of every sequence)            (model.py:383-384)
__global__ void gather_rows_kernel(const float* x, float* y, int D, int seq_tokens, long long total) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= total) return;
    const int d = (int)(i % D);
    const long long r = i / D;
    y[i] = x[(r * seq_tokens) * D + d];
}
// y[b, 0] = cls; y[b, 1+t] = x[b, t]                                 (model.py:560)
__global__ void prepend_cls_kernel(const float* x, const float* cls, float* y, int T, int D, long long total) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (i >= total) return;
    const int d = (int)(i % D);
    long long r = i / D;
    const int t = (int)(r % (T + 1)); const long long b = r / (T + 1);
    y[i] = t == 0 ? cls[d] : x[(b * T + (t - 1)) * D + d];
}
// masks: mask (B,T) {0,1} -> additive m1 (B,T), m2 (B,T+1) with leading 0; table (B,13,3) -> tmask (B,14), txy (B*13,2).
// FLAGS (the forward): *flags collects what values the mask holds, for the format check; else `flags` is not touched.
template <bool FLAGS>
__global__ void prepare_kernel(const float* mask, const float* table, float* m1, float* m2, float* tmask, float* txy, int B, int T, int NT, int* flags) {
    const long long i = (long long)ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    const long long nmask = (long long)B * T, ntab = (long long)B * NT;
    int fl = 0;
    if (i < nmask) {
        const float m = mask[i];
        const float add = m == 0.f ? -INFINITY : 0.f;
        m1[i] = add;
        const long long b = i / T; const int t = (int)(i % T);
        m2[b * (T + 1) + 1 + t] = add;
        if (t == 0) m2[b * (T + 1)] = 0.f;
        // bit0: some m==0, bit1: some m==1, bit2: some m<0, bit3: some m>1  (min==0 && max==1  <=>  flags==3)
        if (FLAGS) fl = m == 0.f ? 1 : m == 1.f ? 2 : m < 0.f ? 4 : 8;
    } else if (i < nmask + ntab) {
        const long long j = i - nmask;
        const long long b = j / NT; const int n = (int)(j % NT);
        tmask[b * (NT + 1) + 1 + n] = table[j * 3 + 2] == 1.f ? 0.f : -INFINITY;      // KEYPOINT_VISIBLE == 1, model.py:363
        if (n == 0) tmask[b * (NT + 1)] = 0.f;
        txy[j * 2] = table[j * 3]; txy[j * 2 + 1] = table[j * 3 + 1];
    }
    if (!FLAGS) return;
    // one atomic per wave (every thread used to hit the one flag word: 1.4 ms per call at B = 10 000)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) fl |= __shfl_xor(fl, off, 64);
    if ((ttup_tid_x() & 63) == 0 && fl) atomicOr(flags, fl);
}
// transform_rotationaxes (uplifting/helper.py:394-420)
__global__ void rotationaxes_kernel(const float* rot, const float* pos, int B, int T, float* out) {
    const int b = ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (b >= B) return;
    const float* p = pos + (size_t)b * T * 3;
    const float vx = p[3] - p[0], vy = p[4] - p[1];
    const float nrm = sqrtf(vx * vx + vy * vy);
    const float ex = vx / nrm, ey = vy / nrm;            // e_x = (ex, ey, 0); e_y = e_z x e_x = (-ey, ex, 0)
    const float* r = rot + (size_t)b * 3;
    out[b * 3 + 0] = r[0] * ex + r[1] * ey + r[2] * 0.f;
    out[b * 3 + 1] = r[0] * (-ey) + r[1] * ex + r[2] * 0.f;
    out[b * 3 + 2] = r[0] * 0.f + r[1] * 0.f + r[2] * 1.f;
}

}  // namespace
