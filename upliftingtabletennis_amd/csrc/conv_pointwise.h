// One-thread-per-output kernels: the fp32 direct conv (cross-check), fuse-layer sum, layout changes, head, pre-processing.
#pragma once
#include "conv_dev.h"
#include "conv.h"

namespace ttup {

// ------------------------------------------------------------------ fp32 direct path (parity/debug)
struct ConvFArgs {
    const float* src0; const float* src1; const float* w; const float* bias; const float* residual; float* dst;
    int c0, c1, cout, ks, stride, H, W, OH, OW, relu;
    long long total;
};

__global__ void conv_direct_f32_kernel(ConvFArgs a) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const int co = (int)(i % a.cout);
    long long p = i / a.cout;
    const int ox = (int)(p % a.OW); p /= a.OW;
    const int oy = (int)(p % a.OH);
    const int b = (int)(p / a.OH);
    const int pad = a.ks / 2, cin = a.c0 + a.c1;
    float acc = 0.f;
    for (int dy = 0; dy < a.ks; ++dy) {
        const int gy = oy * a.stride - pad + dy;
        if (gy < 0 || gy >= a.H) continue;
        for (int dx = 0; dx < a.ks; ++dx) {
            const int gx = ox * a.stride - pad + dx;
            if (gx < 0 || gx >= a.W) continue;
            const size_t pix = (size_t)(b * a.H + gy) * a.W + gx;
            const float* wt = a.w + (size_t)((dy * a.ks + dx) * cin) * a.cout + co;
            const float* s0 = a.src0 + pix * a.c0;
            for (int c = 0; c < a.c0; ++c) acc = fmaf(s0[c], wt[(size_t)c * a.cout], acc);
            if (a.c1) {
                const float* s1 = a.src1 + pix * a.c1;
                const float* wt1 = wt + (size_t)a.c0 * a.cout;
                for (int c = 0; c < a.c1; ++c) acc = fmaf(s1[c], wt1[(size_t)c * a.cout], acc);
            }
        }
    }
    acc += a.bias[co];
    if (a.residual) acc += a.residual[i];
    if (a.relu) acc = acc > 0.f ? acc : 0.f;
    a.dst[i] = acc;
}

// ------------------------------------------------------------------ pointwise kernels
template <typename T> __device__ __forceinline__ float ld(const T* p);
template <> __device__ __forceinline__ float ld<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ld<bf16_t>(const bf16_t* p) { return bf16_to_f32(*p); }
template <typename T> __device__ __forceinline__ void st(T* p, float v);
template <> __device__ __forceinline__ void st<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void st<bf16_t>(bf16_t* p, float v) { *p = f32_to_bf16(v); }

struct UpsumArgs { const void* base; const void* t[3]; int shift[3]; int n; void* dst; int H, W, C; long long total; const int* n_active; long long per_sample; Roi roi; int batch; };

template <typename T>
__global__ void upsum_kernel(UpsumArgs a) {
    // every sample's whole tensor is walked; samples whose pruning flag is set produce only the op's cone region
    int nb = a.batch;
    if (a.n_active) nb = *a.n_active < nb ? *a.n_active : nb;
    const long long total = (long long)nb * a.H * a.W * a.C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % a.C);
        long long p = i / a.C;
        const int x = (int)(p % a.W); p /= a.W;
        const int y = (int)(p % a.H);
        const int b = (int)(p / a.H);
        if (a.roi.flag) { const int f = a.roi.flag[b]; if (f != 0 && a.roi.outside(f, y, x)) continue; }
        float v = ld((const T*)a.base + i);
        for (int k = 0; k < a.n; ++k) {
            const int sh = a.shift[k], hh = a.H >> sh, ww = a.W >> sh;
            v += ld((const T*)a.t[k] + ((size_t)(b * hh + (y >> sh)) * ww + (x >> sh)) * a.C + c);
        }
        st((T*)a.dst + i, v > 0.f ? v : 0.f);
    }
}

// bf16 fast path: one lane = 8 channels (16 bytes) of one pixel; low-resolution terms are re-read by the 2^shift
// neighbours from L1/L2
__global__ __launch_bounds__(256) void upsum_bf16x8_kernel(UpsumArgs a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // over b*h*w*(C/8)
    if (i >= a.total) return;
    const int c8n = a.C >> 3;
    const int c8 = (int)(i % c8n);
    long long p = i / c8n;
    const int x = (int)(p % a.W); p /= a.W;
    const int y = (int)(p % a.H);
    const int b = (int)(p / a.H);
    float v[8];
    {
        const u32x4 r = *((const u32x4*)a.base + i);
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[2 * k] = bf16_to_f32((bf16_t)(w[k] & 0xffff)); v[2 * k + 1] = bf16_to_f32((bf16_t)(w[k] >> 16)); }
    }
    for (int t = 0; t < a.n; ++t) {
        const int sh = a.shift[t], hh = a.H >> sh, ww = a.W >> sh;
        add_bf16x8(v, *((const u32x4*)a.t[t] + ((size_t)(b * hh + (y >> sh)) * ww + (x >> sh)) * c8n + c8));
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
    *((u32x4*)a.dst + i) = u32x4{pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
}

template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* src, T* dst, int cin, int cpad, int hw, long long total) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // over b*hw*cpad
    if (i >= total) return;
    const int c = (int)(i % cpad);
    const long long p = i / cpad;
    const int b = (int)(p / hw), pix = (int)(p % hw);
    st(dst + i, c < cin ? src[((size_t)b * cin + c) * hw + pix] : 0.f);
}

template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* src, float* dst, int c, int hw, long long total) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // over b*c*hw (dst order)
    if (i >= total) return;
    const int pix = (int)(i % hw);
    const long long q = i / hw;
    const int ch = (int)(q % c), b = (int)(q / c);
    dst[i] = ld(src + ((size_t)b * hw + pix) * c + ch);
}

// head: 1x1 conv 16 -> n_out selected output channels (+bias), fp32 NCHW (B, n_out, H, W) out
template <typename T, int CIN>
__global__ void head_kernel(const T* src, const float* w, const float* bias, int n_out, float* heat, long long hw, long long npix_max, const int* n_active, Roi roi, int W) {
    long long nb = npix_max / hw;
    if (n_active) nb = *n_active < nb ? *n_active : nb;
    const long long npix = nb * hw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long long)gridDim.x * blockDim.x) {
        if (roi.flag) {
            const long long bq = i / hw, rem = i - bq * hw;
            const int y = (int)(rem / W), xq = (int)(rem % W);
            const int f = roi.flag[bq];
            if (f != 0 && roi.outside(f, y, xq)) continue;
        }
        float x[CIN];
#pragma unroll
        for (int c = 0; c < CIN; ++c) x[c] = ld(src + i * CIN + c);
        const long long b = i / hw, pix = i % hw;
        for (int k = 0; k < n_out; ++k) {
            float acc = 0.f;
#pragma unroll
            for (int c = 0; c < CIN; ++c) acc = fmaf(x[c], w[k * CIN + c], acc);
            heat[(b * n_out + k) * hw + pix] = acc + bias[k];
        }
    }
}

// ------------------------------------------------------------------ a1: uint8 frames -> normalised triples
// OpenCV INTER_LINEAR on uint8 (fixed point, 11-bit coefficients) + (x/255 - mean)/std, see
// oracle/glue_ref.py for the algorithm statement.  Parity of the resize is unpinned (cv2 absent offline).
struct PreArgs {
    const uint8_t* frames; void* out; int src_h, src_w, dst_h, dst_w, first_triple, n_triples, layout; long long total;
    double scale_x, scale_y;
    int nf;                // frames per sample: 3 (ball triples t,t+1,t+2) or 1 (table detector, single frame)
    const float* lut;      // [3][256]: (v/255 - mean[c]) / std[c] evaluated in fp64 on the host, rounded to fp32
    // crop mode (certified argmax): output sample j is the crop_h x crop_w window at (y0, x0) of sample `frame`, as crops[crop0 + j]
    // (csrc/certify_plan.h CropRec) says; only the first *n_active samples are produced
    const CropRec* crops; const int* n_active; int crop0, crop_h, crop_w;
};

__device__ __forceinline__ int cv_round(float v) { return (int)rintf(v); }

__device__ __forceinline__ void axis_tap_x(int d, double scale, int src_n, int& i0, int& i1, int& c0, int& c1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= src_n - 1) { f = 0.f; s = src_n - 1; }
    i0 = s; i1 = s + 1 < src_n ? s + 1 : src_n - 1;
    c1 = cv_round(f * 2048.f); c0 = cv_round((1.f - f) * 2048.f);
}
__device__ __forceinline__ void axis_tap_y(int d, double scale, int src_n, int& i0, int& i1, int& c0, int& c1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    i0 = s < 0 ? 0 : (s > src_n - 1 ? src_n - 1 : s);
    i1 = s + 1 < 0 ? 0 : (s + 1 > src_n - 1 ? src_n - 1 : s + 1);
    c1 = cv_round(f * 2048.f); c0 = cv_round((1.f - f) * 2048.f);
}

template <typename T>
__global__ void preprocess_kernel(PreArgs a) {
    // one thread per (sample, y, x): produces the 3*nf channels of that pixel.  Whole frames run on a 3-D grid (column block,
    // row, sample) -- no index division, which used to be most of this kernel's instructions; crop windows keep a linear index
    int x, y, t;
    size_t opix;                        // output pixel index (sample-major)
    if (a.crops) {
        const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= (unsigned)a.total) return;
        const int cx = (int)(i % (unsigned)a.crop_w);
        const unsigned p = i / (unsigned)a.crop_w;
        const int cy = (int)(p % (unsigned)a.crop_h);
        const int j = (int)(p / (unsigned)a.crop_h);
        if (j >= *a.n_active) return;
        const CropRec rec = a.crops[a.crop0 + j];
        t = rec.frame; y = rec.y0 + cy; x = rec.x0 + cx;
        opix = ((size_t)j * a.crop_h + cy) * a.crop_w + cx;
    } else {
        x = blockIdx.x * blockDim.x + threadIdx.x; y = blockIdx.y; t = blockIdx.z;
        if (x >= a.dst_w) return;
        opix = ((size_t)t * a.dst_h + y) * a.dst_w + x;
    }
    const bool same = a.src_h == a.dst_h && a.src_w == a.dst_w;
    int x0 = x, x1 = x, a0 = 2048, a1 = 0, y0 = y, y1 = y, b0 = 2048, b1 = 0;
    if (!same) {
        axis_tap_x(x, a.scale_x, a.src_w, x0, x1, a0, a1);
        axis_tap_y(y, a.scale_y, a.src_h, y0, y1, b0, b1);
    }
    float vals[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) vals[k] = 0.f;
    // the three channel bytes of a source pixel come in one unaligned 4-byte load (the fourth byte is the next pixel's
    // first channel); only the very last pixel of the clip falls back to byte loads so that nothing is read past the end
    typedef unsigned int __attribute__((aligned(1))) u32_unaligned;
    const size_t frame_bytes = (size_t)a.src_h * a.src_w * 3;
    const uint8_t* clip_last = a.frames + (size_t)(a.first_triple + a.n_triples + a.nf - 1) * frame_bytes - 4;
    auto load3 = [&](const uint8_t* q) -> unsigned {
        if (q <= clip_last) return *(const u32_unaligned*)q;
        return (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
    };
    for (int f = 0; f < a.nf; ++f) {
        const uint8_t* img = a.frames + (size_t)(a.first_triple + t + f) * frame_bytes;
        if (same) {
            const unsigned w = load3(img + ((size_t)y * a.src_w + x) * 3);
#pragma unroll
            for (int c = 0; c < 3; ++c) vals[f * 3 + c] = a.lut[c * 256 + ((w >> (8 * c)) & 255)];
            continue;
        }
        // a tap with weight 0 (equal widths: every second x tap; integer row positions) is not loaded: 0 * v adds nothing
        const unsigned p00 = load3(img + ((size_t)y0 * a.src_w + x0) * 3);
        const unsigned p01 = a1 ? load3(img + ((size_t)y0 * a.src_w + x1) * 3) : 0u;
        const unsigned p10 = b1 ? load3(img + ((size_t)y1 * a.src_w + x0) * 3) : 0u;
        const unsigned p11 = (a1 && b1) ? load3(img + ((size_t)y1 * a.src_w + x1) * 3) : 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sh = 8 * c;
            const int top = (int)((p00 >> sh) & 255) * a0 + (int)((p01 >> sh) & 255) * a1;
            const int bot = (int)((p10 >> sh) & 255) * a0 + (int)((p11 >> sh) & 255) * a1;
            int v = (((b0 * (top >> 4)) >> 16) + ((b1 * (bot >> 4)) >> 16) + 2) >> 2;
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
            vals[f * 3 + c] = a.lut[c * 256 + v];
        }
    }
    const size_t hw = (size_t)a.dst_h * a.dst_w, pix = (size_t)y * a.dst_w + x;
    if (a.layout == TTUP_LAYOUT_NHWC4_FRAME) {          // one 4-channel bf16 record per frame pixel (stem frames mode)
        *(u32x2*)((bf16_t*)a.out + opix * 4) = u32x2{pack2(vals[0], vals[1]), pack2(vals[2], 0.f)};
        return;
    }
    if (a.layout == TTUP_LAYOUT_NCHW_F32) {
        float* o = (float*)a.out + (size_t)t * 3 * a.nf * hw + pix;
        for (int c = 0; c < 3 * a.nf; ++c) o[c * hw] = vals[c];
    } else {
        T* o = (T*)a.out + opix * 16;
        if (sizeof(T) == 2) {
            u32x4* o4 = (u32x4*)o;
            o4[0] = u32x4{pack2(vals[0], vals[1]), pack2(vals[2], vals[3]), pack2(vals[4], vals[5]), pack2(vals[6], vals[7])};
            o4[1] = u32x4{pack2(vals[8], 0.f), 0u, 0u, 0u};
        } else {
            for (int c = 0; c < 16; ++c) st(o + c, c < 9 ? vals[c] : 0.f);
        }
    }
}

// Frame records (one 4-channel bf16 record per pixel of ONE frame: the production input of the stem) when source and network
// width are equal, as for 1280x720 frames at 1280x704 -- the horizontal taps are (2048, 0), only rows are interpolated.  Four
// pixels of four rows per thread: the 12 source bytes of a row are three aligned words, the normalisation table sits in LDS (the general
// kernel's three dependent table loads per pixel from memory were what it waited for), two 16-byte stores.  Same integer arithmetic
// per pixel as preprocess_kernel: bit-identical records.
constexpr int PRE4_ROWS = 4;          // output rows per workgroup: the table load and its barrier are paid once for 4096 pixels
__global__ __launch_bounds__(256) void preprocess_frames4_kernel(PreArgs a) {
    __shared__ float s_lut[768];
    const int x = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4, yb = (int)blockIdx.y * PRE4_ROWS, t = blockIdx.z;
    const bool live = x < a.dst_w;
    const uint8_t* img = a.frames + (size_t)(a.first_triple + t) * a.src_h * a.src_w * 3;
    int b0[PRE4_ROWS], b1[PRE4_ROWS];
    u32x4 r0[PRE4_ROWS], r1[PRE4_ROWS];
    // all loads of the workgroup's rows first (one memory round trip), the table while they travel
#pragma unroll
    for (int r = 0; r < PRE4_ROWS; ++r) {
        const int y = yb + r;
        int y0 = y, y1 = y;
        b0[r] = 2048; b1[r] = 0;
        r0[r] = u32x4{0u, 0u, 0u, 0u}; r1[r] = u32x4{0u, 0u, 0u, 0u};
        if (y >= a.dst_h) continue;
        if (a.src_h != a.dst_h) axis_tap_y(y, a.scale_y, a.src_h, y0, y1, b0[r], b1[r]);
        if (live) {
            const unsigned* p0 = (const unsigned*)(img + ((size_t)y0 * a.src_w + x) * 3);
            r0[r] = u32x4{p0[0], p0[1], p0[2], 0u};
            if (b1[r]) {                                     // wave-uniform (a row property): a tap with weight 0 is not loaded
                const unsigned* p1 = (const unsigned*)(img + ((size_t)y1 * a.src_w + x) * 3);
                r1[r] = u32x4{p1[0], p1[1], p1[2], 0u};
            }
        }
    }
    for (int k = threadIdx.x; k < 768; k += 256) s_lut[k] = a.lut[k];
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int r = 0; r < PRE4_ROWS; ++r) {
        const int y = yb + r;
        if (y >= a.dst_h) break;
        const unsigned w0[3] = {r0[r].x, r0[r].y, r0[r].z}, w1[3] = {r1[r].x, r1[r].y, r1[r].z};
        unsigned rec[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int i = 3 * j + c;
                const int top = (int)((w0[i >> 2] >> (8 * (i & 3))) & 255) * 2048;
                const int bot = (int)((w1[i >> 2] >> (8 * (i & 3))) & 255) * 2048;
                int q = (((b0[r] * (top >> 4)) >> 16) + ((b1[r] * (bot >> 4)) >> 16) + 2) >> 2;
                q = q < 0 ? 0 : (q > 255 ? 255 : q);
                v[c] = s_lut[c * 256 + q];
            }
            rec[2 * j] = pack2(v[0], v[1]); rec[2 * j + 1] = pack2(v[2], 0.f);
        }
        u32x4* o = (u32x4*)((bf16_t*)a.out + (((size_t)t * a.dst_h + y) * a.dst_w + x) * 4);
        o[0] = u32x4{rec[0], rec[1], rec[2], rec[3]};
        o[1] = u32x4{rec[4], rec[5], rec[6], rec[7]};
    }
}

}  // namespace ttup
