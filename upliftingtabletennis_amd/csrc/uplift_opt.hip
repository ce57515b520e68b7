// The uplift transformer's optimizer step on the device (include/ttup.h): what uplifting/train.py:129-132 does after loss.backward() --
// torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0), torch.optim.Adam.step(), update_ema -- on the flat gradient buffer of
// ttup_uplift_loss_grad and the handle's plain fp32 weights (ttup_uplift::plain, the only weights the gradient pass reads).
//
// Three launches, no host synchronisation, no floating-point atomics:
//   1. sqsum_kernel   per-block partial sums of grad^2 in fp64, a fixed tree (the element -> thread -> block assignment depends on
//                     the length alone, not on the buffer's alignment)
//   2. norm_kernel    one block adds the partials in fixed order; total norm and clip coefficient -> two device floats
//   3. step_kernel    one pass: reads g, p, m, v, ema, writes p, m, v, ema (36 bytes per parameter), 16-byte accesses with scalar
//                     handling of the group that straddles the hole, of the tail and of unaligned buffers
//
// Arithmetic: fp32, in the operation order of torch 2.x's CPU kernels for the same calls, which is what the parity test compares
// with bit for bit.  torch fuses two of them (the lerp of exp_avg and the last addition of addcmul are fmadd in its vectorised
// kernels) and no other; the unit is compiled with contraction off (the pragma below) and writes those two as explicit fma, so the
// compiler adds none of its own.
#include "no_packed_fp32_begin.h"
#include "uplift_net.h"

#include <math.h>
#include <memory>

#pragma clang fp contract(off)

using namespace ttup;
using namespace ttup::upl;

namespace {

constexpr int OPT_THREADS = 256;          // threads per block of all three kernels
constexpr int OPT_MAX_BLOCKS = 1024;      // partial sums of the norm (scratch: that many doubles, then {norm, clip coefficient})

struct Hyper {
    float w1, beta2, w2, bc2_sqrt, eps, neg_step_size, ema_a, ema_b, max_norm;
};

// thread t of block b takes the groups of four elements b * 256 + t, + gridDim * 256, ...; VEC: the buffer is 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(OPT_THREADS) void sqsum_kernel(const float* __restrict__ g, long long n, double* __restrict__ partial) {
    __shared__ double sm[OPT_THREADS];
    const int tid = ttup_tid_x();
    const long long groups = (n + 3) / 4, stride = (long long)ttup_gsize_x();
    double acc = 0.0;
    for (long long q = (long long)ttup_bid_x() * OPT_THREADS + tid; q < groups; q += stride) {
        const long long i = q * 4;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (i + 3 < n) {
            if (VEC) {
                const float4 v = *reinterpret_cast<const float4*>(g + i);
                x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
            } else {
                x[0] = g[i]; x[1] = g[i + 1]; x[2] = g[i + 2]; x[3] = g[i + 3];
            }
        } else {
            for (int k = 0; k < 4; ++k) if (i + k < n) x[k] = g[i + k];
        }
        for (int k = 0; k < 4; ++k) acc = acc + (double)x[k] * (double)x[k];
    }
    sm[tid] = acc;
    __syncthreads();
    for (int off = OPT_THREADS / 2; off >= 1; off >>= 1) {
        if (tid < off) sm[tid] = sm[tid] + sm[tid + off];
        __syncthreads();
    }
    if (tid == 0) partial[ttup_bid_x()] = sm[0];
}

// scalars[0] = ||g||_2, scalars[1] = min(1, max_norm / (norm + 1e-6)) as clip_grad_norm_ computes it in fp32:
// max_norm / x is x.reciprocal() * max_norm there, and the clamp lets a NaN through
__global__ __launch_bounds__(OPT_THREADS) void norm_kernel(const double* __restrict__ partial, int n_partial, float max_norm, float* __restrict__ scalars,
                                                            float* __restrict__ norm_out) {
    __shared__ double sm[OPT_THREADS];
    const int tid = ttup_tid_x();
    double acc = 0.0;
    for (int i = tid; i < n_partial; i += OPT_THREADS) acc = acc + partial[i];
    sm[tid] = acc;
    __syncthreads();
    for (int off = OPT_THREADS / 2; off >= 1; off >>= 1) {
        if (tid < off) sm[tid] = sm[tid] + sm[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        const float norm = (float)sqrt(sm[0]);
        const float coef = (1.0f / (norm + 1e-6f)) * max_norm;
        scalars[0] = norm;
        scalars[1] = coef > 1.0f ? 1.0f : coef;
        if (norm_out) norm_out[0] = norm;
    }
}

// one parameter: clip, Adam, EMA in torch's order (header of this file)
__device__ __forceinline__ void step_one(float g, float clip, const Hyper& h, float& p, float& m, float& v, float& e) {
    g = g * clip;                                            // clip_grad_norm_: g.mul_(clip_coef_clamped)
    m = __builtin_fmaf(h.w1, g - m, m);                      // exp_avg.lerp_(grad, 1 - beta1)
    v = __builtin_fmaf(h.w2 * g, g, v * h.beta2);            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;       // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p + (h.neg_step_size * m) / denom;                   // param.addcdiv_(exp_avg, denom, value=-step_size)
    e = h.ema_a * e + h.ema_b * p;                           // update_ema: alpha * ema + (1 - alpha) * param
}

// 16 bytes at once where the address is known to be 16-byte aligned (VEC, a compile-time choice: one global_load / global_store
// _dwordx4 each); four separate words otherwise, which the compiler may merge into wider unaligned accesses -- the hardware takes those
typedef float vec4f __attribute__((ext_vector_type(4), aligned(16)));
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* a) {
    if (VEC) {
        const vec4f x = *reinterpret_cast<const vec4f*>(__builtin_assume_aligned(a, 16));
        return make_float4(x.x, x.y, x.z, x.w);
    }
    return make_float4(a[0], a[1], a[2], a[3]);
}
template <bool VEC>
__device__ __forceinline__ void store4(float* a, const float4& x) {
    if (VEC) {
        vec4f y = {x.x, x.y, x.z, x.w};
        *reinterpret_cast<vec4f*>(__builtin_assume_aligned(a, 16)) = y;
        return;
    }
    a[0] = x.x; a[1] = x.y; a[2] = x.z; a[3] = x.w;
}

// One thread per group of four parameters i = 4 q .. 4 q + 3; gradient element of parameter i: i + (i >= hole_begin ? hole_len : 0).
// PVEC: param, m, v and ema are all 16-byte aligned.  The gradient's alignment is looked at per group: it changes behind a hole
// whose length is no multiple of four.
template <bool PVEC>
__global__ __launch_bounds__(OPT_THREADS) void step_kernel(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ m, float* __restrict__ v,
                                                            float* __restrict__ ema, long long n, long long hole_begin, long long hole_len, Hyper h,
                                                            const float* __restrict__ scalars) {
    const long long i = ((long long)ttup_bid_x() * OPT_THREADS + ttup_tid_x()) * 4;
    if (i >= n) return;
    const float clip = scalars[1];
    if (i + 3 < n && (i + 3 < hole_begin || i >= hole_begin)) {
        const float* gp = grad + i + (i >= hole_begin ? hole_len : 0);
        const float4 g4 = ((size_t)gp & 15) == 0 ? load4<true>(gp) : load4<false>(gp);
        float4 p4 = load4<PVEC>(param + i), m4 = load4<PVEC>(m + i), v4 = load4<PVEC>(v + i), e4 = load4<PVEC>(ema + i);
        step_one(g4.x, clip, h, p4.x, m4.x, v4.x, e4.x);
        step_one(g4.y, clip, h, p4.y, m4.y, v4.y, e4.y);
        step_one(g4.z, clip, h, p4.z, m4.z, v4.z, e4.z);
        step_one(g4.w, clip, h, p4.w, m4.w, v4.w, e4.w);
        store4<PVEC>(param + i, p4); store4<PVEC>(m + i, m4); store4<PVEC>(v + i, v4); store4<PVEC>(ema + i, e4);
        return;
    }
    for (long long j = i; j < i + 4 && j < n; ++j) {
        float pj = param[j], mj = m[j], vj = v[j], ej = ema[j];
        step_one(grad[j + (j >= hole_begin ? hole_len : 0)], clip, h, pj, mj, vj, ej);
        param[j] = pj; m[j] = mj; v[j] = vj; ema[j] = ej;
    }
}

bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

size_t scratch_bytes() { return OPT_MAX_BLOCKS * sizeof(double) + 4 * sizeof(float); }

struct HyperD { double lr, beta1, beta2, eps, ema_decay, max_norm; };

int check_hyper(const char* who, const HyperD& h) {
    TTUP_REQUIRE(h.lr >= 0.0 && h.beta1 >= 0.0 && h.beta1 < 1.0 && h.beta2 >= 0.0 && h.beta2 < 1.0 && h.eps >= 0.0 && h.ema_decay >= 0.0 && h.ema_decay <= 1.0 &&
                     h.max_norm > 0.0,
                 TTUP_EINVAL, "%s: hyper-parameters outside torch.optim.Adam's ranges (lr %g, betas %g %g, eps %g, ema_decay %g, max_norm %g)", who, h.lr, h.beta1,
                 h.beta2, h.eps, h.ema_decay, h.max_norm);
    return TTUP_OK;
}

// torch.optim.Adam computes the bias corrections and the step size from the step count on the host in double (Python floats);
// every scalar reaches the fp32 kernels rounded to fp32 once
Hyper make_hyper(const HyperD& d, long long step) {
    const double bc1 = 1.0 - pow(d.beta1, (double)step), bc2 = 1.0 - pow(d.beta2, (double)step);
    Hyper h;
    h.w1 = (float)(1.0 - d.beta1); h.beta2 = (float)d.beta2; h.w2 = (float)(1.0 - d.beta2);
    h.bc2_sqrt = (float)pow(bc2, 0.5); h.eps = (float)d.eps; h.neg_step_size = (float)(-(d.lr / bc1));
    h.ema_a = (float)d.ema_decay; h.ema_b = (float)(1.0 - d.ema_decay); h.max_norm = (float)d.max_norm;
    return h;
}

int flat_step(float* param, const float* grad, float* m, float* v, float* ema, long long n, long long hole_begin, long long hole_len, const HyperD& hd, long long step,
              void* scratch, float* norm_out, hipStream_t st) {
    const Hyper h = make_hyper(hd, step);
    double* partial = (double*)scratch;
    float* scalars = (float*)(partial + OPT_MAX_BLOCKS);
    const long long ng = n + hole_len, ggroups = (ng + 3) / 4;
    long long blocks = (ggroups + OPT_THREADS - 1) / OPT_THREADS;
    if (blocks > OPT_MAX_BLOCKS) blocks = OPT_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    if (aligned16(grad)) hipLaunchKernelGGL(sqsum_kernel<true>, dim3((unsigned)blocks), dim3(OPT_THREADS), 0, st, grad, ng, partial);
    else hipLaunchKernelGGL(sqsum_kernel<false>, dim3((unsigned)blocks), dim3(OPT_THREADS), 0, st, grad, ng, partial);
    TTUP_LAUNCH_CHECK();
    hipLaunchKernelGGL(norm_kernel, dim3(1), dim3(OPT_THREADS), 0, st, (const double*)partial, (int)blocks, h.max_norm, scalars, norm_out);
    TTUP_LAUNCH_CHECK();
    if (n > 0) {
        const long long groups = (n + 3) / 4;
        const dim3 grid((unsigned)((groups + OPT_THREADS - 1) / OPT_THREADS));
        if (aligned16(param) && aligned16(m) && aligned16(v) && aligned16(ema))
            hipLaunchKernelGGL(step_kernel<true>, grid, dim3(OPT_THREADS), 0, st, param, grad, m, v, ema, n, hole_begin, hole_len, h, (const float*)scalars);
        else
            hipLaunchKernelGGL(step_kernel<false>, grid, dim3(OPT_THREADS), 0, st, param, grad, m, v, ema, n, hole_begin, hole_len, h, (const float*)scalars);
        TTUP_LAUNCH_CHECK();
    }
    return TTUP_OK;
}

}  // namespace

struct ttup_uplift_opt {
    ttup_uplift* net = nullptr;
    float *m = nullptr, *v = nullptr, *ema = nullptr;
    void* scratch = nullptr;
    long long n = 0, hole_begin = 0, hole_len = 0, step = 0;
    HyperD hyper = {};
    ~ttup_uplift_opt() {
        for (void* p : {(void*)m, (void*)v, (void*)ema, scratch}) if (p) (void)hipFree(p);
    }
};

extern "C" size_t ttup_opt_flat_scratch_bytes(void) { return scratch_bytes(); }

extern "C" int ttup_opt_flat_step(float* param_dev, const float* grad_dev, float* m_dev, float* v_dev, float* ema_dev, long long n, long long hole_begin,
                                  long long hole_len, double lr, double beta1, double beta2, double eps, double ema_decay, double max_norm, long long step,
                                  void* scratch_dev, float* norm_out_dev, void* stream) {
    TTUP_REQUIRE(param_dev && grad_dev && m_dev && v_dev && ema_dev && scratch_dev, TTUP_EINVAL, "ttup_opt_flat_step: null pointer");
    TTUP_REQUIRE(n >= 0 && n < (1LL << 40) && hole_len >= 0 && hole_len < (1LL << 40) && hole_begin >= 0 && hole_begin <= n, TTUP_EINVAL,
                 "ttup_opt_flat_step: n %lld, hole [%lld, +%lld) -- the hole must begin inside [0, n]", n, hole_begin, hole_len);
    TTUP_REQUIRE(step >= 1, TTUP_EINVAL, "ttup_opt_flat_step: the step count is 1-based, got %lld", step);
    TTUP_REQUIRE(((size_t)param_dev & 3) == 0 && ((size_t)grad_dev & 3) == 0 && ((size_t)m_dev & 3) == 0 && ((size_t)v_dev & 3) == 0 && ((size_t)ema_dev & 3) == 0 &&
                     ((size_t)scratch_dev & 7) == 0,
                 TTUP_EINVAL, "ttup_opt_flat_step: buffers must be 4-byte aligned, the scratch 8-byte aligned");
    const HyperD hd = {lr, beta1, beta2, eps, ema_decay, max_norm};
    if (int rc = check_hyper("ttup_opt_flat_step", hd)) return rc;
    return flat_step(param_dev, grad_dev, m_dev, v_dev, ema_dev, n, hole_begin, hole_len, hd, step, scratch_dev, norm_out_dev, (hipStream_t)stream);
}

extern "C" int ttup_uplift_opt_create(ttup_uplift* net, double lr, double beta1, double beta2, double eps, double ema_decay, double max_norm, ttup_uplift_opt** out) {
    TTUP_REQUIRE(net && out, TTUP_EINVAL, "ttup_uplift_opt_create: null pointer");
    TTUP_REQUIRE(trains(net), TTUP_EINVAL, "ttup_uplift_opt_create: the optimizer serves connectstage/dynamic handles only (the variant with gradients)");
    const HyperD hd = {lr, beta1, beta2, eps, ema_decay, max_norm};
    if (int rc = check_hyper("ttup_uplift_opt_create", hd)) return rc;
    const GradLayout lay = grad_layout(grad_dims(net));
    std::unique_ptr<ttup_uplift_opt> opt(new ttup_uplift_opt);
    opt->net = net; opt->hyper = hd; opt->n = net->plain_floats;
    opt->hole_begin = lay.hole_begin; opt->hole_len = lay.hole_len;          // embed.*, right after cls_token
    TTUP_REQUIRE(opt->hole_begin <= opt->n, TTUP_EINVAL, "ttup_uplift_opt_create: the handle's plain weights do not fit the layout");
    const size_t bytes = (size_t)opt->n * sizeof(float);
    TTUP_HIP_CHECK(hipMalloc((void**)&opt->m, bytes));
    TTUP_HIP_CHECK(hipMalloc((void**)&opt->v, bytes));
    TTUP_HIP_CHECK(hipMalloc((void**)&opt->ema, bytes));
    TTUP_HIP_CHECK(hipMalloc(&opt->scratch, scratch_bytes()));
    TTUP_HIP_CHECK(hipMemset(opt->m, 0, bytes));
    TTUP_HIP_CHECK(hipMemset(opt->v, 0, bytes));
    TTUP_HIP_CHECK(hipMemcpy(opt->ema, net->plain, bytes, hipMemcpyDeviceToDevice));      // update_ema(model, model_ema, 0): train.py:58
    TTUP_HIP_CHECK(hipDeviceSynchronize());
    *out = opt.release();
    return TTUP_OK;
}

extern "C" void ttup_uplift_opt_destroy(ttup_uplift_opt* opt) {
    if (!opt) return;
    (void)hipDeviceSynchronize();
    delete opt;
}

extern "C" int ttup_uplift_opt_step(ttup_uplift_opt* opt, const float* grad_flat_dev, float* norm_out_dev, void* stream) {
    TTUP_REQUIRE(opt && grad_flat_dev, TTUP_EINVAL, "ttup_uplift_opt_step: null pointer");
    TTUP_REQUIRE(((size_t)grad_flat_dev & 3) == 0, TTUP_EINVAL, "ttup_uplift_opt_step: the gradient buffer must be 4-byte aligned");
    opt->net->trained = true;
    if (int rc = flat_step(opt->net->plain, grad_flat_dev, opt->m, opt->v, opt->ema, opt->n, opt->hole_begin, opt->hole_len, opt->hyper, opt->step + 1, opt->scratch,
                           norm_out_dev, (hipStream_t)stream))
        return rc;
    opt->step += 1;
    return TTUP_OK;
}

namespace {
float* which_buffer(ttup_uplift_opt* opt, int which) {
    switch (which) {
        case TTUP_OPT_PARAM: return opt->net->plain;
        case TTUP_OPT_EMA: return opt->ema;
        case TTUP_OPT_M: return opt->m;
        case TTUP_OPT_V: return opt->v;
    }
    return nullptr;
}
}  // namespace

extern "C" int ttup_uplift_opt_read(ttup_uplift_opt* opt, int which, float* out_dev, void* stream) {
    TTUP_REQUIRE(opt && out_dev, TTUP_EINVAL, "ttup_uplift_opt_read: null pointer");
    const float* src = which_buffer(opt, which);
    TTUP_REQUIRE(src, TTUP_EINVAL, "ttup_uplift_opt_read: unknown buffer %d", which);
    hipStream_t st = (hipStream_t)stream;
    const long long hb = opt->hole_begin, hl = opt->hole_len;
    TTUP_HIP_CHECK(hipMemcpyAsync(out_dev, src, (size_t)hb * sizeof(float), hipMemcpyDeviceToDevice, st));
    TTUP_HIP_CHECK(hipMemsetAsync(out_dev + hb, 0, (size_t)hl * sizeof(float), st));
    TTUP_HIP_CHECK(hipMemcpyAsync(out_dev + hb + hl, src + hb, (size_t)(opt->n - hb) * sizeof(float), hipMemcpyDeviceToDevice, st));
    return TTUP_OK;
}

extern "C" int ttup_uplift_opt_load(ttup_uplift_opt* opt, int which, const float* in_dev, void* stream) {
    TTUP_REQUIRE(opt && in_dev, TTUP_EINVAL, "ttup_uplift_opt_load: null pointer");
    float* dst = which_buffer(opt, which);
    TTUP_REQUIRE(dst, TTUP_EINVAL, "ttup_uplift_opt_load: unknown buffer %d", which);
    hipStream_t st = (hipStream_t)stream;
    const long long hb = opt->hole_begin, hl = opt->hole_len;
    if (which == TTUP_OPT_PARAM) opt->net->trained = true;          // the packed weight images no longer match `plain`
    TTUP_HIP_CHECK(hipMemcpyAsync(dst, in_dev, (size_t)hb * sizeof(float), hipMemcpyDeviceToDevice, st));
    TTUP_HIP_CHECK(hipMemcpyAsync(dst + hb, in_dev + hb + hl, (size_t)(opt->n - hb) * sizeof(float), hipMemcpyDeviceToDevice, st));
    return TTUP_OK;
}

extern "C" int ttup_uplift_opt_set_step(ttup_uplift_opt* opt, long long step) {
    TTUP_REQUIRE(opt && step >= 0, TTUP_EINVAL, "ttup_uplift_opt_set_step: null handle or negative step count");
    opt->step = step;
    return TTUP_OK;
}

extern "C" int ttup_uplift_opt_get_step(ttup_uplift_opt* opt, long long* step_host) {
    TTUP_REQUIRE(opt && step_host, TTUP_EINVAL, "ttup_uplift_opt_get_step: null pointer");
    *step_host = opt->step;
    return TTUP_OK;
}

#include "no_packed_fp32_end.h"
