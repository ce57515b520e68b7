// The uplift model's evaluation metrics on the device (include/ttup.h): the per-batch arithmetic of the reference's val()
// (uplifting/train.py:166-195) and val_real() (:250-283) over a whole prediction set in one pass each.
//
// Inputs are the fp32 tensors the forward produces or consumes; every per-sample operation and every sum is fp64.
//
// Mapping: EV_LANES = 16 lanes per sample, EV_SAMPLES = 16 samples per 256-thread block.  Lane l of a sample takes the time steps
// l, l + 16, ...: the 16 lanes of a sample read 16 consecutive (x, y, z) triples, and the four samples of a wave are neighbours in
// memory, so a wave's loads cover one contiguous stretch of each (N,T,3) tensor (a lane per sample would stride by T * 12 bytes).
// The once-per-sample spin arithmetic is done by lane 0 of the sample.
//
// Sums: a fixed tree that depends on N and T alone, no floating-point atomics, so two calls return the same bits --
//   per lane over its time steps in order -> xor butterfly over the sample's 16 lanes -> the block's 16 samples in order
//   (one partial per block and quantity, in the workspace) -> eval_final_kernel: one block per quantity, thread i adds the
//   partials i, i + 256, ... in order, then a 256-leaf tree in LDS.  The butterfly, the partials and the final kernel are
//   csrc/eval_reduce.h's, shared with csrc/detect_eval.hip.
//
// Where this differs from the reference, on purpose:
//   * a time step with mask == 0 is selected out, not multiplied by 0: a non-finite value in a masked slot is inert (val_real's
//     metric_pos2D_fn already does this; val's metric_pos_fn would return NaN);
//   * the cosine is clamped to [-1, 1] before acos (the reference returns NaN when fp32 rounding pushes it past 1); a NaN cosine
//     stays NaN;
//   * a sample whose first two positions coincide in x and y has the NaN local frame of the reference (0 / 0): components 0 and 1
//     of its local spin are NaN and component 2 is not, exactly as helper.py:411-418 leaves them.
#include "no_packed_fp32_begin.h"
#include "common.h"
#include "eval_reduce.h"

#include <math.h>

#pragma clang fp contract(off)

using namespace ttup;

namespace {

constexpr int EV_THREADS = ER_THREADS;                       // threads per block of all three kernels
constexpr int EV_LANES = 16;                             // lanes per sample
constexpr int EV_SAMPLES = EV_THREADS / EV_LANES;        // samples per block
constexpr int VAL_SUMS = 8, VAL_COUNTS = 12;             // ttup_uplift_val_metrics: sums_dev / counts_dev (without N)
constexpr int REAL_SUMS = 1, REAL_COUNTS = 4;            // ttup_uplift_val_real_metrics
constexpr double IMG_WIDTH = 2560.0, IMG_HEIGHT = 1440.0;          // uplifting/helper.py:26
constexpr int TOPSPIN_CLASS = 1, BACKSPIN_CLASS = 2;     // uplifting/data.py

__device__ __forceinline__ double group_sum(double v) { return lanes_sum<EV_LANES>(v); }          // over a sample's lanes

// transform_rotationaxes (uplifting/helper.py:394-420) in fp64: e_x = (ex, ey, 0), e_y = e_z x e_x = (-ey, ex, 0), e_z = (0, 0, 1)
__device__ __forceinline__ void local_spin(const float* __restrict__ rot, const float* __restrict__ pos, double w[3]) {
    const double vx = (double)pos[3] - (double)pos[0], vy = (double)pos[4] - (double)pos[1];
    const double nrm = sqrt(vx * vx + vy * vy);
    const double ex = vx / nrm, ey = vy / nrm;
    const double r0 = rot[0], r1 = rot[1], r2 = rot[2];
    w[0] = r0 * ex + r1 * ey;
    w[1] = r1 * ex - r0 * ey;
    w[2] = r2;
}

// sums (per block): 0 ||d||  1 |dx|  2 |dy|  3 |dz|  4 | ||pred|| - ||gt|| |  5 angle [deg]  6 masked mean position error  7 ||d||^2
// counts: TP[3] TN[3] FP[3] FN[3] of helper.binary_metrics(rot_gt = PREDICTION, rot_pred = TARGET) -- the order train.py:181 calls it in
__global__ __launch_bounds__(EV_THREADS) void val_kernel(const float* __restrict__ pred_rot, const float* __restrict__ pred_pos, const float* __restrict__ r_world,
                                                          const float* __restrict__ rotation, const float* __restrict__ mask, long long n, int T, int global,
                                                          long long nblocks, double* __restrict__ psum, int* __restrict__ pcnt) {
    __shared__ double sm[VAL_SUMS][EV_SAMPLES];
    __shared__ int sc[VAL_COUNTS][EV_SAMPLES];
    const int tid = ttup_tid_x(), g = tid / EV_LANES, sub = tid % EV_LANES;
    const long long b = (long long)ttup_bid_x() * EV_SAMPLES + g;
    const bool valid = b < n;
    double acc = 0.0, msum = 0.0;
    if (valid) {
        const float* pp = pred_pos + (size_t)b * T * 3;
        const float* pw = r_world + (size_t)b * T * 3;
        const float* pm = mask + (size_t)b * T;
        for (int t = sub; t < T; t += EV_LANES) {
            const double m = pm[t];
            const double dx = (double)pp[t * 3] - (double)pw[t * 3], dy = (double)pp[t * 3 + 1] - (double)pw[t * 3 + 1], dz = (double)pp[t * 3 + 2] - (double)pw[t * 3 + 2];
            const double d = sqrt(dx * dx + dy * dy + dz * dz);
            if (m != 0.0) {
                acc = acc + d * m;
                msum = msum + m;
            }
        }
    }
    acc = group_sum(acc);
    msum = group_sum(msum);
    if (sub == 0) {
        double s[VAL_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int c[VAL_COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (valid) {
            const float* pw = r_world + (size_t)b * T * 3;
            double gt[3], pr[3];
            local_spin(rotation + b * 3, pw, gt);
            if (global) local_spin(pred_rot + b * 3, pw, pr);
            else { pr[0] = pred_rot[b * 3]; pr[1] = pred_rot[b * 3 + 1]; pr[2] = pred_rot[b * 3 + 2]; }
            const double d0 = pr[0] - gt[0], d1 = pr[1] - gt[1], d2 = pr[2] - gt[2];
            const double sq = d0 * d0 + d1 * d1 + d2 * d2;
            const double np_ = sqrt(pr[0] * pr[0] + pr[1] * pr[1] + pr[2] * pr[2]), ng = sqrt(gt[0] * gt[0] + gt[1] * gt[1] + gt[2] * gt[2]);
            double cosv = (pr[0] * gt[0] + pr[1] * gt[1] + pr[2] * gt[2]) / (np_ * ng);
            cosv = cosv > 1.0 ? 1.0 : (cosv < -1.0 ? -1.0 : cosv);          // a NaN passes through both comparisons
            s[0] = sqrt(sq);
            s[1] = __builtin_fabs(d0); s[2] = __builtin_fabs(d1); s[3] = __builtin_fabs(d2);
            s[4] = __builtin_fabs(np_ - ng);
            s[5] = acos(cosv) * (180.0 / 3.14159265358979323846);
            s[6] = acc / msum;
            s[7] = sq;
            for (int k = 0; k < 3; ++k) {                                   // sign(NaN) and sign(0) match neither +1 nor -1
                const bool pp_ = pr[k] > 0.0, pn = pr[k] < 0.0, gp = gt[k] > 0.0, gn = gt[k] < 0.0;
                c[k] = pp_ && gp;            // TP: rot_gt == 1 and rot_pred == 1
                c[3 + k] = pn && gn;         // TN: both -1
                c[6 + k] = pn && gp;         // "FP": rot_gt == -1 (the prediction) and rot_pred == 1 (the target)
                c[9 + k] = pp_ && gn;        // "FN": rot_gt == 1 (the prediction) and rot_pred == -1 (the target)
            }
        }
        for (int k = 0; k < VAL_SUMS; ++k) sm[k][g] = s[k];
        for (int k = 0; k < VAL_COUNTS; ++k) sc[k][g] = c[k];
    }
    __syncthreads();
    store_block_partials(sm, sc, VAL_COUNTS, nblocks, psum, pcnt);          // the block's samples in order
}

// sums: 0 masked mean of the 2-D distance [px].  counts: TP TN FP FN (train.py:265-276).  scores[b]: local spin component 1;
// labels[b]: 1 topspin, 0 backspin, -1 not annotated.
__global__ __launch_bounds__(EV_THREADS) void val_real_kernel(const float* __restrict__ pred_rot, const float* __restrict__ pred_pos, const float* __restrict__ r_img,
                                                               const float* __restrict__ mask, const float* __restrict__ Mint, const float* __restrict__ Mext,
                                                               const int* __restrict__ spin_class, long long n, int T, int global, long long nblocks,
                                                               double* __restrict__ psum, int* __restrict__ pcnt, double* __restrict__ scores, int* __restrict__ labels) {
    __shared__ double sm[REAL_SUMS][EV_SAMPLES];
    __shared__ int sc[REAL_COUNTS][EV_SAMPLES];
    const int tid = ttup_tid_x(), g = tid / EV_LANES, sub = tid % EV_LANES;
    const long long b = (long long)ttup_bid_x() * EV_SAMPLES + g;
    const bool valid = b < n;
    double acc = 0.0, msum = 0.0;
    if (valid) {
        const float* pp = pred_pos + (size_t)b * T * 3;
        const float* pi = r_img + (size_t)b * T * 2;
        const float* pm = mask + (size_t)b * T;
        double E[16], K[9];
        for (int k = 0; k < 16; ++k) E[k] = Mext[b * 16 + k];
        for (int k = 0; k < 9; ++k) K[k] = Mint[b * 9 + k];
        for (int t = sub; t < T; t += EV_LANES) {
            const double m = pm[t];
            const double x = pp[t * 3], y = pp[t * 3 + 1], z = pp[t * 3 + 2];
            double h[4];                                                    // world2cam (helper.py:190-195): Mext (x, y, z, 1), then / h[3]
            for (int i = 0; i < 4; ++i) h[i] = E[i * 4] * x + E[i * 4 + 1] * y + E[i * 4 + 2] * z + E[i * 4 + 3];
            const double cx = h[0] / h[3], cy = h[1] / h[3], cz = h[2] / h[3];
            double q[3];                                                    // cam2img (helper.py:154-157): Mint cam, then / q[2]
            for (int i = 0; i < 3; ++i) q[i] = K[i * 3] * cx + K[i * 3 + 1] * cy + K[i * 3 + 2] * cz;
            const double du = q[0] / q[2] - (double)pi[t * 2] * IMG_WIDTH, dv = q[1] / q[2] - (double)pi[t * 2 + 1] * IMG_HEIGHT;
            const double d = sqrt(du * du + dv * dv);
            if (m != 0.0) {
                acc = acc + d * m;
                msum = msum + m;
            }
        }
    }
    acc = group_sum(acc);
    msum = group_sum(msum);
    if (sub == 0) {
        double s = 0.0;
        int c[REAL_COUNTS] = {0, 0, 0, 0};
        if (valid) {
            double score;
            if (global) {
                double w[3];
                local_spin(pred_rot + b * 3, pred_pos + (size_t)b * T * 3, w);          // the PREDICTED positions (train.py:253)
                score = w[1];
            } else {
                score = pred_rot[b * 3 + 1];
            }
            const int cls = spin_class[b];
            if (cls == TOPSPIN_CLASS) {
                if (score > 0.0) c[0] = 1; else c[3] = 1;
            } else if (cls == BACKSPIN_CLASS) {
                if (score < 0.0) c[1] = 1; else c[2] = 1;
            }
            s = acc / msum;
            scores[b] = score;
            labels[b] = cls == TOPSPIN_CLASS ? 1 : (cls == BACKSPIN_CLASS ? 0 : -1);
        }
        sm[0][g] = s;
        for (int k = 0; k < REAL_COUNTS; ++k) sc[k][g] = c[k];
    }
    __syncthreads();
    store_block_partials(sm, sc, REAL_COUNTS, nblocks, psum, pcnt);
}

long long eval_blocks(long long n) { return (n + EV_SAMPLES - 1) / EV_SAMPLES; }

// per block: VAL_SUMS doubles, then (behind all doubles) VAL_COUNTS ints -- val_real needs less and shares the query
size_t eval_workspace_bytes(long long n) { return n > 0 ? (size_t)eval_blocks(n) * (VAL_SUMS * sizeof(double) + VAL_COUNTS * sizeof(int)) : 0; }

int check_common(const char* who, int n, int t, const void* ws, size_t ws_bytes) {
    TTUP_REQUIRE(n > 0, TTUP_EINVAL, "%s: need at least one sample, got n = %d", who, n);
    TTUP_REQUIRE(t >= 2, TTUP_EINVAL, "%s: need at least two time steps (the local frame is built from steps 0 and 1), got t = %d", who, t);
    TTUP_REQUIRE(((size_t)ws & 7) == 0, TTUP_EINVAL, "%s: the workspace must be 8-byte aligned", who);
    TTUP_REQUIRE(ws_bytes >= eval_workspace_bytes(n), TTUP_EINVAL, "%s: workspace of %zu bytes, need %zu (ttup_uplift_eval_workspace_bytes)", who, ws_bytes,
                 eval_workspace_bytes(n));
    return TTUP_OK;
}

}  // namespace

extern "C" size_t ttup_uplift_eval_workspace_bytes(int n) { return eval_workspace_bytes(n); }

extern "C" int ttup_uplift_val_metrics(const float* pred_rot_dev, const float* pred_pos_dev, const float* r_world_dev, const float* rotation_dev, const float* mask_dev,
                                       int n, int t, int transform_global, void* workspace_dev, size_t workspace_bytes, double* sums_dev, long long* counts_dev,
                                       void* stream) {
    TTUP_REQUIRE(pred_rot_dev && pred_pos_dev && r_world_dev && rotation_dev && mask_dev && workspace_dev && sums_dev && counts_dev, TTUP_EINVAL,
                 "ttup_uplift_val_metrics: null pointer");
    if (int rc = check_common("ttup_uplift_val_metrics", n, t, workspace_dev, workspace_bytes)) return rc;
    const long long nb = eval_blocks(n);
    const EvalPartials p = eval_partials(workspace_dev, nb, VAL_SUMS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(val_kernel, dim3((unsigned)nb), dim3(EV_THREADS), 0, st, pred_rot_dev, pred_pos_dev, r_world_dev, rotation_dev, mask_dev, (long long)n, t,
                       transform_global ? 1 : 0, nb, p.psum, p.pcnt);
    TTUP_LAUNCH_CHECK();
    return eval_finish(p, nb, VAL_SUMS, VAL_COUNTS, n, sums_dev, counts_dev, st);
}

extern "C" int ttup_uplift_val_real_metrics(const float* pred_rot_dev, const float* pred_pos_dev, const float* r_img_dev, const float* mask_dev, const float* mint_dev,
                                            const float* mext_dev, const int* spin_class_dev, int n, int t, int transform_global, void* workspace_dev,
                                            size_t workspace_bytes, double* sums_dev, long long* counts_dev, double* scores_dev, int* labels_dev, void* stream) {
    TTUP_REQUIRE(pred_rot_dev && pred_pos_dev && r_img_dev && mask_dev && mint_dev && mext_dev && spin_class_dev && workspace_dev && sums_dev && counts_dev &&
                     scores_dev && labels_dev,
                 TTUP_EINVAL, "ttup_uplift_val_real_metrics: null pointer");
    if (int rc = check_common("ttup_uplift_val_real_metrics", n, t, workspace_dev, workspace_bytes)) return rc;
    const long long nb = eval_blocks(n);
    const EvalPartials p = eval_partials(workspace_dev, nb, REAL_SUMS);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(val_real_kernel, dim3((unsigned)nb), dim3(EV_THREADS), 0, st, pred_rot_dev, pred_pos_dev, r_img_dev, mask_dev, mint_dev, mext_dev, spin_class_dev,
                       (long long)n, t, transform_global ? 1 : 0, nb, p.psum, p.pcnt, scores_dev, labels_dev);
    TTUP_LAUNCH_CHECK();
    return eval_finish(p, nb, REAL_SUMS, REAL_COUNTS, n, sums_dev, counts_dev, st);
}

#include "no_packed_fp32_end.h"
