// The detectors' evaluation on the device (include/ttup.h): the heatmap loss of the reference's ball and table val()
// (balldetection/train.py:177-179, tabledetection/train.py:154-156) and of both train() loops (:112-113, :106-107), and the
// position metrics its val() and inference scripts report (PCK at fixed pixel tolerances, average distance, distance to the
// motion-blur streak, ratio of detected keypoints).
//
// Inputs are fp32 (heatmaps, positions) and fp64 (target centres); every operation and every sum is fp64.
//
// Heatmap loss.  The reference upsamples the predicted heatmap bilinearly to the evaluation resolution and compares it there with a
// Gaussian target of that size: two full-resolution tensors per batch.  loss_kernel writes neither.  One workgroup takes a strip of
// `strip` output rows of one (sample, channel) map: it copies the source rows the strip interpolates between into LDS (fp32, as
// they are), then thread t walks the output columns t, t + 256, ... and, per column, the strip's rows.  The target is separable,
// exp(-dx^2 / 2s^2) * exp(-dy^2 / 2s^2): factor_kernel evaluates the out_h + out_w factors of a map once, in fp64, and the
// product is rounded once to fp32 as the reference's torch.tensor(heatmap, dtype=float32) rounds its exp.
//
// LDS: which source rows a strip keeps, and in which slot, is decided without a device in csrc/detect_loss_plan.h (the coordinate
// itself is csrc/detect_grad_plan.h's dg_src_coord): the kernel's fill loop and its reads call those functions, and loss_plan()
// walks the strips with them and picks the largest strip height <= DE_STRIP whose slots fit DE_ROW_BYTES
// (tests/test_detect_loss_plan_host.py holds the three together on the CPU), so a workgroup never needs more than 60 KB and
// 2 .. 30 workgroups share a CU's 160 KB: WASB (704, 1280) ->
// 8 rows x 5 KB = 40 KB, 4 workgroups (16 waves) per CU; ViTPose (160, 288) -> 4 rows x 1.1 KB.  Within a wave the 64 lanes read
// 64 neighbouring output columns: when upsampling these are <= 64 consecutive floats of one LDS row (no bank is hit by two
// different addresses), lanes that share a source column are served by the broadcast.
//
// Sums: thread (columns in order, rows in order) -> xor butterfly over the wave -> the block's 4 waves in order (one partial per
// strip, in the workspace) -> final kernel: one block per map, thread i adds the partials i, i + 256, ... in order, then a
// 256-leaf tree in LDS.  No floating-point atomics: two calls return the same bits.  The metric kernels use the same tree; it is
// written once, in csrc/eval_reduce.h.
//
// The gradient of that loss into the predicted heatmaps (ttup_detect_heatmap_loss_grad) is grad_kernel, described where it stands;
// what it decides without a device is csrc/detect_grad_plan.h.
#include "no_packed_fp32_begin.h"
#include "common.h"
#include "detect_grad_plan.h"
#include "detect_loss_plan.h"
#include "eval_reduce.h"

#include <math.h>

#pragma clang fp contract(off)

using namespace ttup;

namespace {

constexpr int DE_THREADS = ER_THREADS;
constexpr int DE_WAVES = DE_THREADS / 64;
constexpr int DE_MAX_TOL = TTUP_DETECT_MAX_TOLERANCES;
constexpr int DE_SUMS = 2;                               // metric kernels: sums per call
constexpr int DE_COUNTS = 3 + DE_MAX_TOL;                // ... counts per call, at most
constexpr float VISIBLE = 1.0f;                          // BALL_VISIBLE / KEYPOINT_VISIBLE
constexpr double NOT_DETECTED = -100.0;                  // helper_balldetection.py:262: a detection is valid when x, y > -100

struct Tolerances {
    double v[DE_MAX_TOL];
    int n;
};

// fac (maps, out_h + out_w): the row factors exp(-(y - cy)^2 / 2 sigma^2), then the column factors; zeros for a map without target
__global__ __launch_bounds__(DE_THREADS) void factor_kernel(const double* __restrict__ centres, const int* __restrict__ has_target, int out_h, int out_w, int blocks_per_map,
                                                             double two_sigma2, double* __restrict__ fac) {
    const int map = ttup_bid_x() / blocks_per_map;
    const int j = (ttup_bid_x() % blocks_per_map) * DE_THREADS + ttup_tid_x();
    if (j >= out_h + out_w) return;
    double f = 0.0;
    if (has_target[map] != 0) {
        const double c = j < out_h ? centres[(size_t)map * 2 + 1] : centres[(size_t)map * 2];
        const double d = (double)(j < out_h ? j : j - out_h) - c;
        f = exp(-(d * d) / two_sigma2);
    }
    fac[(size_t)map * (out_h + out_w) + j] = f;
}

__global__ __launch_bounds__(DE_THREADS) void loss_kernel(const float* __restrict__ pred, const double* __restrict__ fac, int h, int w, int out_h, int out_w,
                                                           double scale_y, double scale_x, int strip, int nstrips, int weighted, double* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float rows[];          // [slots][w]
    __shared__ double s_ly[DE_STRIP], s_gy[DE_STRIP], s_red[DE_WAVES];
    __shared__ int s_a[DE_STRIP], s_b[DE_STRIP];
    const int tid = ttup_tid_x();
    const int map = ttup_bid_x() / nstrips, r0 = (ttup_bid_x() % nstrips) * strip;
    const int nr = out_h - r0 < strip ? out_h - r0 : strip;
    const LossStrip ls = dl_strip(r0, nr, scale_y, h);
    const double* f = fac + (size_t)map * (out_h + out_w);
    if (tid < nr) {
        int i0, i1;
        double lam;
        dg_src_coord(r0 + tid, scale_y, h, i0, i1, lam);
        s_ly[tid] = lam;
        s_a[tid] = dl_slot(ls, tid, 0, i0);
        s_b[tid] = dl_slot(ls, tid, 1, i1);
        s_gy[tid] = f[r0 + tid];
    }
    const float* src = pred + (size_t)map * h * w;
    for (int s = 0; s < ls.slots; ++s) {
        const float* g = src + (size_t)dl_slot_row(ls, r0, s, scale_y, h) * w;
        float* l = rows + (size_t)s * w;
        for (int x = tid; x < w; x += DE_THREADS) l[x] = g[x];
    }
    __syncthreads();
    const double* gxp = f + out_h;
    double acc = 0.0;
    for (int c = tid; c < out_w; c += DE_THREADS) {
        int x0, x1;
        double lx;
        dg_src_coord(c, scale_x, w, x0, x1, lx);
        const double wx0 = 1.0 - lx, gx = gxp[c];
        for (int i = 0; i < nr; ++i) {
            const float* ra = rows + (size_t)s_a[i] * w;
            const float* rb = rows + (size_t)s_b[i] * w;
            const double ly = s_ly[i];
            const double top = wx0 * (double)ra[x0] + lx * (double)ra[x1];
            const double bot = wx0 * (double)rb[x0] + lx * (double)rb[x1];
            const double v = (1.0 - ly) * top + ly * bot;
            const float t = (float)(gx * s_gy[i]);
            const double d = v - (double)t;
            double q = d * d;
            if (weighted && t > 0.1f) q = 100.0 * q;
            acc = acc + q;
        }
    }
    acc = lanes_sum<64>(acc);
    if ((tid & 63) == 0) s_red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < DE_WAVES; ++k) s = s + s_red[k];
        partial[ttup_bid_x()] = s;
    }
}

// one block per map: its strips' partials in fixed order
__global__ __launch_bounds__(DE_THREADS) void loss_final_kernel(const double* __restrict__ partial, int nstrips, double* __restrict__ sums) {
    __shared__ double sd[DE_THREADS];
    const double s = block_tree_sum(partial + (size_t)ttup_bid_x() * nstrips, nstrips, sd);
    if (ttup_tid_x() == 0) sums[ttup_bid_x()] = s;
}

// ---- the gradient of the heatmap loss into pred: grad = scale * sum_y sum_x 2 w (up - t) a_y(i) b_x(j)
//
// Gather.  One workgroup takes `strip` source rows r0 .. and one group of source columns of one map (detect_grad_plan.h), copies
// them with one neighbour row above and below and one neighbour column left and right into LDS, and walks the output rows that read
// those rows, in order: the rows whose upper source row y0 is r0 - 1 .. r0 + nr - 1.  A lane serves one source column j: per
// output row it interpolates the column pair (j, j + 1) vertically once, walks the output columns x whose left source column is j
// -- [dg_first(j), dg_first(j + 1)): x0 is j by the plan, never recomputed -- forms r = 2 w (up - t) and adds b_x(j) r to cA,
// b_x(j + 1) r to cB.  cA belongs to column j, cB to column j + 1; both go, times a_y(y0) and a_y(y0 + 1), to the accumulators of the
// rows y0 and y0 + 1.  Only those two rows are open at a time: when y0 moves on, row y0 is complete; column j's value is its own A
// plus the B of the lane before (one shuffle), scaled, rounded once and stored; the accumulators shift.  Lane 0 of a wave serves
// the last column of the wave before, for its B alone, so a wave never needs another wave's registers: after the LDS copy there
// is no barrier, nothing of the output resolution is written anywhere, no two lanes add to the same value and the order of every
// sum is fixed.  A row or column nothing reads keeps accumulators of 0 and is stored as +0.0 whatever scale's sign.
__global__ __launch_bounds__(DG_MAX_WAVES * 64) void grad_kernel(const float* __restrict__ pred, const double* __restrict__ fac, int h, int w, int out_h, int out_w,
                                                                  double scale_y, double scale_x, int strip, int nstrips, int waves, int groups, int weighted, double scale,
                                                                  float* __restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) float g_rows[];          // [strip + 2][cw]
    const int tid = ttup_tid_x(), wave = tid >> 6, lane = tid & 63;
    const int group = ttup_bid_x() % groups, sid = ttup_bid_x() / groups;
    const int map = sid / nstrips, r0 = (sid % nstrips) * strip;
    const int nr = h - r0 < strip ? h - r0 : strip;
    int rb, re, cb, ce;
    dg_strip_rows(r0, strip, h, rb, re);
    dg_group_columns(group, waves, w, cb, ce);
    const int cw = ce - cb;
    const float* src = pred + (size_t)map * h * w;
    for (int r = rb; r < re; ++r) {
        const float* g = src + (size_t)r * w + cb;
        float* l = g_rows + (size_t)(r - rb) * cw;
        for (int x = tid; x < cw; x += waves * 64) l[x] = g[x];
    }
    // this lane's column and the output columns whose left source column it is: [f1, f2), empty for no column
    const int j = dg_column(group, waves, wave, lane), j1 = j < w - 1 ? j + 1 : j;
    const bool served = j >= 0 && j < w;
    const int f1 = served ? dg_first(j, scale_x, w, out_w) : 0, f2 = served ? dg_first(j + 1, scale_x, w, out_w) : 0;
    const double* fy = fac + (size_t)map * (out_h + out_w);
    const double* fx = fy + out_h;
    float* gmap = grad + (size_t)map * h * w;
    const int ybeg = dg_first(r0 - 1, scale_y, h, out_h), yend = dg_first(r0 + nr, scale_y, h, out_h);
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;          // a0 / b0 belong to the source row cur, a1 / b1 to cur + 1
    int cur = r0 - 1;
    __syncthreads();
    for (int y = ybeg; y <= yend; ++y) {
        int y0 = r0 + nr, y1 = y0;          // (y == yend: past the strip, the rows still open are flushed)
        double ly = 0.0, wy0 = 0.0, wy1 = 0.0;
        if (y < yend) dg_weights(y, scale_y, h, y0, y1, ly, wy0, wy1);
        for (; cur < y0; ++cur) {
            const double tot = a0 + __shfl_up(b0, 1, 64);
            if (cur >= r0 && lane >= 1 && served) gmap[(size_t)cur * w + j] = tot == 0.0 ? 0.0f : (float)(scale * tot);
            a0 = a1;
            b0 = b1;
            a1 = b1 = 0.0;
        }
        if (y < yend && f2 > f1) {
            const float* ra = g_rows + (size_t)(y0 - rb) * cw;
            const float* rc = g_rows + (size_t)(y1 - rb) * cw;
            const double gy = fy[y], uy = 1.0 - ly;
            const double vl = uy * (double)ra[j - cb] + ly * (double)rc[j - cb];
            const double vr = uy * (double)ra[j1 - cb] + ly * (double)rc[j1 - cb];
            double ca = 0.0, cr = 0.0;
            for (int x = f1; x < f2; ++x) {
                const double lx = dg_lambda(x, scale_x, j), ux = 1.0 - lx;          // dg_src_coord's lambda: its i0 is j by the ranges
                const double v = ux * vl + lx * vr;
                const float t = (float)(fx[x] * gy);
                double r = 2.0 * (v - (double)t);
                if (weighted && t > 0.1f) r = 100.0 * r;
                ca = ca + (j1 == j ? ux + lx : ux) * r;          // dg_weights' pair
                cr = cr + (j1 == j ? 0.0 : lx) * r;
            }
            a0 = a0 + wy0 * ca;
            a1 = a1 + wy1 * ca;
            b0 = b0 + wy0 * cr;
            b1 = b1 + wy1 * cr;
        }
    }
}

// _batched_distance_point_to_segment (helper_balldetection.py:335-399): t = 0 on a segment with L^2 <= 1e-12, clamped to [0, 1]
__device__ __forceinline__ double segment_distance(double px, double py, double ax, double ay, double bx, double by) {
    const double sx = bx - ax, sy = by - ay;
    const double l2 = sx * sx + sy * sy;
    const double dot = (px - ax) * sx + (py - ay) * sy;
    double t = 0.0;
    if (l2 > 1e-12) t = dot / l2;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double ex = px - (ax + t * sx), ey = py - (ay + t * sy);
    return sqrt(ex * ex + ey * ey);
}

__device__ __forceinline__ double nan_min(double a, double b) { return (a <= b || a != a) ? a : b; }          // np.minimum: a NaN wins

// a thread's sums and counts -> one partial per block and quantity: wave butterfly, then the block's waves in order
__device__ __forceinline__ void block_partials(const double (&s)[DE_SUMS], const int (&c)[DE_COUNTS], int ncounts, long long nblocks, double* __restrict__ psum,
                                               int* __restrict__ pcnt) {
    __shared__ double sm[DE_SUMS][DE_WAVES];
    __shared__ int sc[DE_COUNTS][DE_WAVES];
    const int tid = ttup_tid_x(), wave = tid >> 6;
    for (int k = 0; k < DE_SUMS; ++k) {
        const double v = lanes_sum<64>(s[k]);
        if ((tid & 63) == 0) sm[k][wave] = v;
    }
    for (int k = 0; k < DE_COUNTS; ++k) {
        const int v = lanes_sum<64>(c[k]);
        if ((tid & 63) == 0) sc[k][wave] = v;
    }
    __syncthreads();
    store_block_partials(sm, sc, ncounts, nblocks, psum, pcnt);
}

// sums: 0 distance to gt  1 distance to the streak as val() measures it, both over the visible samples with a detection (x, y > -100)
// counts: 0 visible (vis == 1)  1 of those, prediction flagged visible (pred[2] == 1: PCK's denominator)  2 of those, detected
//         3 + k: within tolerance k of the streak and flagged visible
__global__ __launch_bounds__(DE_THREADS) void ball_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ gt_min,
                                                                   const float* __restrict__ gt_max, const int* __restrict__ vis, long long n, Tolerances tol,
                                                                   long long nblocks, double* __restrict__ psum, int* __restrict__ pcnt) {
    const long long i = (long long)ttup_bid_x() * DE_THREADS + ttup_tid_x();
    double s[DE_SUMS] = {0.0, 0.0};
    int c[DE_COUNTS];
    for (int k = 0; k < DE_COUNTS; ++k) c[k] = 0;
    if (i < n && vis[i] == 1) {
        const double px = pred[i * 3], py = pred[i * 3 + 1];
        const double gx = gt[i * 2], gy = gt[i * 2 + 1], ax = gt_min[i * 2], ay = gt_min[i * 2 + 1], bx = gt_max[i * 2], by = gt_max[i * 2 + 1];
        const bool flagged = pred[i * 3 + 2] == VISIBLE, detected = px > NOT_DETECTED && py > NOT_DETECTED;
        c[0] = 1;
        c[1] = flagged;
        c[2] = detected;
        // calculate_pck_fixed_tolerance (:228-230): the segments gt_min -> gt and gt -> gt_max
        const double dp = nan_min(segment_distance(px, py, ax, ay, gx, gy), segment_distance(px, py, gx, gy, bx, by));
        for (int k = 0; k < tol.n; ++k) c[3 + k] = flagged && dp <= tol.v[k];
        if (detected) {
            const double dx = px - gx, dy = py - gy;
            s[0] = sqrt(dx * dx + dy * dy);
            // train.py:220 calls distance_to_streak(pred, gt, gt_min, gt_max) against the signature (pred, r_min, r_b, r_max): the
            // segments it measures are gt -> gt_min and gt_min -> gt_max
            s[1] = nan_min(segment_distance(px, py, gx, gy, ax, ay), segment_distance(px, py, ax, ay, bx, by));
        }
    }
    block_partials(s, c, 3 + tol.n, nblocks, psum, pcnt);
}

// one thread per keypoint.  sums: 0 distance over valid & visible (1 unused).  counts: 0 valid (pred[2] == 1)  1 valid & visible
// (gt[2] == 1)  2 unused  3 + k: of those, within tolerance k
__global__ __launch_bounds__(DE_THREADS) void table_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt, long long n, Tolerances tol,
                                                                    long long nblocks, double* __restrict__ psum, int* __restrict__ pcnt) {
    const long long i = (long long)ttup_bid_x() * DE_THREADS + ttup_tid_x();
    double s[DE_SUMS] = {0.0, 0.0};
    int c[DE_COUNTS];
    for (int k = 0; k < DE_COUNTS; ++k) c[k] = 0;
    if (i < n) {
        const bool valid = pred[i * 3 + 2] == VISIBLE, both = valid && gt[i * 3 + 2] == VISIBLE;
        c[0] = valid;
        c[1] = both;
        if (both) {
            const double dx = (double)pred[i * 3] - (double)gt[i * 3], dy = (double)pred[i * 3 + 1] - (double)gt[i * 3 + 1];
            const double d = sqrt(dx * dx + dy * dy);
            s[0] = d;
            for (int k = 0; k < tol.n; ++k) c[3 + k] = d <= tol.v[k];
        }
    }
    block_partials(s, c, 3 + tol.n, nblocks, psum, pcnt);
}

long long metric_blocks(long long n) { return (n + DE_THREADS - 1) / DE_THREADS; }
size_t metrics_workspace_bytes(long long n) { return n > 0 ? (size_t)metric_blocks(n) * (DE_SUMS * sizeof(double) + DE_COUNTS * sizeof(int)) : 0; }
// the factors of every map, then one partial per map and strip (out_h strips at most: strip height 1)
size_t loss_workspace_bytes(long long maps, int out_h, int out_w) {
    return maps > 0 && out_h > 0 && out_w > 0 ? (size_t)maps * ((size_t)2 * out_h + out_w) * sizeof(double) : 0;
}

int check_tolerances(const char* who, const double* tol, int ntol, Tolerances& t) {
    TTUP_REQUIRE(tol != nullptr, TTUP_EINVAL, "%s: null pointer", who);
    TTUP_REQUIRE(ntol >= 1 && ntol <= DE_MAX_TOL, TTUP_EINVAL, "%s: need 1 to %d tolerances, got %d", who, DE_MAX_TOL, ntol);
    for (int k = 0; k < DE_MAX_TOL; ++k) t.v[k] = k < ntol ? tol[k] : 0.0;
    t.n = ntol;
    return TTUP_OK;
}

// what ttup_detect_heatmap_loss and ttup_detect_heatmap_loss_grad (with_grad) share: the checks, both plans, the workspace, the
// factors, the loss pass (the gradient entry skips it when sums_dev is null) and the gradient pass on the same factors
int heatmap_loss_pass(const char* who, bool with_grad, const float* pred_dev, const double* centres_dev, const int* has_target_dev, int n, int c, int h, int w, double sigma,
                      int out_h, int out_w, int weighted, double scale, void* workspace_dev, size_t workspace_bytes, double* sums_dev, float* grad_dev, void* stream) {
    TTUP_REQUIRE(pred_dev && centres_dev && has_target_dev && workspace_dev && (with_grad ? grad_dev != nullptr : sums_dev != nullptr), TTUP_EINVAL, "%s: null pointer", who);
    TTUP_REQUIRE(n > 0 && c > 0, TTUP_EINVAL, "%s: need at least one sample and one channel, got n = %d, c = %d", who, n, c);
    TTUP_REQUIRE(h > 0 && w > 0 && out_h > 0 && out_w > 0, TTUP_EINVAL, "%s: empty heatmap or output: (%d, %d) -> (%d, %d)", who, h, w, out_h, out_w);
    TTUP_REQUIRE(sigma > 0.0, TTUP_EINVAL, "%s: sigma must be positive, got %g", who, sigma);          // (a NaN fails the comparison too)
    if (with_grad) TTUP_REQUIRE(isfinite(scale), TTUP_EINVAL, "%s: scale must be finite, got %g", who, scale);
    const long long maps = (long long)n * c;
    const LossPlan lp = loss_plan(h, w, out_h);          // the loss pass's limit holds for the pair, whether the sums are asked for or not
    TTUP_REQUIRE(lp.strip >= 1, TTUP_EINVAL, "%s: two source rows of %d floats do not fit the %zu bytes of LDS %s keeps them in (w <= %zu)", who, w, DE_ROW_BYTES,
                 with_grad ? "the loss pass" : "a workgroup", DE_ROW_BYTES / (2 * sizeof(float)));
    const GradPlan gp = with_grad ? dg_plan(h, w, out_h, out_w) : GradPlan();
    const int fblocks = (out_h + out_w + DE_THREADS - 1) / DE_THREADS;
    if (with_grad) {
        TTUP_REQUIRE(gp.strip >= 1 && gp.waves <= DG_MAX_WAVES && gp.lds <= DG_LDS_BYTES, TTUP_EINVAL, "%s: no plan for (%d, %d) -> (%d, %d)", who, h, w, out_h, out_w);
        TTUP_REQUIRE(maps * lp.nstrips <= 0x7fffffffLL && maps * fblocks <= 0x7fffffffLL && maps * gp.nstrips * gp.groups <= 0x7fffffffLL, TTUP_EINVAL, "%s: %lld maps exceed the grid", who, maps);
    } else {
        TTUP_REQUIRE(maps * lp.nstrips <= 0x7fffffffLL && maps * fblocks <= 0x7fffffffLL, TTUP_EINVAL, "%s: %lld maps of %d strips exceed the grid", who, maps, lp.nstrips);
    }
    TTUP_REQUIRE(((size_t)workspace_dev & 7) == 0, TTUP_EINVAL, "%s: the workspace must be 8-byte aligned", who);
    TTUP_REQUIRE(workspace_bytes >= loss_workspace_bytes(maps, out_h, out_w), TTUP_EINVAL, "%s: workspace of %zu bytes, need %zu (%s)", who, workspace_bytes,
                 loss_workspace_bytes(maps, out_h, out_w), with_grad ? "ttup_detect_loss_grad_workspace_bytes" : "ttup_detect_loss_workspace_bytes");
    double* fac = (double*)workspace_dev;
    double* partial = fac + (size_t)maps * (out_h + out_w);
    const double scale_y = (double)h / (double)out_h, scale_x = (double)w / (double)out_w;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(factor_kernel, dim3((unsigned)(maps * fblocks)), dim3(DE_THREADS), 0, st, centres_dev, has_target_dev, out_h, out_w, fblocks, 2.0 * sigma * sigma, fac);
    TTUP_LAUNCH_CHECK();
    if (sums_dev) {
        hipLaunchKernelGGL(loss_kernel, dim3((unsigned)(maps * lp.nstrips)), dim3(DE_THREADS), lp.lds, st, pred_dev, (const double*)fac, h, w, out_h, out_w, scale_y, scale_x,
                           lp.strip, lp.nstrips, weighted ? 1 : 0, partial);
        TTUP_LAUNCH_CHECK();
        hipLaunchKernelGGL(loss_final_kernel, dim3((unsigned)maps), dim3(DE_THREADS), 0, st, (const double*)partial, lp.nstrips, sums_dev);
        TTUP_LAUNCH_CHECK();
    }
    if (with_grad) {
        hipLaunchKernelGGL(grad_kernel, dim3((unsigned)(maps * gp.nstrips * gp.groups)), dim3(gp.waves * 64), gp.lds, st, pred_dev, (const double*)fac, h, w, out_h, out_w,
                           scale_y, scale_x, gp.strip, gp.nstrips, gp.waves, gp.groups, weighted ? 1 : 0, scale, grad_dev);
        TTUP_LAUNCH_CHECK();
    }
    return TTUP_OK;
}

// what the two metrics entries share once they know their item count: the workspace, the launch of their kernel (`launch`: nblocks,
// partials, stream -> the hipLaunchKernelGGL of that kernel) and the final reduction
template <typename Launch>
int metrics_pass(const char* who, long long n, const Tolerances& tol, void* workspace_dev, size_t workspace_bytes, double* sums_dev, long long* counts_dev, void* stream,
                 Launch launch) {
    TTUP_REQUIRE(n > 0, TTUP_EINVAL, "%s: need at least one sample, got n = %lld", who, n);
    TTUP_REQUIRE(((size_t)workspace_dev & 7) == 0, TTUP_EINVAL, "%s: the workspace must be 8-byte aligned", who);
    TTUP_REQUIRE(workspace_bytes >= metrics_workspace_bytes(n), TTUP_EINVAL, "%s: workspace of %zu bytes, need %zu (ttup_detect_metrics_workspace_bytes)", who, workspace_bytes,
                 metrics_workspace_bytes(n));
    const long long nb = metric_blocks(n);
    const EvalPartials p = eval_partials(workspace_dev, nb, DE_SUMS);
    hipStream_t st = (hipStream_t)stream;
    launch(nb, p, st);
    TTUP_LAUNCH_CHECK();
    return eval_finish(p, nb, DE_SUMS, 3 + tol.n, n, sums_dev, counts_dev, st);
}

}  // namespace

extern "C" size_t ttup_detect_loss_workspace_bytes(int n_maps, int out_h, int out_w) { return loss_workspace_bytes(n_maps, out_h, out_w); }

extern "C" size_t ttup_detect_metrics_workspace_bytes(int n_items) { return metrics_workspace_bytes(n_items); }

extern "C" int ttup_detect_heatmap_loss(const float* pred_dev, const double* centres_dev, const int* has_target_dev, int n, int c, int h, int w, double sigma, int out_h,
                                        int out_w, int weighted, void* workspace_dev, size_t workspace_bytes, double* sums_dev, void* stream) {
    return heatmap_loss_pass("ttup_detect_heatmap_loss", false, pred_dev, centres_dev, has_target_dev, n, c, h, w, sigma, out_h, out_w, weighted, 0.0, workspace_dev,
                             workspace_bytes, sums_dev, nullptr, stream);
}

extern "C" size_t ttup_detect_loss_grad_workspace_bytes(int n_maps, int h, int w, int out_h, int out_w) {
    return h > 0 && w > 0 ? loss_workspace_bytes(n_maps, out_h, out_w) : 0;
}

extern "C" int ttup_detect_heatmap_loss_grad(const float* pred_dev, const double* centres_dev, const int* has_target_dev, int n, int c, int h, int w, double sigma, int out_h,
                                             int out_w, int weighted, double scale, void* workspace_dev, size_t workspace_bytes, double* sums_dev, float* grad_dev,
                                             void* stream) {
    return heatmap_loss_pass("ttup_detect_heatmap_loss_grad", true, pred_dev, centres_dev, has_target_dev, n, c, h, w, sigma, out_h, out_w, weighted, scale, workspace_dev,
                             workspace_bytes, sums_dev, grad_dev, stream);
}

extern "C" int ttup_detect_ball_metrics(const float* pred_pos_dev, const float* gt_dev, const float* gt_min_dev, const float* gt_max_dev, const int* vis_dev, int n,
                                        const double* tolerances, int n_tolerances, void* workspace_dev, size_t workspace_bytes, double* sums_dev,
                                        long long* counts_dev, void* stream) {
    const char* who = "ttup_detect_ball_metrics";
    TTUP_REQUIRE(pred_pos_dev && gt_dev && gt_min_dev && gt_max_dev && vis_dev && workspace_dev && sums_dev && counts_dev, TTUP_EINVAL, "%s: null pointer", who);
    Tolerances tol;
    if (int rc = check_tolerances(who, tolerances, n_tolerances, tol)) return rc;
    return metrics_pass(who, n, tol, workspace_dev, workspace_bytes, sums_dev, counts_dev, stream, [&](long long nb, const EvalPartials& p, hipStream_t st) {
        hipLaunchKernelGGL(ball_metrics_kernel, dim3((unsigned)nb), dim3(DE_THREADS), 0, st, pred_pos_dev, gt_dev, gt_min_dev, gt_max_dev, vis_dev, (long long)n, tol, nb, p.psum,
                           p.pcnt);
    });
}

extern "C" int ttup_detect_table_metrics(const float* pred_pos_dev, const float* gt_dev, int n, int keypoints, const double* tolerances, int n_tolerances,
                                         void* workspace_dev, size_t workspace_bytes, double* sums_dev, long long* counts_dev, void* stream) {
    const char* who = "ttup_detect_table_metrics";
    TTUP_REQUIRE(pred_pos_dev && gt_dev && workspace_dev && sums_dev && counts_dev, TTUP_EINVAL, "%s: null pointer", who);
    Tolerances tol;
    if (int rc = check_tolerances(who, tolerances, n_tolerances, tol)) return rc;
    TTUP_REQUIRE(n > 0 && keypoints > 0, TTUP_EINVAL, "%s: need at least one sample and one keypoint, got n = %d, keypoints = %d", who, n, keypoints);
    const long long items = (long long)n * keypoints;
    TTUP_REQUIRE(items <= 0x7fffffffLL, TTUP_EINVAL, "%s: %lld keypoints exceed 2^31 - 1", who, items);
    return metrics_pass(who, items, tol, workspace_dev, workspace_bytes, sums_dev, counts_dev, stream, [&](long long nb, const EvalPartials& p, hipStream_t st) {
        hipLaunchKernelGGL(table_metrics_kernel, dim3((unsigned)nb), dim3(DE_THREADS), 0, st, pred_pos_dev, gt_dev, items, tol, nb, p.psum, p.pcnt);
    });
}

#include "no_packed_fp32_end.h"
