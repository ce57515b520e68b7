// The heatmap-loss gradient's decisions without a device: which output rows / columns read which source row / column, with which
// weight, and how a map's source rows are cut into strips.  Standard library only -- the same source compiles for gfx950 (hipcc:
// csrc/detect_eval.hip's grad_kernel calls these functions) and for the host (g++: tests/helpers/host_detect_grad_plan.cpp sweeps
// them), so the host and the kernel cannot disagree about which output index touches which source index.
//
// One axis at a time (the interpolation is separable).  An output index dst reads the source indices i0 and i1 of dg_src_coord with
// the weights 1 - lam and lam; where the clamp at the last index makes i1 == i0 that index gets their sum.  The source coordinate is
// monotone in dst, so the output indices whose i0 is at least k start at dg_first(k) and the readers of the source index i are
//     [dg_first(i - 1), dg_first(i))        reading i as their i1, weight lam
//     [dg_first(i), dg_first(i + 1))        reading i as their i0, weight 1 - lam (or the sum)
// -- one contiguous range, empty when a downsampling skips i.
#pragma once
#include <stddef.h>

#ifndef TTUP_HD
#if defined(__HIPCC__)
#define TTUP_HD __host__ __device__
#else
#define TTUP_HD
#endif
#endif

namespace ttup {

constexpr int DG_STRIP = 8;                       // source rows per workgroup, at most
constexpr int DG_LANES = 63;                      // source columns a wave owns: its lanes 1 .. 63; lane 0 recomputes the column before them
constexpr int DG_MAX_WAVES = 8;                   // waves per workgroup, at most
constexpr size_t DG_LDS_BYTES = 60 * 1024;        // dynamic LDS of a workgroup, at most (there is no static part): 10 rows of 506 floats are 20 KB

// torch's upsample_bilinear2d, align_corners = False, no antialiasing; scale = in / out.  The coordinate lives here alone: the loss
// pass (csrc/detect_eval.hip's loss_kernel, csrc/detect_loss_plan.h) reads it through dg_src_coord as the gradient does.
// the clamped source coordinate of dst: an add, a multiply and a subtract, each rounded -- never an fma, on the device as on the
// host (the pragma stands inside the body, as in mt19937.h, so that a unit that includes this header keeps its own setting).
// This is the one place the coordinate is written: the ranges, the weights and the kernel's inner loop all come through it.
TTUP_HD inline double dg_coord(int dst, double scale) {
#pragma clang fp contract(off)
    const double s = ((double)dst + 0.5) * scale - 0.5;
    return s < 0.0 ? 0.0 : s;
}

// lambda of an output index whose lower source index is known to be i0 (the kernel's inner loop: i0 comes from dg_first's ranges)
TTUP_HD inline double dg_lambda(int dst, double scale, int i0) { return dg_coord(dst, scale) - (double)i0; }

// the source indices dst interpolates between and its lambda: i0 = floor of the coordinate, i1 clamped at the last index
TTUP_HD inline void dg_src_coord(int dst, double scale, int in, int& i0, int& i1, double& lam) {
    const double s = dg_coord(dst, scale);
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;                        // (unreachable: s < in - 0.5; keeps every index in bounds whatever scale is)
    i1 = i0 < in - 1 ? i0 + 1 : i0;
    lam = s - (double)i0;
}

// the weights with which dst reads i0 (w0) and i0 + 1 (w1; 0 where the clamp folds both onto i0); lam: the interpolation's own
TTUP_HD inline void dg_weights(int dst, double scale, int in, int& i0, int& i1, double& lam, double& w0, double& w1) {
    dg_src_coord(dst, scale, in, i0, i1, lam);
    w0 = 1.0 - lam;
    w1 = lam;
    if (i1 == i0) {
        w0 = w0 + lam;
        w1 = 0.0;
    }
}

// the smallest dst in [0, out] whose i0 is at least k (out: none).  The estimate inverts the coordinate; the two walks settle it
// with dg_src_coord itself, so the answer is exact whatever the estimate's rounding.
TTUP_HD inline int dg_first(int k, double scale, int in, int out) {
    if (k <= 0) return 0;
    const double e = ((double)k + 0.5) / scale - 0.5;
    int d = e < 0.0 ? 0 : (e > (double)out ? out : (int)e);
    int i0, i1;
    double lam;
    while (d > 0) {
        dg_src_coord(d - 1, scale, in, i0, i1, lam);
        if (i0 < k) break;
        --d;
    }
    while (d < out) {
        dg_src_coord(d, scale, in, i0, i1, lam);
        if (i0 >= k) break;
        ++d;
    }
    return d;
}

// the output indices that read the source index i: [lo, hi)
TTUP_HD inline void dg_readers(int i, double scale, int in, int out, int& lo, int& hi) {
    lo = dg_first(i - 1, scale, in, out);
    hi = dg_first(i + 1, scale, in, out);
}

// A workgroup takes the source rows [r0, r0 + strip) and one group of source columns of one map.  It walks the output rows whose i0
// lies in r0 - 1 .. r0 + strip - 1 and keeps the source rows r0 - 1 .. r0 + strip (inside the map) of its columns in LDS as fp32.
// Wave v of group g owns the DG_LANES columns from (g * waves + v) * DG_LANES with its lanes 1 .. 63.
struct GradPlan {
    int strip = 0;          // 0: the shape is refused
    int nstrips = 0;
    int waves = 0;          // waves per workgroup
    int groups = 0;         // column groups: groups * waves * DG_LANES >= w
    size_t lds = 0;         // dynamic LDS bytes of a workgroup
};

// the source column lane `lane` of wave `wave` of group `group` serves (-1 or >= w: none); lane 0's is the last column of the wave before
TTUP_HD inline int dg_column(int group, int waves, int wave, int lane) { return (group * waves + wave) * DG_LANES - 1 + lane; }

// first / one past the last source column a group keeps in LDS: its lanes' columns and the right neighbour of the last
TTUP_HD inline void dg_group_columns(int group, int waves, int w, int& lo, int& hi) {
    lo = dg_column(group, waves, 0, 0) > 0 ? dg_column(group, waves, 0, 0) : 0;
    hi = dg_column(group, waves, waves - 1, 63) + 2 < w ? dg_column(group, waves, waves - 1, 63) + 2 : w;
}

TTUP_HD inline size_t dg_lds_bytes(int strip, int w, int waves) {
    const int cw = waves * DG_LANES + 2 < w ? waves * DG_LANES + 2 : w;
    return (size_t)(strip + 2) * cw * sizeof(float);
}

// first / one past the last source row a strip keeps in LDS
TTUP_HD inline void dg_strip_rows(int r0, int strip, int h, int& lo, int& hi) {
    lo = r0 > 0 ? r0 - 1 : 0;
    hi = r0 + strip + 1 < h ? r0 + strip + 1 : h;
}

// the fewest column groups of at most DG_MAX_WAVES waves, the fewest waves that serve them, strips of DG_STRIP rows; refused
// (strip 0): an empty map or output
inline GradPlan dg_plan(int h, int w, int out_h, int out_w) {
    GradPlan p;
    if (h <= 0 || w <= 0 || out_h <= 0 || out_w <= 0) return p;
    const int nwaves = (w + DG_LANES - 1) / DG_LANES;
    p.strip = DG_STRIP < h ? DG_STRIP : h;
    p.nstrips = (h + p.strip - 1) / p.strip;
    p.groups = (nwaves + DG_MAX_WAVES - 1) / DG_MAX_WAVES;
    p.waves = (nwaves + p.groups - 1) / p.groups;
    p.lds = dg_lds_bytes(p.strip, w, p.waves);
    return p;
}

}  // namespace ttup
