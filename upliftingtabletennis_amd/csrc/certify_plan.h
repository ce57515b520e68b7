// The certified argmax's decisions without a device: constants, status values, counter names, the crop record, the crop geometry
// and the sizing of a handle's certification state.  Standard library and include/ttup.h only -- the same source compiles for
// gfx950 (hipcc: csrc/certify.hip calls these functions from its kernels) and for the host (g++: tests/helpers/host_certify_plan.cpp
// checks the geometry exhaustively per axis, the progress of the crop walk, the sizing table and the names).
#pragma once
#include "../../include/ttup.h"
#include <stdio.h>

#ifndef TTUP_HD
#if defined(__HIPCC__)
#define TTUP_HD __host__ __device__
#else
#define TTUP_HD
#endif
#endif

namespace ttup {

constexpr int CERT_MAX_K = 512;                 // candidates per heatmap the plan kernel can sort (CertState::K <= this)
constexpr int CERT_MAX_FRAME_CROPS = 32;        // crops the heatmaps of one frame may open in all
constexpr int CERT_R = 72;                      // receptive-field radius of one heatmap pixel (measured: 71)
constexpr int CERT_SMALL = 14;                  // core positions of a class-2 crop

// Per-heatmap status (ttup.h).  ttup_wasb_certify_status returns `& CERT_STATUS_MASK`, ttup_wasb_certify_flags `& CERT_FLAGS_MASK`;
// the two bits above the masks live only between the plan and the resolve kernel.
enum : int {
    CERT_SINGLE = 0,                 // one candidate: the bf16 index is certain
    CERT_RESOLVED = 1,               // settled on fp32 crops
    CERT_NOT_CERTIFIED = 2,          // candidate / crop budget exceeded
    CERT_STATUS_MASK = 3,
    CERT_GUARD = 4,                  // the guard band below the candidate band is not empty
    CERT_FLAGS_MASK = 7,
    CERT_PENDING = 8,                // provisional: the heatmap's crops wait for their ids on the call's shared list
    CERT_AUDIT_ONLY = 16,            // its crop only MEASURES (audit crop of a single-candidate heatmap): index and window stay the bf16 path's
};

// The twelve counters of ttup_wasb_certify_stats, in ABI order (upliftingtabletennis_amd/_lib.py CERT_STATS mirrors the names)
#define TTUP_CERT_STATS(X)                                                                                                           \
    X(heatmaps) X(single) X(resolved) X(not_certified) X(crops) X(candidates) X(max_candidate_err) X(exact_singles) X(over_candidates) \
    X(over_crops_per_map) X(over_crop_list) X(small_crops)
enum CertStat {
#define X(name) CS_##name,
    TTUP_CERT_STATS(X)
#undef X
    CERT_N_STATS
};
inline const char* cert_stat_name(int k) {
    static const char* const names[CERT_N_STATS] = {
#define X(name) #name,
        TTUP_CERT_STATS(X)
#undef X
    };
    return k >= 0 && k < CERT_N_STATS ? names[k] : "";
}

// One fp32 crop of a call's list: the Hc x Wc window at (y0, x0) of sample `frame`; cls = 1: a class-2 crop (candidates within the
// CERT_SMALL-position core)
struct CropRec { int frame, y0, x0, cls; };

// ---- geometry, one axis at a time: a crop of `c` positions at origin `o` of an axis of `full` positions

// valid core of a crop: positions whose value AND 3x3 neighbourhood are exact -- at least R + 1 inside the crop, or up to a true
// image border, where the crop's zero padding IS the frame's
// (small > 0: a class-2 crop, pruned to the cone of the positions R + 1 .. R + small: only those are exact)
TTUP_HD inline void cert_core_range(int o, int c, int full, int R, int small, int& lo, int& hi) {
    lo = (o == 0) ? 0 : o + R + 1;
    hi = (o + c == full) ? full : (small > 0 ? o + R + 1 + small : o + c - R - 1);
}

// origin of the crop that puts `centre` in the middle of its core: rounded to a multiple of 8 (the three stride-2 levels and the
// nearest-neighbour upsampling then sample exactly as in the full frame; full - c is a multiple of 8, cert_sizing) and clamped
TTUP_HD inline int cert_crop_origin(int centre, int c, int full, int R, int small) {
    const int mid = small > 0 ? R + 1 + small / 2 : c / 2;          // crop position of the centre
    const int o = (centre - mid + 4) & ~7;          // rounded to the nearest multiple of 8, also below 0 (no shift of a negative value)
    return o < 0 ? 0 : (o > full - c ? full - c : o);
}

// A new crop for sorted[first], the first candidate (index order, so the top-most) that no crop of the frame holds: centred on the
// bounding box of the candidates from `first` on that can share it.  With the origin ROUNDED to a multiple of 8 the core covers
// centre - 7 .. centre + 7 at least, so a cluster of up to 15 x 15 pixels -- the flat top of a saturated blob -- takes ONE crop.
// Class 2: a cluster that fits a core of `small` positions with the same rounding slack (span <= small - 8; every single candidate
// does) is centred on the core R + 1 .. R + small instead of the crop's centre; its fp32 pass is pruned to the cone of THAT core,
// which ends 8 pixels short of the crop's last row / column (conv.h Roi).
// The whole bounding box -- sorted[first] with it, which is what lets the walk end -- lies in the new crop's core: the spans the
// walk allows leave the 7 positions that rounding can cost on either side (tests/test_certify_plan_host.py, every case per axis).
struct NewCrop { int y0, x0, small; };
TTUP_HD inline NewCrop cert_open_crop(const int* sorted, int cnt, int first, int H, int W, int Hc, int Wc, int R, int small) {
    const int fy = sorted[first] / W, fx = sorted[first] % W;
    const int span_y = Hc - 2 * R - 2 - 7, span_x = Wc - 2 * R - 2 - 7;
    int ylo = fy, yhi = fy, xlo = fx, xhi = fx;
    for (int j = first + 1; j < cnt; ++j) {
        const int yj = sorted[j] / W, xj = sorted[j] % W;
        if (yj - fy >= span_y) break;
        const int nxlo = xj < xlo ? xj : xlo, nxhi = xj > xhi ? xj : xhi;
        if (nxhi - nxlo >= span_x) continue;
        xlo = nxlo; xhi = nxhi; yhi = yj;
    }
    NewCrop n;
    n.small = (small > 0 && yhi - ylo <= small - 8 && xhi - xlo <= small - 8) ? small : 0;
    n.y0 = cert_crop_origin((ylo + yhi) / 2, Hc, H, R, n.small);
    n.x0 = cert_crop_origin((xlo + xhi) / 2, Wc, W, R, n.small);
    return n;
}

// Audit crops (ttup_wasb_certify_audit_crops): the single candidate of ONE channel of every audit_mod-th frame gets a crop too
TTUP_HD inline bool cert_audit_pick(int audit_mod, int audit_phase, int cnt, int frame, int ch, int C) {
    return audit_mod > 0 && cnt == 1 && (frame + audit_phase) % audit_mod == 0 && ch == (frame / audit_mod) % C;
}

// Cone pruning applies to INTERIOR crops: a crop on an image border has a core that reaches that border (its zero padding IS the
// frame's), i.e. a wider cone: those are computed in full.  0 = in full, 1 / 2 = pruned to the class-1 / class-2 regions (conv.h Roi)
TTUP_HD inline int cert_roi_class(const CropRec& r, int H, int W, int Hc, int Wc) {
    return (r.y0 <= 0 || r.x0 <= 0 || r.y0 + Hc >= H || r.x0 + Wc >= W) ? 0 : (r.cls ? 2 : 1);
}

// ---- sizing of a handle's certification state (ttup_wasb_set_certify)

// experiment knobs, read from the environment once (csrc/certify.hip cert_knobs)
struct CertKnobs {
    int list = 0;                // TTUP_CERT_LIST: capacity of the call's crop list per heatmap, 1 .. 16 (else 4)
    int ch = 0;                  // TTUP_CERT_CH: crops per fp32 pass, 8 .. 512 (else 128)
    bool no_small = false;       // TTUP_CERT_SMALL=0: no class-2 crops
    bool no_cone = false;        // TTUP_NO_CONE / TTUP_F32_EXACT / TTUP_F32_DIRECT: the crop net is computed in full
};

struct CertSizing {
    int rc = TTUP_OK;
    char msg[256] = "";          // for ttup_last_error when rc != TTUP_OK
    int Hc = 0, Wc = 0;          // crop size
    int CH = 0;                  // crops per fp32 pass
    int maxc = 0, maxf = 0;      // new crops a heatmap may add / crops a frame may use in all (its channels share them)
    int max_crops = 0;           // capacity of the call's crop list = nchunks * CH
    int nchunks = 0;
    int budget = 0;              // crops a forward may use until ttup_wasb_certify_budget says otherwise: one per sample
    bool cone = false;           // the crop net is pruned to the cone of the core (interior crops)
    int small = 0;               // core positions of the class-2 crops (0 = off; needs the cone pruning)
};

inline bool cert_args_ok(int crop, int max_crops_per_map) { return crop >= 0 && max_crops_per_map >= 0 && max_crops_per_map <= CERT_MAX_FRAME_CROPS; }

inline CertSizing cert_sizing(int H, int W, int max_batch, int n_out, int crop, int max_crops_per_map, const CertKnobs& knobs) {
    CertSizing s;
    const int R = CERT_R;
#define CERT_SIZING_REQUIRE(cond, ...) do { if (!(cond)) { s.rc = TTUP_EINVAL; snprintf(s.msg, sizeof s.msg, __VA_ARGS__); return s; } } while (0)
    CERT_SIZING_REQUIRE(cert_args_ok(crop, max_crops_per_map), "ttup_wasb_set_certify: bad argument");
    s.maxc = max_crops_per_map > 0 ? max_crops_per_map : 8;
    s.maxf = s.maxc * n_out < CERT_MAX_FRAME_CROPS ? s.maxc * n_out : CERT_MAX_FRAME_CROPS;
    // Crop side: 2 R + the core.  The origin of a crop is a multiple of 8 (the 1/8-resolution branch), so a crop centred on a candidate
    // has it within 4 pixels of its centre: the core must hold 8 positions + the 3x3 window = 2 R + 16 at least.
    const int side = crop > 0 ? crop : 168;
    CERT_SIZING_REQUIRE(side % 8 == 0 && side >= 2 * R + 16, "ttup_wasb_set_certify: crop %d must be a multiple of 8 and at least %d", side, 2 * R + 16);
    s.Hc = side < H ? side : H;
    s.Wc = side < W ? side : W;
    // the scan reads float4 quads of whole heatmaps; a crop is exact only when its (clamped) origin is a multiple of 8
    CERT_SIZING_REQUIRE(((long long)H * W) % 4 == 0 && (H - s.Hc) % 8 == 0 && (W - s.Wc) % 8 == 0,
                        "ttup_wasb_set_certify: %dx%d heatmaps with %dx%d crops cannot be certified (H*W %% 4, (H-Hc) %% 8, (W-Wc) %% 8 must be 0)", H, W, s.Hc, s.Wc);
    const int ch_cap = knobs.ch >= 8 && knobs.ch <= 512 ? knobs.ch : 128;          // 128 against 64: fewer, fuller passes
    s.CH = max_batch < ch_cap ? max_batch : ch_cap;
    // the call's crop list: four crops per heatmap on average (the overflow is flagged), and never less than ONE frame may ask for
    // (one-sample handles: re-certification of single frames); rounded up to whole passes
    const int per_map = knobs.list > 0 && knobs.list <= 16 ? knobs.list : 4;
    s.max_crops = per_map * max_batch > s.maxf ? per_map * max_batch : s.maxf;
    s.nchunks = (s.max_crops + s.CH - 1) / s.CH;
    CERT_SIZING_REQUIRE(s.nchunks <= 64, "ttup_wasb_set_certify: max_batch %d too large", max_batch);
    s.max_crops = s.nchunks * s.CH;
    s.budget = max_batch;
    // cone pruning of the crop net: an interior crop's candidates lie R + 1 pixels inside it, their 3x3 windows one more: only the
    // heatmap rows / columns [R, side - R) are ever read, and every layer only has to produce what those depend on.
    // Class 2: a 16-pixel heatmap region (14 candidate positions + their 3x3 windows) at the crop's corner-aligned end of the core
    // range -- its cone is the crop's first 160 rows / columns, i.e. one 16-pixel tile row / column less in the full-resolution layers
    s.cone = !knobs.no_cone && s.Hc == s.Wc && s.Hc > 2 * R + 2 && s.Hc < H && s.Wc < W;
    s.small = (s.cone && !knobs.no_small && s.Hc >= 2 * R + 24) ? CERT_SMALL : 0;
#undef CERT_SIZING_REQUIRE
    return s;
}

}  // namespace ttup
