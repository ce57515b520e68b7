// The heatmap-loss pass's decisions without a device: which source rows a strip of output rows keeps in LDS, in which slot, and how
// many output rows a workgroup takes.  Standard library only -- the same source compiles for gfx950 (hipcc: csrc/detect_eval.hip's
// loss_kernel calls these functions, its entry points call loss_plan) and for the host (g++: tests/helpers/host_detect_loss_plan.cpp
// sweeps them), so the kernel's fill loop, its reads and the LDS size it is launched with cannot disagree.
//
// The coordinate is detect_grad_plan.h's dg_src_coord: an output row reads the source rows i0 and i1.  A strip of nr output rows
// from r0 lies between at most min(span, 2 nr) source rows, span = i1(last row) - i0(first row) + 1.  When span <= 2 nr (every
// upsampling, and downsampling by less than 2) the rows i0(first) .. i1(last) are kept in order: slot = row - i0(first).  Otherwise
// (strong downsampling, the rows are far apart) row i of the strip keeps its own pair in the slots 2 i and 2 i + 1.
#pragma once
#include "detect_grad_plan.h"

namespace ttup {

constexpr int DE_STRIP = 8;                              // output rows per workgroup, at most
constexpr size_t DE_ROW_BYTES = 60 * 1024;               // LDS for the source rows of a strip (dynamic); the kernel's static part is < 1 KB

struct LossStrip {
    int ylo;                // the first source row kept (contiguous layout)
    bool contiguous;
    int slots;              // source rows kept
};

// the layout of the strip of nr output rows from r0
TTUP_HD inline LossStrip dl_strip(int r0, int nr, double scale, int in) {
    LossStrip s;
    int a, b, yhi;
    double lam;
    dg_src_coord(r0, scale, in, s.ylo, b, lam);
    dg_src_coord(r0 + nr - 1, scale, in, a, yhi, lam);
    const int span = yhi - s.ylo + 1;
    s.contiguous = span <= 2 * nr;
    s.slots = s.contiguous ? span : 2 * nr;
    return s;
}

// the source row the fill loop copies into slot `slot`
TTUP_HD inline int dl_slot_row(const LossStrip& s, int r0, int slot, double scale, int in) {
    int y = s.ylo + slot;
    if (!s.contiguous) {
        int i0, i1;
        double lam;
        dg_src_coord(r0 + (slot >> 1), scale, in, i0, i1, lam);
        y = (slot & 1) ? i1 : i0;
    }
    return y;
}

// the slot in which row i of the strip (output row r0 + i) finds the source row y it reads: its i0 (upper 0) or its i1 (upper 1)
TTUP_HD inline int dl_slot(const LossStrip& s, int i, int upper, int y) { return s.contiguous ? y - s.ylo : 2 * i + upper; }

struct LossPlan {
    int strip = 0;          // output rows per workgroup; 0: the shape is refused
    int slots = 0;          // the most source rows a strip keeps
    int nstrips = 0;
    size_t lds = 0;         // dynamic LDS bytes of a workgroup
};

// the largest strip height <= DE_STRIP whose worst strip fits DE_ROW_BYTES; refused (strip 0): two rows of w floats do not fit, or
// an empty map or output
inline LossPlan loss_plan(int h, int w, int out_h) {
    LossPlan p;
    if (h <= 0 || w <= 0 || out_h <= 0) return p;
    const double scale = (double)h / (double)out_h;
    for (int strip = DE_STRIP; strip >= 1; --strip) {
        int slots = 0;
        for (int r0 = 0; r0 < out_h; r0 += strip) {
            const int s = dl_strip(r0, out_h - r0 < strip ? out_h - r0 : strip, scale, h).slots;
            slots = s > slots ? s : slots;
        }
        if ((size_t)slots * w * sizeof(float) <= DE_ROW_BYTES) {
            p.strip = strip;
            p.slots = slots;
            p.nstrips = (out_h + strip - 1) / strip;
            p.lds = (size_t)slots * w * sizeof(float);
            return p;
        }
    }
    return p;
}

}  // namespace ttup
