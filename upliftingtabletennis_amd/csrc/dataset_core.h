// One uplift training sample from one generated trajectory: the reference's uplifting/data.py::TableTennisDataset.__getitem__
// (:77-166), sample_camera (:168-223), transform_resolution (:527-553) and the train transforms of uplifting/transformations.py
// (MotionBlur, RandomizeDetections, RandomStop, RandomDetection, RandomMissing, TableMissing, NormalizeImgCoords), in the
// reference's order and in fp64 like its numpy.  One call = one sample = one (trajectory, seed) pair; everything is sequential
// because every draw's place in the two MT19937 streams depends on how the rejections before it went.
//
// Randomness: the sample's two streams are CPython's `random` after random.seed(s) (init_by_array) and numpy's legacy global
// stream after np.random.seed(s) (init_genrand): both are mt19937.h, which csrc/trajgen.hip seeds from as well.  The table
// keypoints are scene.h's.
//
// No fma contraction anywhere in this file: the time grid, the nearest-frame differences and RandomStop's |times - hit| decide
// integer outputs and must round like numpy's separate operations (mt19937.h switches it off for the doubles built from MT
// words and the polar method's r2 on its own).
//
// The same source compiles for gfx950 (hipcc, the product: csrc/dataset.hip runs it one lane per sample) and for the host
// (g++, test infrastructure only: tests/helpers/host_dataset.cpp, compared with the reference's fixture on the CPU).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "mt19937.h"
#include "scene.h"

#pragma clang fp contract(off)

namespace ttup {
namespace ds {

constexpr int SEQ = 50;               // sequence_len: crop or pad to this
constexpr int NTAB = scene::N_KEYPOINTS;
constexpr int MAX_T = 128;            // frames kept for the camera test (the generator's 1 s at 65 fps gives at most 65)
constexpr int MAX_TRIES = 100;
constexpr double IMG_W = 2560.0, IMG_H = 1440.0;          // uplifting/helper.py WIDTH, HEIGHT
constexpr double ORIG_W = 2560.0, ORIG_H = 1440.0;        // original_resolution of the simulated frames
using scene::PI;
using scene::TABLE_HEIGHT;
// np.rad2deg(math.atan2(TABLE_WIDTH / 2, TABLE_LENGTH / 2)), printed with 17 significant digits
constexpr double PHI_LO = 29.098971272734509, PHI_HI = PHI_LO + 180.0;
constexpr double FX_LO = 0.6 * 2710, FX_HI = 2.0 * 2710, FY_LO = 0.6 * 2907, FY_HI = 2.0 * 2907;
enum { T_BLUR = 1, T_RANDOMIZE = 2, T_STOP = 4, T_RANDDET = 8, T_RANDMISS = 16, T_TABLEMISS = 32, T_NORMALIZE = 64 };
enum { OUT_R_IMG, OUT_TABLE_IMG, OUT_MASK, OUT_R_WORLD, OUT_ROTATION, OUT_TIMES, OUT_BOUNCES, OUT_MINT, OUT_MEXT, N_OUT };
// record (tests): nearest stored sample, blur sample, dropped flag per frame slot
constexpr int RECORD_INTS = 3 * SEQ;

struct Args {
    const double* rows;               // (R, 9) packed trajectories: position, velocity, rotation
    const long long* offsets;         // (V + 1)
    long long n_rows;
    const double* bounces;            // (V, 4)
    const int* n_bounces;             // (V)
    const double* times;              // (n_times) shared time labels
    int n_times;
    const double* mext;               // (V or 1, 16), test mode
    const double* mint;               // (V or 1, 9)
    int cam_per_traj;
    int n_traj;
    int mode;                         // 0 train, 1 test
    unsigned enabled;                 // T_* bits (the six random ones count in train mode only)
    double blur_strength, randomize_std, stop_prob, randdet_prob, randmiss_prob, tablemiss_prob;
    float* out32[N_OUT];              // each (N, ...) contiguous; the whole set may be null
    double* out64[N_OUT];             // the same in fp64 (tests), may be null
    int* diag;                        // (N, 4): fps, n_frames, camera_tries, camera_success
    int* record;                      // (N, RECORD_INTS) or null
};

// world2cam + cam2img (uplifting/helper.py:137-204) of one point: homogeneous product with the 4x4, division by its fourth
// component, product with the 3x3, division by the third
TTUP_DS_HD inline void project(const double* ex, const double* in, const double* p, double* u, double* v) {
    double c[4];
    for (int i = 0; i < 4; ++i) c[i] = ex[4 * i] * p[0] + ex[4 * i + 1] * p[1] + ex[4 * i + 2] * p[2] + ex[4 * i + 3] * 1.0;
    const double xc = c[0] / c[3], yc = c[1] / c[3], zc = c[2] / c[3];
    const double q0 = in[0] * xc + in[1] * yc + in[2] * zc, q1 = in[3] * xc + in[4] * yc + in[5] * zc, q2 = in[6] * xc + in[7] * yc + in[8] * zc;
    *u = q0 / q2;
    *v = q1 / q2;
}

TTUP_DS_HD inline int lower_bound(const double* t, int n, double x) {        // first index with t[i] >= x
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (t[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}
TTUP_DS_HD inline int upper_bound(const double* t, int n, double x) {        // first index with t[i] > x
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (t[mid] <= x) lo = mid + 1; else hi = mid; }
    return lo;
}

TTUP_DS_HD inline void table_point(int k, double* p) {
    p[0] = scene::TABLE_PTS[k][0]; p[1] = scene::TABLE_PTS[k][1]; p[2] = scene::TABLE_PTS[k][2];
}

TTUP_DS_HD inline double norm3(const double* a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
TTUP_DS_HD inline void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// one camera of sample_camera from eight uniforms, in the reference's draw order
TTUP_DS_HD inline void draw_camera(MT& py, double* ex, double* in) {
    const double fx = py.uniform(FX_LO, FX_HI), fy = py.uniform(FY_LO, FY_HI);
    in[0] = fx; in[1] = 0.0; in[2] = (IMG_W - 1) / 2; in[3] = 0.0; in[4] = fy; in[5] = (IMG_H - 1) / 2; in[6] = 0.0; in[7] = 0.0; in[8] = 1.0;
    const double distance = py.uniform(7.0, 17.0);
    const double phi = py.uniform(PHI_LO, PHI_HI);
    const double theta = py.uniform(30.0, 70.0);
    const double lookat[3] = {py.uniform(-0.2, 0.2), py.uniform(-0.2, 0.2), TABLE_HEIGHT};
    const double th = theta * (PI / 180.0), ph = phi * (PI / 180.0);
    double c[3] = {distance * sin(th) * cos(ph), distance * sin(th) * sin(ph), distance * cos(th)};
    c[2] += TABLE_HEIGHT;
    const double d[3] = {c[0] - lookat[0], c[1] - lookat[1], c[2] - lookat[2]};
    const double dn = norm3(d);
    const double f[3] = {-d[0] / dn, -d[1] / dn, -d[2] / dn};
    const double eps = py.uniform(-0.1, 0.1);
    double r[3] = {-f[1] / f[0] - f[2] / f[0] * eps, 1.0, eps};
    double rn = norm3(r);
    r[0] /= rn; r[1] /= rn; r[2] /= rn;
    const double u2 = -(f[0] * r[1] - f[1] * r[0]);          // z of u = -cross(f, r)
    if (u2 < 0) {                                            // the up vector has to point upwards: take the other r
        r[0] = f[1] / f[0] - f[2] / f[0] * eps; r[1] = -1.0; r[2] = eps;
        rn = norm3(r);
        r[0] /= rn; r[1] /= rn; r[2] /= rn;
    }
    double up[3];
    cross3(f, r, up);
    const double un = norm3(up);
    up[0] /= un; up[1] /= un; up[2] /= un;
    const double* R[3] = {r, up, f};
    for (int i = 0; i < 3; ++i) {
        ex[4 * i] = R[i][0]; ex[4 * i + 1] = R[i][1]; ex[4 * i + 2] = R[i][2];
        ex[4 * i + 3] = -(R[i][0] * c[0] + R[i][1] * c[1] + R[i][2] * c[2]);
    }
    ex[12] = 0.0; ex[13] = 0.0; ex[14] = 0.0; ex[15] = 1.0;
}

TTUP_DS_HD inline void put(const Args& a, int which, size_t at, double v) {
    if (a.out32[0]) a.out32[which][at] = (float)v;
    if (a.out64[0]) a.out64[which][at] = v;
}

// sample s of the launch: trajectory ti, streams py / np (seeded, position 0)
TTUP_DS_HD inline void build_sample(const Args& a, size_t s, long long ti, MT& py, MT& np) {
    int* diag = a.diag + 4 * s;
    const long long off = a.offsets[ti];
    const long long nl = a.offsets[ti + 1] - off;
    const bool train = a.mode == 0;
    double rimg[SEQ][2], tm[SEQ], tab[NTAB][3], ex[16], in[9];
    int widx[SEQ];                    // stored sample behind r_world[j]: k >= 0 the row, -1 zeros, -(k + 2) the row times zero
    short near[MAX_T];
    int rec_blur[SEQ];
    unsigned long long dropped = 0;
    for (int j = 0; j < SEQ; ++j) { rimg[j][0] = 0.0; rimg[j][1] = 0.0; tm[j] = 0.0; widx[j] = -1; rec_blur[j] = -1; }
    for (int k = 0; k < NTAB; ++k) { tab[k][0] = 0.0; tab[k][1] = 0.0; tab[k][2] = 1.0; }
    for (int i = 0; i < 16; ++i) ex[i] = 0.0;
    for (int i = 0; i < 9; ++i) in[i] = 0.0;
    int fps = 0, T = 0, tries = 0, len = 0;
    const bool ok = off >= 0 && nl >= 1 && nl <= a.n_times && off + nl <= a.n_rows;
    const int n = ok ? (int)nl : 0;
    const double* pos = a.rows + (size_t)(ok ? off : 0) * 9;
    const double* bt = a.times;
    if (ok) {
        // ---- frame rate: random.randint(20, 65) = 20 + getrandbits(6) redrawn until < 46
        fps = 50;
        if (train) {
            unsigned k = py.next() >> 26;
            while (k >= 46u) k = py.next() >> 26;
            fps = 20 + (int)k;
        }
        // ---- np.arange(t0, t_end, 1 / fps) and the nearest stored sample, ties to the left
        const double t0 = bt[0], t1 = bt[n - 1], step = 1.0 / fps;
        const double cnt = ceil((t1 - t0) / step);
        T = cnt > 0 ? (cnt < MAX_T ? (int)cnt : MAX_T) : 0;
        const double delta = (t0 + step) - t0;
        for (int i = 0; i < T; ++i) {
            const double t = i == 0 ? t0 : (i == 1 ? t0 + step : t0 + (double)i * delta);
            const int ins = lower_bound(bt, n, t);
            const int ir = ins < n - 1 ? ins : n - 1, il = ins - 1 < 0 ? 0 : (ins - 1 < n - 1 ? ins - 1 : n - 1);
            const double dl = fabs(bt[il] - t), dr = fabs(bt[ir] - t);
            near[i] = (short)(dr < dl ? ir : il);
            if (i < SEQ) tm[i] = t;
        }
        len = T < SEQ ? T : SEQ;
        // ---- camera
        if (train) {
            bool valid = false;
            while (!valid && tries < MAX_TRIES) {
                draw_camera(py, ex, in);
                bool inside = true;
                double x0 = 0, x1 = 0, y0 = 0, y1 = 0;
                for (int i = 0; i < T; ++i) {
                    double u, v;
                    project(ex, in, pos + 9 * near[i], &u, &v);
                    inside = inside && (u >= 0) && (u < IMG_W) && (v >= 0) && (v < IMG_H);
                    if (i == 0) { x0 = x1 = u; y0 = y1 = v; }
                    x0 = u < x0 ? u : x0; x1 = u > x1 ? u : x1; y0 = v < y0 ? v : y0; y1 = v > y1 ? v : y1;
                }
                valid = inside && T > 0 && (x1 - x0 > 0.15 * IMG_W || y1 - y0 > 0.15 * IMG_H);
                ++tries;
            }
        } else {
            const double* e = a.mext + (a.cam_per_traj ? (size_t)ti * 16 : 0);
            const double* m = a.mint + (a.cam_per_traj ? (size_t)ti * 9 : 0);
            for (int i = 0; i < 16; ++i) ex[i] = e[i];
            for (int i = 0; i < 9; ++i) in[i] = m[i];
        }
        // ---- crop / pad, keypoints, transform_resolution (numerically the identity here; the arithmetic is kept)
        const double sx = IMG_W / ORIG_W, sy = IMG_H / ORIG_H;
        for (int i = 0; i < len; ++i) {
            double u, v;
            project(ex, in, pos + 9 * near[i], &u, &v);
            rimg[i][0] = (u + 0.5) * sx - 0.5; rimg[i][1] = (v + 0.5) * sy - 0.5;
            widx[i] = near[i];
        }
        for (int k = 0; k < NTAB; ++k) {
            double p[3], u, v;
            table_point(k, p);
            project(ex, in, p, &u, &v);
            tab[k][0] = (u + 0.5) * sx - 0.5; tab[k][1] = (v + 0.5) * sy - 0.5;
        }
        in[0] = in[0] * sx; in[4] = in[4] * sy;
        in[2] = (in[2] + 0.5) * sx - 0.5; in[5] = (in[5] + 0.5) * sy - 0.5;
        const unsigned on = train ? a.enabled : (a.enabled & T_NORMALIZE);
        // ---- MotionBlur: a random stored sample inside [t - b (t - t_prev), t + b (t_next - t)], re-projected
        if ((on & T_BLUR) && a.blur_strength != 0) {
            const double bs = a.blur_strength;
            for (int i = 0; i < len; ++i) {
                const double tp = i > 0 ? tm[i - 1] : tm[i], tn = i < len - 1 ? tm[i + 1] : tm[i];
                const double b = tm[i] + bs * (tp - tm[i]), af = tm[i] + bs * (tn - tm[i]);
                const int lo = lower_bound(bt, n, b), hi = upper_bound(bt, n, af);
                if (hi <= lo) continue;                  // empty window (the reference's np.random.choice raises here)
                const int k = lo + np.below(hi - lo);
                double u, v;
                project(ex, in, pos + 9 * k, &u, &v);
                rimg[i][0] = u; rimg[i][1] = v;
                widx[i] = k; rec_blur[i] = k;
            }
        }
        // ---- RandomizeDetections: normal(0, std) on all 50 ball rows (padding included) and the 13 keypoints
        if (on & T_RANDOMIZE) {
            for (int j = 0; j < SEQ; ++j) {
                double g0, g1;
                np.gauss_pair(&g0, &g1);
                rimg[j][0] = rimg[j][0] + (0.0 + a.randomize_std * g0); rimg[j][1] = rimg[j][1] + (0.0 + a.randomize_std * g1);
            }
            for (int k = 0; k < NTAB; ++k) {
                double g0, g1;
                np.gauss_pair(&g0, &g1);
                tab[k][0] = tab[k][0] + (0.0 + a.randomize_std * g0); tab[k][1] = tab[k][1] + (0.0 + a.randomize_std * g1);
            }
        }
        const double hit = a.n_bounces[ti] > 0 ? a.bounces[(size_t)ti * 4] : -1.0;
        // ---- RandomStop: cut the sequence a random number (>= 4) of frames after the first bounce
        if (on & T_STOP) {
            if (!(np.dbl() > a.stop_prob) && hit > 0) {
                int hit_ind = 0;
                double best = fabs(tm[0] - hit);
                for (int j = 1; j < SEQ; ++j) { const double dj = fabs(tm[j] - hit); if (dj < best) { best = dj; hit_ind = j; } }
                if (len - hit_ind >= 4) {
                    const int new_len = hit_ind + 4 + np.below(len - hit_ind - 3);
                    for (int j = new_len; j < SEQ; ++j) {
                        rimg[j][0] = rimg[j][0] * 0; rimg[j][1] = rimg[j][1] * 0; tm[j] = tm[j] * 0;
                        if (widx[j] >= 0) widx[j] = -(widx[j] + 2);
                    }
                    len = new_len;
                }
            }
        }
        // ---- RandomDetection: a random image point instead of the ball / a keypoint
        if (on & T_RANDDET) {
            for (int i = 0; i < len; ++i)
                if (np.dbl() < a.randdet_prob) { rimg[i][0] = np.dbl() * IMG_W; rimg[i][1] = np.dbl() * IMG_H; }
            for (int k = 0; k < NTAB; ++k)
                if (np.dbl() < a.randdet_prob) { tab[k][0] = np.dbl() * IMG_W; tab[k][1] = np.dbl() * IMG_H; }
        }
        // ---- RandomMissing: drop frames, keep the order of the rest
        if (on & T_RANDMISS) {
            int cur = 0;
            for (int i = 0; i < len; ++i) {
                if (!(np.dbl() < a.randmiss_prob)) {
                    rimg[cur][0] = rimg[i][0]; rimg[cur][1] = rimg[i][1]; tm[cur] = tm[i]; widx[cur] = widx[i];
                    ++cur;
                } else {
                    dropped |= 1ull << i;
                }
            }
            for (int j = cur; j < SEQ; ++j) { rimg[j][0] = 0.0; rimg[j][1] = 0.0; tm[j] = 0.0; widx[j] = -1; }
            len = cur;
        }
        // ---- TableMissing: an undetected keypoint gets visibility 0 and random coordinates
        if (on & T_TABLEMISS) {
            for (int k = 0; k < NTAB; ++k)
                if (np.dbl() < a.tablemiss_prob) { tab[k][2] = 0.0; tab[k][0] = np.dbl() * IMG_W; tab[k][1] = np.dbl() * IMG_H; }
        }
        // ---- NormalizeImgCoords
        if (on & T_NORMALIZE) {
            for (int j = 0; j < SEQ; ++j) { rimg[j][0] = rimg[j][0] / IMG_W; rimg[j][1] = rimg[j][1] / IMG_H; }
            for (int k = 0; k < NTAB; ++k) { tab[k][0] = tab[k][0] / IMG_W; tab[k][1] = tab[k][1] / IMG_H; }
        }
    }
    // ---- output: the reference's torch.tensor(..., float32) casts, bounces[0:1]
    for (int j = 0; j < SEQ; ++j) {
        put(a, OUT_R_IMG, s * (2 * SEQ) + 2 * j, rimg[j][0]);
        put(a, OUT_R_IMG, s * (2 * SEQ) + 2 * j + 1, rimg[j][1]);
        put(a, OUT_MASK, s * SEQ + j, j < len ? 1.0 : 0.0);
        put(a, OUT_TIMES, s * SEQ + j, tm[j]);
        const int w = widx[j];
        for (int c = 0; c < 3; ++c) {
            const double v = w >= 0 ? pos[9 * w + c] : (w == -1 ? 0.0 : pos[9 * (-(w + 2)) + c] * 0);
            put(a, OUT_R_WORLD, s * (3 * SEQ) + 3 * j + c, v);
        }
    }
    for (int k = 0; k < NTAB; ++k)
        for (int c = 0; c < 3; ++c) put(a, OUT_TABLE_IMG, s * (3 * NTAB) + 3 * k + c, tab[k][c]);
    for (int c = 0; c < 3; ++c) put(a, OUT_ROTATION, s * 3 + c, ok ? pos[6 + c] : 0.0);
    put(a, OUT_BOUNCES, s, ok ? (a.n_bounces[ti] > 0 ? a.bounces[(size_t)ti * 4] : -1.0) : 0.0);
    for (int i = 0; i < 9; ++i) put(a, OUT_MINT, s * 9 + i, in[i]);
    for (int i = 0; i < 16; ++i) put(a, OUT_MEXT, s * 16 + i, ex[i]);
    diag[0] = ok ? fps : -1; diag[1] = T; diag[2] = tries; diag[3] = (train && ok && tries < MAX_TRIES) ? 1 : 0;
    if (a.record) {
        int* r = a.record + (size_t)RECORD_INTS * s;
        for (int j = 0; j < SEQ; ++j) {
            r[j] = (ok && j < (T < SEQ ? T : SEQ)) ? near[j] : -1;
            r[SEQ + j] = rec_blur[j];
            r[2 * SEQ + j] = (int)((dropped >> j) & 1ull);
        }
    }
}

}  // namespace ds
}  // namespace ttup
