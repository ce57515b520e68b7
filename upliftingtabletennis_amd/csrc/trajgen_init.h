// The nine uniform draws of the reference's `_init_simulation` (syntheticdataset/mujocosimulation.py:54-109) from a seeded
// CPython stream -> initial position, velocity and spin of one trajectory.  The same source compiles for gfx950 (trajgen.hip's
// init_kernel, one lane per seed) and for the host (g++, test infrastructure only: tests/helpers/host_trajgen_init.cpp).
#pragma once
#include <math.h>
#include "mt19937.h"
#include "scene.h"

namespace ttup {
namespace trajgen {

// mode: index into OOB_DEFINITIONS (3..5 = first_*); direction 0 = left_to_right; m: 624 words of state storage, seeded here as
// random.Random(seed) seeds (with abs(seed)); out = r, v, w
TTUP_DS_HD inline void init_state(long long seed, int mode, int direction, ds::MT& m, double out[9]) {
#pragma clang fp contract(off)      // a + (b - a) * random() and the angles must round like CPython's separate operations
    using namespace scene;
    ds::init_by_array(m, seed < 0 ? 0ull - (unsigned long long)seed : (unsigned long long)seed);
    const bool first = mode >= 3;                   // first_good, first_short, first_long
    const bool l2r = direction == 0;
    const double sign_x = l2r ? 1.0 : -1.0;
    double* r = out;
    if (first) {
        r[0] = m.uniform(1.0, 2.5) * sign_x; r[1] = m.uniform(-1.5, 1.5); r[2] = m.uniform(0.8, 1.6);
    } else {
        r[0] = m.uniform(0.1, 4.0) * sign_x; r[1] = m.uniform(-2.0, 2.0);
        r[2] = (fabs(r[0]) < TABLE_LENGTH / 2 && fabs(r[1]) < TABLE_WIDTH / 2) ? m.uniform(0.8, 1.8) : m.uniform(0.5, 1.8);
    }
    double cx, cy;
    if (first) { cy = r[1] > 0 ? TABLE_WIDTH / 2 : -TABLE_WIDTH / 2; cx = l2r ? TABLE_LENGTH / 2 : -TABLE_LENGTH / 2; }
    else { cy = 0.0; cx = l2r ? -TABLE_LENGTH / 2 : TABLE_LENGTH / 2; }
    const double r2d = 180.0 / PI, d2r = PI / 180.0;
    const double base_phi = 180.0 + atan2(r[1] - cy, r[0] - cx) * r2d;
    const double base_theta = 90.0 - atan2(r[2] - TABLE_HEIGHT, fabs(r[0] - cx)) * r2d;
    double min_theta, max_theta;
    if (r[2] < TABLE_HEIGHT) { min_theta = fmax(90.0, base_theta - 25.0); max_theta = fmin(170.0, base_theta + 60.0); }
    else { min_theta = fmax(10.0, base_theta - 25.0); max_theta = fmin(150.0, base_theta + 60.0); }
    double speed = m.uniform(3.0, 30.0);
    double phi = m.uniform((base_phi - 60.0) * d2r, (base_phi + 60.0) * d2r);
    double theta = m.uniform(min_theta * d2r, max_theta * d2r);
    out[3] = speed * sin(theta) * cos(phi); out[4] = speed * sin(theta) * sin(phi); out[5] = speed * cos(theta);
    speed = m.uniform(0.0, 500.0);
    phi = m.uniform(0.0, 2.0 * PI);
    theta = m.uniform(0.0, PI);
    out[6] = speed * sin(theta) * cos(phi); out[7] = speed * sin(theta) * sin(phi); out[8] = speed * cos(theta);
}

}  // namespace trajgen
}  // namespace ttup
