// The scene every fp64 unit works in: table and net geometry, the 13 table keypoints, the ball and the air around it; one copy
// for the generator (trajgen.hip, trajgen_init.h), the dataset (dataset_core.h), the calibration (calib.hip) and the ODE fit
// (odefit.hip).  Plain constants that also compile for the host (g++, tests/helpers/), and the flight kernels' device-only V3.
#pragma once
#include <math.h>

namespace ttup {
namespace scene {

constexpr double PI = 3.141592653589793238462643383279502884;
// syntheticdataset/helper.py:14-40 [m]; the net's posts stand NET_POST_OFFSET outside the table, its top NET_HEIGHT above it
constexpr double TABLE_LENGTH = 2.74, TABLE_WIDTH = 1.525, TABLE_HEIGHT = 0.76;
constexpr double NET_POST_OFFSET = 0.1525, NET_HEIGHT = 0.1525;
// ball and air of the MuJoCo XML (helper.py:79-117): radius [m], mass [kg], air density, viscosity, gravity, fluidcoef blunt drag / Magnus
constexpr double R_BALL = 0.02, M_BALL = 0.0027, RHO = 1.225, MU_AIR = 0.000018, GRAV = 9.81;
constexpr double C_BLUNT = 0.235, C_MAGNUS = 1.0;
// the 13 table keypoints in world coordinates (uplifting/helper.py:36-50): the table's corners and the ends of its net line, the
// net posts' feet (6, 7), the table centre, the posts' tops (9, 10), the two end-line centres
constexpr int N_KEYPOINTS = 13;
constexpr double HALF_LENGTH = TABLE_LENGTH / 2, HALF_WIDTH = TABLE_WIDTH / 2, POST_Y = TABLE_WIDTH / 2 + NET_POST_OFFSET;
constexpr double TABLE_PTS[N_KEYPOINTS][3] = {
    {-HALF_LENGTH, HALF_WIDTH, TABLE_HEIGHT}, {-HALF_LENGTH, -HALF_WIDTH, TABLE_HEIGHT}, {0.0, HALF_WIDTH, TABLE_HEIGHT}, {0.0, -HALF_WIDTH, TABLE_HEIGHT},
    {HALF_LENGTH, HALF_WIDTH, TABLE_HEIGHT}, {HALF_LENGTH, -HALF_WIDTH, TABLE_HEIGHT}, {0.0, POST_Y, TABLE_HEIGHT}, {0.0, -POST_Y, TABLE_HEIGHT},
    {0.0, 0.0, TABLE_HEIGHT}, {0.0, POST_Y, TABLE_HEIGHT + NET_HEIGHT}, {0.0, -POST_Y, TABLE_HEIGHT + NET_HEIGHT},
    {-HALF_LENGTH, 0.0, TABLE_HEIGHT}, {HALF_LENGTH, 0.0, TABLE_HEIGHT}};

#if defined(__HIPCC__)
struct V3 { double x, y, z; };
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double norm(V3 a) { return sqrt(dot(a, a)); }
#endif

}  // namespace scene
}  // namespace ttup
