// Uplift training samples from generated trajectories (reference uplifting/data.py::TableTennisDataset.__getitem__ and the train
// transforms of uplifting/transformations.py), fp64; the per-sample arithmetic is dataset_core.h, the two streams mt19937.h.
//   seed_kernel    one lane per sample: both MT19937 states (CPython random.seed(s), np.random.seed(s)) into the workspace
//   build_kernel   one lane per sample: frame rate, resampling, camera rejection loop, transforms, the nine outputs
//   draws_kernel   tests: the next `count` raw words of one of the two streams
// Mapping: a sample is one sequential chain (every draw's place in its stream depends on the rejections before it: the camera
// loop, the masked-rejection `choice` / `randint`, the polar method), so a sample is a lane and the batch supplies the parallelism.
// Workspace: [2][624][n] state words, word-major -- the lanes of a wave read and write neighbouring words as long as their
// stream positions agree, and a state element is renewed when its word is drawn (mt19937.h), never 624 at a time.
// The per-sample arrays (50 image points, 50 times, 13 keypoints, <= 128 frame indices) are private to the lane.
#include "common.h"
#include "dataset_core.h"

using namespace ttup;

namespace {

__global__ void seed_kernel(const long long* seeds, int n, unsigned* ws) {
    const int lane = ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (lane >= n) return;
    const unsigned long long s = (unsigned long long)seeds[lane];          // validated on the host: 0 <= s < 2^32
    ds::MT py = {ws + lane, (size_t)n, 0}, np = {ws + (size_t)624 * n + lane, (size_t)n, 0};
    ds::init_by_array(py, s);
    ds::init_genrand(np, (unsigned)s);
}

__global__ void build_kernel(ds::Args a, const long long* traj_index, int n, unsigned* ws) {
    const int lane = ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (lane >= n) return;
    ds::MT py = {ws + lane, (size_t)n, 0}, np = {ws + (size_t)624 * n + lane, (size_t)n, 0};
    ds::build_sample(a, (size_t)lane, traj_index[lane], py, np);
}

__global__ void draws_kernel(unsigned* ws, int n, int which, int count, unsigned* out) {
    const int lane = ttup_bid_x() * ttup_bdim_x() + ttup_tid_x();
    if (lane >= n) return;
    ds::MT m = {ws + (size_t)(which ? 624 : 0) * n + lane, (size_t)n, 0};
    for (int k = 0; k < count; ++k) out[(size_t)lane * count + k] = m.next();
}

constexpr size_t STATE_BYTES = 2 * 624 * sizeof(unsigned);

inline bool prob_ok(double p) { return p >= 0.0 && p <= 1.0; }

}  // namespace

extern "C" size_t ttup_dataset_workspace_bytes(int n) {
    return n <= 0 ? 0 : (size_t)n * (STATE_BYTES + 2 * sizeof(long long));
}

extern "C" int ttup_dataset_seed(const int64_t* seeds_host, int n, void* workspace, size_t workspace_bytes, void* stream) {
    TTUP_REQUIRE(n >= 0, TTUP_EINVAL, "ttup_dataset_seed: negative sample count %d", n);
    if (n == 0) return TTUP_OK;
    TTUP_REQUIRE(seeds_host && workspace, TTUP_EINVAL, "ttup_dataset_seed: null pointer");
    TTUP_REQUIRE(workspace_bytes >= ttup_dataset_workspace_bytes(n), TTUP_EINVAL, "ttup_dataset_seed: workspace too small (%zu < %zu bytes)",
                 workspace_bytes, ttup_dataset_workspace_bytes(n));
    for (int i = 0; i < n; ++i)
        TTUP_REQUIRE(seeds_host[i] >= 0 && seeds_host[i] <= 0xffffffffll, TTUP_EINVAL,
                     "ttup_dataset_seed: seed %lld of sample %d is outside [0, 2**32 - 1] (np.random.seed refuses it)", (long long)seeds_host[i], i);
    hipStream_t st = (hipStream_t)stream;
    long long* seeds_dev = (long long*)((char*)workspace + (size_t)n * STATE_BYTES);
    TTUP_HIP_CHECK(hipMemcpyAsync(seeds_dev, seeds_host, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, st));
    TTUP_HIP_CHECK(hipStreamSynchronize(st));          // the caller's array may go away after the call
    hipLaunchKernelGGL(seed_kernel, dim3(cdiv(n, 64)), dim3(64), 0, st, seeds_dev, n, (unsigned*)workspace);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

extern "C" int ttup_dataset_draws(void* workspace, size_t workspace_bytes, int n, int which, int count, uint32_t* out_dev, void* stream) {
    TTUP_REQUIRE(workspace && out_dev, TTUP_EINVAL, "ttup_dataset_draws: null pointer");
    TTUP_REQUIRE(n > 0 && count > 0 && (which == 0 || which == 1), TTUP_EINVAL, "ttup_dataset_draws: bad n %d / count %d / stream %d", n, count, which);
    TTUP_REQUIRE(workspace_bytes >= ttup_dataset_workspace_bytes(n), TTUP_EINVAL, "ttup_dataset_draws: workspace too small");
    hipLaunchKernelGGL(draws_kernel, dim3(cdiv(n, 64)), dim3(64), 0, (hipStream_t)stream, (unsigned*)workspace, n, which, count, out_dev);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}

extern "C" int ttup_dataset_build(const double* rows_dev, const int64_t* offsets_dev, int64_t n_rows, int n_traj, const double* bounces_dev,
                                  const int* n_bounces_dev, const double* times_dev, int n_times, const double* mext_dev, const double* mint_dev,
                                  int cam_per_traj, const int64_t* traj_index_host, int n, int mode, const double* strengths_host,
                                  unsigned transform_mask, void* const* out32_host, void* const* out64_host, int* diag_dev, int* record_dev,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    TTUP_REQUIRE(n >= 0, TTUP_EINVAL, "ttup_dataset_build: negative sample count %d", n);
    TTUP_REQUIRE(mode == 0 || mode == 1, TTUP_EINVAL, "ttup_dataset_build: bad mode %d (0 train, 1 test)", mode);
    TTUP_REQUIRE(rows_dev && offsets_dev && bounces_dev && n_bounces_dev && times_dev && diag_dev && strengths_host && (out32_host || out64_host),
                 TTUP_EINVAL, "ttup_dataset_build: null pointer");
    TTUP_REQUIRE(mode == 0 || (mext_dev && mint_dev), TTUP_EINVAL, "ttup_dataset_build: 'test' mode needs the stored camera (null pointer)");
    TTUP_REQUIRE(n_traj > 0 && n_rows > 0 && n_times > 0, TTUP_EINVAL, "ttup_dataset_build: empty trajectory set");
    TTUP_REQUIRE((transform_mask >> 7) == 0, TTUP_EINVAL, "ttup_dataset_build: transform mask 0x%x has bits beyond the seven transforms", transform_mask);
    const double* s = strengths_host;
    TTUP_REQUIRE(s[0] == 0.0 || (s[0] >= 0.1 && s[0] < 0.5), TTUP_EINVAL, "ttup_dataset_build: blur_strength %g should be in [0.1, 0.5) or 0", s[0]);
    TTUP_REQUIRE(s[1] >= 0.0, TTUP_EINVAL, "ttup_dataset_build: negative randomize_std %g", s[1]);
    TTUP_REQUIRE(prob_ok(s[2]) && prob_ok(s[3]) && prob_ok(s[4]) && prob_ok(s[5]), TTUP_EINVAL,
                 "ttup_dataset_build: probability outside [0, 1] (stop %g, randdet %g, randmiss %g, tablemiss %g)", s[2], s[3], s[4], s[5]);
    if (n == 0) return TTUP_OK;
    TTUP_REQUIRE(traj_index_host && workspace, TTUP_EINVAL, "ttup_dataset_build: null pointer");
    TTUP_REQUIRE(workspace_bytes >= ttup_dataset_workspace_bytes(n), TTUP_EINVAL, "ttup_dataset_build: workspace too small (%zu < %zu bytes)",
                 workspace_bytes, ttup_dataset_workspace_bytes(n));
    for (int i = 0; i < n; ++i)
        TTUP_REQUIRE(traj_index_host[i] >= 0 && traj_index_host[i] < n_traj, TTUP_EINVAL,
                     "ttup_dataset_build: trajectory index %lld of sample %d out of range [0, %d)", (long long)traj_index_host[i], i, n_traj);
    ds::Args a;
    a.rows = rows_dev; a.offsets = (const long long*)offsets_dev; a.n_rows = n_rows; a.bounces = bounces_dev; a.n_bounces = n_bounces_dev;
    a.times = times_dev; a.n_times = n_times; a.mext = mext_dev; a.mint = mint_dev; a.cam_per_traj = cam_per_traj; a.n_traj = n_traj;
    a.mode = mode; a.enabled = transform_mask;
    a.blur_strength = s[0]; a.randomize_std = s[1]; a.stop_prob = s[2]; a.randdet_prob = s[3]; a.randmiss_prob = s[4]; a.tablemiss_prob = s[5];
    for (int k = 0; k < ds::N_OUT; ++k) {
        a.out32[k] = out32_host ? (float*)out32_host[k] : nullptr;
        a.out64[k] = out64_host ? (double*)out64_host[k] : nullptr;
        TTUP_REQUIRE((!out32_host || a.out32[k]) && (!out64_host || a.out64[k]), TTUP_EINVAL, "ttup_dataset_build: output %d is null", k);
    }
    a.diag = diag_dev; a.record = record_dev;
    hipStream_t st = (hipStream_t)stream;
    long long* index_dev = (long long*)((char*)workspace + (size_t)n * STATE_BYTES) + n;
    TTUP_HIP_CHECK(hipMemcpyAsync(index_dev, traj_index_host, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, st));
    TTUP_HIP_CHECK(hipStreamSynchronize(st));
    hipLaunchKernelGGL(build_kernel, dim3(cdiv(n, 64)), dim3(64), 0, st, a, index_dev, n, (unsigned*)workspace);
    TTUP_LAUNCH_CHECK();
    return TTUP_OK;
}
