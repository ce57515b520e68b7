// Host build of csrc/dataset_core.h for CPU tests (g++ -O2 -ffp-contract=off -shared -fPIC): the code that runs one lane per
// sample in the HIP kernels, here one sample after the other with the two MT19937 states on the stack.
#include <string.h>
#include "../../upliftingtabletennis_amd/csrc/dataset_core.h"
using namespace ttup::ds;
extern "C" void ttup_host_dataset_draws(long long seed, int which, int count, unsigned* out) {
    unsigned st[624];
    MT m = {st, 1, 0};
    if (which) init_genrand(m, (unsigned)seed); else init_by_array(m, (unsigned long long)seed);
    for (int k = 0; k < count; ++k) out[k] = m.next();
}
// out64: nine arrays stacked over n as in ttup_dataset_build; strengths[6]
extern "C" void ttup_host_dataset_build(const double* rows, const long long* offsets, long long n_rows, int n_traj, const double* bounces,
                                        const int* n_bounces, const double* times, int n_times, const double* mext, const double* mint,
                                        const long long* traj_index, const long long* seeds, int n, int mode, const double* strengths,
                                        unsigned enabled, double* const* out64, int* diag, int* record) {
    Args a;
    memset(&a, 0, sizeof a);
    a.rows = rows; a.offsets = offsets; a.n_rows = n_rows; a.bounces = bounces; a.n_bounces = n_bounces; a.times = times; a.n_times = n_times;
    a.mext = mext; a.mint = mint; a.cam_per_traj = 0; a.n_traj = n_traj; a.mode = mode; a.enabled = enabled;
    a.blur_strength = strengths[0]; a.randomize_std = strengths[1]; a.stop_prob = strengths[2]; a.randdet_prob = strengths[3];
    a.randmiss_prob = strengths[4]; a.tablemiss_prob = strengths[5];
    for (int k = 0; k < N_OUT; ++k) a.out64[k] = out64[k];
    a.diag = diag; a.record = record;
    for (int s = 0; s < n; ++s) {
        unsigned st_py[624], st_np[624];
        MT py = {st_py, 1, 0}, np = {st_np, 1, 0};
        init_by_array(py, (unsigned long long)seeds[s]);
        init_genrand(np, (unsigned)seeds[s]);
        build_sample(a, (size_t)s, traj_index[s], py, np);
    }
}
