// Host build of csrc/trajgen_init.h for CPU tests (g++ -O2 -ffp-contract=off -shared -fPIC): what init_kernel of csrc/trajgen.hip
// runs one lane per seed, here one seed per call with the MT19937 state on the stack.
#include "../../upliftingtabletennis_amd/csrc/trajgen_init.h"
extern "C" void ttup_host_trajgen_init(long long seed, int mode, int direction, double* out9) {
    unsigned st[624];
    ttup::ds::MT m = {st, 1, 0};
    ttup::trajgen::init_state(seed, mode, direction, m, out9);
}
