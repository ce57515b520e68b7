// MT19937 as CPython's `random` (random.seed(int) = init_by_array) and numpy's legacy global stream (np.random.seed =
// init_genrand) use it; the one copy for dataset_core.h, trajgen_init.h and the host builds of both under tests/helpers/.
// The 624-word state lives in caller memory with a stride between words (device: word-major over the lanes of a launch, so that
// the lanes of a wave touch neighbouring addresses; host: stride 1).  A state element is renewed at the moment its word is drawn:
// that is the usual whole-state regeneration done one element at a time (it walks the state in this very order), so no draw ever
// waits for 624 updates.
// No fma contraction in `dbl`, `uniform`, `gauss_pair`: they must round like CPython's and numpy's separate operations.  The
// pragma stands inside those bodies, not at file scope, so that a unit that includes this header keeps its own setting.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define TTUP_DS_HD __host__ __device__
#else
#define TTUP_DS_HD
#endif

namespace ttup {
namespace ds {

struct MT {
    unsigned* s;
    size_t stride;
    int pos;
    TTUP_DS_HD unsigned& at(int i) { return s[(size_t)i * stride]; }
    TTUP_DS_HD unsigned next() {
        const int i = pos, i1 = i + 1 < 624 ? i + 1 : 0, im = i + 397 < 624 ? i + 397 : i + 397 - 624;
        const unsigned y = (at(i) & 0x80000000u) | (at(i1) & 0x7fffffffu);
        unsigned v = at(im) ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        at(i) = v;
        pos = i1;
        v ^= v >> 11; v ^= (v << 7) & 0x9d2c5680u; v ^= (v << 15) & 0xefc60000u; v ^= v >> 18;
        return v;
    }
    // genrand_res53: CPython's random() and numpy's legacy random_sample()
    TTUP_DS_HD double dbl() {
#pragma clang fp contract(off)
        const unsigned a = next() >> 5, b = next() >> 6;
        return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
    }
    TTUP_DS_HD double uniform(double lo, double hi) {
#pragma clang fp contract(off)
        return lo + (hi - lo) * dbl();
    }
    // numpy legacy randint(0, count): masked rejection on single words; no word is drawn for count == 1
    TTUP_DS_HD int below(int count) {
        const unsigned rng = (unsigned)(count - 1);
        if (rng == 0) return 0;
        unsigned mask = rng;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        unsigned v = next() & mask;
        while (v > rng) v = next() & mask;
        return (int)v;
    }
    // legacy_gauss: polar method; numpy returns f * x2 first and keeps f * x1 for the next call
    TTUP_DS_HD void gauss_pair(double* first, double* second) {
#pragma clang fp contract(off)
        double x1, x2, r2;
        do {
            x1 = 2.0 * dbl() - 1.0;
            x2 = 2.0 * dbl() - 1.0;
            r2 = x1 * x1 + x2 * x2;
        } while (r2 >= 1.0 || r2 == 0.0);
        const double f = sqrt(-2.0 * log(r2) / r2);
        *first = f * x2;
        *second = f * x1;
    }
};

TTUP_DS_HD inline void init_genrand(MT& m, unsigned seed) {
    unsigned prev = seed;
    m.at(0) = prev;
    for (int i = 1; i < 624; ++i) {
        prev = 1812433253u * (prev ^ (prev >> 30)) + (unsigned)i;
        m.at(i) = prev;
    }
    m.pos = 0;
}

// CPython random.seed(int): init_by_array over the 32-bit little-endian words of abs(seed) (one word below 2^32, else two)
TTUP_DS_HD inline void init_by_array(MT& m, unsigned long long a) {
    init_genrand(m, 19650218u);
    const unsigned key[2] = {(unsigned)(a & 0xffffffffu), (unsigned)(a >> 32)};
    const int keylen = key[1] ? 2 : 1;
    int i = 1, j = 0;
    for (int k = 0; k < 624; ++k) {
        const unsigned p = m.at(i - 1);
        m.at(i) = (m.at(i) ^ ((p ^ (p >> 30)) * 1664525u)) + key[j] + (unsigned)j;
        ++i; ++j;
        if (i >= 624) { m.at(0) = m.at(623); i = 1; }
        if (j >= keylen) j = 0;
    }
    for (int k = 0; k < 623; ++k) {
        const unsigned p = m.at(i - 1);
        m.at(i) = (m.at(i) ^ ((p ^ (p >> 30)) * 1566083941u)) - (unsigned)i;
        ++i;
        if (i >= 624) { m.at(0) = m.at(623); i = 1; }
    }
    m.at(0) = 0x80000000u;
    m.pos = 0;
}

}  // namespace ds
}  // namespace ttup
