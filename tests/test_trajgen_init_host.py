"""f2: the generator's seeding on the CPU -- the host build of csrc/trajgen_init.h (CPython's random.Random(seed) from
csrc/mt19937.h and the nine draws of `_init_simulation`; tests/helpers/host_trajgen_init.cpp) against
oracle.trajgen_ref.init_state, which draws from Python's own `random`.  The seeds take both key lengths of init_by_array
(below and from 2**32) and both signs; the golden `init_seeds` of tests/test_trajgen_gpu.py hold no negative one."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import trajgen_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5, 2 ** 63 - 1, -7, -(2 ** 32 + 7)]


@pytest.fixture(scope='module')
def host_init(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('hosttrajgen') / 'host_trajgen_init.so')
    subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-Wno-unknown-pragmas', '-o', so,
                           os.path.join(ROOT, 'tests', 'helpers', 'host_trajgen_init.cpp')])
    return ctypes.CDLL(so)


@pytest.mark.parametrize('direction', T.DIRECTIONS)
@pytest.mark.parametrize('mode', T.MODES)
def test_host_build_draws_the_initial_state_of_the_reference(host_init, mode, direction):
    """Positions come from products and sums of the draws alone: bit for bit.  Velocity and spin go through sin / cos / atan2
    of two libms: the bound of tests/test_trajgen_gpu.py, <= 1e-13 relative to max |ref|."""
    got = np.zeros((len(SEEDS), 9))
    for k, seed in enumerate(SEEDS):
        host_init.ttup_host_trajgen_init(ctypes.c_longlong(seed), T.MODES.index(mode), T.DIRECTIONS.index(direction),
                                         got[k].ctypes.data_as(ctypes.c_void_p))
    ref = np.array([np.concatenate(T.init_state(seed, mode, direction)) for seed in SEEDS])
    assert np.array_equal(got[:, :3], ref[:, :3])
    dev = np.abs(got[:, 3:] - ref[:, 3:]).max() / np.abs(ref[:, 3:]).max()
    print('\n%s %s: velocity / spin deviation %.3e of max |ref|' % (mode, direction, dev))
    assert dev <= 1e-13
