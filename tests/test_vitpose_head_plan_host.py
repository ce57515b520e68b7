"""The ViTPose head's device-free decisions (csrc/vitpose_head_plan.h, and the gather index of csrc/gemm_modes.h) on the CPU, through
the stand-alone program tests/helpers/host_vitpose_head_plan.cpp built with AddressSanitizer and UndefinedBehaviorSanitizer.  The
program runs as a child process (nothing of it is loaded into python) and carries its sanitizer runtimes itself (linked
statically); every run must end with status 0 and an empty stderr, i.e. without a sanitizer report.

Taps: every tap of the reference's 4x4 kernel belongs to exactly one (phase, 2x2 tap), by weights.vitpose_fold_head's rule, and the
pack to the forward's phase matrices, the pack to the backward's (cin, 16 cout) matrix and the un-pack are permutations and
inverses.  Gather: the backward's one operand against a brute-force scatter of the transposed convolution.  Slices: the counts and
last slices of the case table's row counts.  Workspace: alignment, overlap, sizing.  Refusals: the TTUP_EINVAL list."""
import os
import subprocess

import numpy as np
import pytest

from helpers import vitpose_head_cases as cases
from upliftingtabletennis_amd import weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('hostheadplan') / 'host_vitpose_head_plan')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-static-libubsan', '-o', exe,
                           os.path.join(ROOT, 'tests', 'helpers', 'host_vitpose_head_plan.cpp')])
    return exe


def run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == '', (args, r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def _no_failures(lines, n_cases):
    assert not [l for l in lines if l.startswith('FAIL')], lines[:20]
    assert lines[-2:] == ['cases %d' % n_cases, 'failures 0'], lines[-3:]


def test_tap_bijection_and_pack_unpack_are_inverses(prog):
    """16 taps + 4 weight shapes ((384, 256), (256, 256), (3, 5), (1, 1))"""
    _no_failures(run(prog, 'taps'), 20)


def test_phase_matrices_are_vitpose_fold_head_with_scale_one():
    """The plan's rule is checked against the fold's formula inside the program; here the fold itself, with BN at identity, is held to
    the same formula from the Python side: phase matrix [2py+px][co][(2dy+dx) cin + ci] = w[ci, co, 3-py-2dy, 3-px-2dx]."""
    rng = np.random.default_rng(0)
    sd = {}
    for i, cin in ((0, 6), (3, 4)):
        h = 'model.keypoint_head.deconv_layers.'
        sd[h + '%d.weight' % i] = rng.standard_normal((cin, 4, 4, 4)).astype(np.float32)
        sd[h + '%d.weight' % (i + 1)] = np.full(4, np.sqrt(1.0 + weights.BN_EPS))
        sd[h + '%d.bias' % (i + 1)] = np.zeros(4)
        sd[h + '%d.running_mean' % (i + 1)] = np.zeros(4)
        sd[h + '%d.running_var' % (i + 1)] = np.ones(4)
    for (wp, b), i in zip(weights.vitpose_fold_head(sd), (0, 3)):
        w = sd['model.keypoint_head.deconv_layers.%d.weight' % i]
        cin = w.shape[0]
        assert not b.any()
        for ph in range(4):
            for t in range(4):
                ky, kx = 3 - (ph >> 1) - 2 * (t >> 1), 3 - (ph & 1) - 2 * (t & 1)
                np.testing.assert_allclose(wp[ph][:, t * cin:(t + 1) * cin], w[:, :, ky, kx].T, rtol=1e-6)


def test_gather_index_is_the_transposed_convolutions_scatter(prog):
    """batch {1, 2} x grids 1x1 .. 6x6"""
    _no_failures(run(prog, 'gather'), 72)


def test_slices_of_the_case_table(prog):
    """The table's copy of SLICE_TOKENS is the plan's, and the table reaches one slice exactly, whole slices only and a last slice of
    one token -- one row of the dW1 product's k range, 4 and 16 rows at the two levels above."""
    names = list(cases.CASES)
    out = run(prog, 'slices', *[cases.tokens(n) for n in names])
    consts = out[-1].split()
    assert consts[0] == 'slice_tokens' and int(consts[1]) == cases.SLICE_TOKENS
    s = cases.SLICE_TOKENS
    assert [int(v) for v in consts[5:8]] == [s, 4 * s, 16 * s]
    got = {n: [int(v) for v in l.split()] for n, l in zip(names, out)}
    for n, (t, ns, l0, l1, l2) in got.items():
        assert t == cases.tokens(n) and ns == -(-t // s) and (l0, l1, l2) == ((t - 1) % s + 1, 4 * ((t - 1) % s + 1), 16 * ((t - 1) % s + 1)), n
    assert got['one_slice'][1:3] == [1, s]
    assert got['whole_slices'][1:3] == [2, s]
    assert got['last_of_one'][1:] == [2, 1, 4, 16]
    assert all(got[n][1] == 1 and got[n][2] < s for n in names if n.startswith('g'))          # the small grids: one partial slice


def test_workspace_is_aligned_disjoint_and_large_enough(prog):
    """max_rows {1, 2, 35, 64, 65, 511, 512, 513, 1024, 1025, 23040, 2^22} x out_ch {1, 13, 16}"""
    _no_failures(run(prog, 'workspace'), 36)


def test_refusals(prog):
    _no_failures(run(prog, 'refusals'), 6)
