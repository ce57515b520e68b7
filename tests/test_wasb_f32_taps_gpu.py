"""The fp32 CNN tap by tap, teacher-forced, against the float64 oracle with fp32 storage (oracle/wasb_bf16_ref.py,
Weights(rounding='f32')) at the tile, border, instance and persistent-trip edges of conv_x3_kernel (cases, launch arithmetic and
bounds: tests/helpers/wasb_f32_cases.py; the CPU half is tests/test_wasb_f32_oracle.py).

Per case the fp32 net runs once (batch <= micro-batch, so the taps hold the whole batch).  Every segment of the oracle then starts
from the DEVICE's input taps -- S0 from the oracle's own input, which puts the layout and pre-processing kernels inside the
comparison -- and every element of every stored tap and of the heatmap is compared on the checked images: a difference is the
summation order of at most six layers.  How much of that is legitimate is measured by the oracle's fp32 variant on the same inputs
(the spread); the device may reach M_MAX x its max and M_MEAN x its mean (M_MEAN_NOISE on the noise-weight cases) and never more
than 1e-5 of a tap's scale: constants per kernel choice, measured ratios and where the excess over the spread sits are written
beside them in the helper and in DESIGN 3.  The cross-check kernels (TTUP_F32_EXACT, TTUP_F32_DIRECT) run in child processes, one at a time, and meet the same comparison."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import wasb_f32_cases as F

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def _synthetic_weights(monkeypatch):
    monkeypatch.setenv('TTUP_SYNTHETIC_WEIGHTS', '1')
    monkeypatch.delenv('TTUP_WEIGHTS', raising=False)
    for env in F.KERNEL_ENV.values():          # the default kernels here; the cross-checks set their switch for the child alone
        if env:
            monkeypatch.delenv(env, raising=False)


def _assert_checked(case, taps, heat, idx, kernels='x3'):
    assert set(taps) == set(F.TAPS)
    assert all(torch.isfinite(t).all() for t in taps.values()) and torch.isfinite(heat).all()
    failures, compared = F.check_taps(case, taps, heat, idx, kernels)
    assert compared == set(F.TAPS) | {'heat'}, compared
    assert not failures, failures


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('case', F.CASES, ids=lambda c: c.id)
def test_fp32_taps_match_the_float64_oracle_teacher_forced(case):
    (taps, heat, idx), (taps2, heat2, idx2) = F.device_run(case)
    _assert_checked(case, taps, heat, idx)
    # a second run of the same handle returns the same bits (the persistent kernels' work split is fixed by the launch)
    assert _same_bits(heat, heat2) and torch.equal(idx, idx2)
    assert [k for k in F.TAPS if not _same_bits(taps[k], taps2[k])] == []


def test_last_image_alone_equals_its_values_inside_the_batch():
    """The trip case's last image -- second and later trips of every launch that has them -- run alone through a max_batch=1 handle,
    where the same tiles are first-trip work of other workgroups: every tap and the heatmap bit-equal (csrc/conv_x3.hip: the k order
    of an output pixel depends neither on the tile nor on the image)."""
    case = F.BY_ID['1032x8_b8']
    last = case.batch - 1
    taps, heat, idx = F.device_run(case)[0]
    taps1, heat1, idx1 = F.device_run(case, batch=1, first=last)[0]
    assert [k for k in F.TAPS if not _same_bits(taps[k][last:], taps1[k])] == []
    assert _same_bits(heat[last:], heat1) and torch.equal(idx[last:], idx1)


@pytest.mark.parametrize('kernels,case', F.CROSS_CASES, ids=lambda v: v if isinstance(v, str) else v.id)
def test_cross_check_kernels_match_the_float64_oracle(kernels, case, tmp_path):
    """conv_f32_mfma_kernel (TTUP_F32_EXACT=1) and conv_direct_f32_kernel (TTUP_F32_DIRECT=1) against the same oracle with their own
    constants.  csrc/conv.hip reads the switches once per process, so each run is a fresh child that writes its taps to a file."""
    out = str(tmp_path / 'taps.npz')
    code = 'import sys; sys.path[:0] = [%r, %r]; from helpers import wasb_f32_cases as F; F.child_main(sys.argv[1], sys.argv[2])' % (os.path.dirname(TESTS), TESTS)
    env = dict(os.environ)
    env[F.KERNEL_ENV[kernels]] = '1'
    subprocess.run([sys.executable, '-c', code, case.id, out], check=True, env=env, timeout=300)
    got = np.load(out)
    taps = {k: torch.from_numpy(got[k]) for k in F.TAPS}
    _assert_checked(case, taps, torch.from_numpy(got['heat']), torch.from_numpy(got['idx']), kernels)
