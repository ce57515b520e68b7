"""The heatmap-loss gradient's device-free decisions (csrc/detect_grad_plan.h) on the CPU, through the stand-alone program
tests/helpers/host_detect_grad_plan.cpp built with AddressSanitizer and UndefinedBehaviorSanitizer.  The program runs as a child
process (nothing of it is loaded into python) and carries its sanitizer runtimes itself (linked statically); every run must end with
status 0 and an empty stderr, i.e. without a sanitizer report.

Ranges: which output indices read which source index, one axis at a time (the interpolation is separable), on every (in, out) of
1 .. 40 x 1 .. 80 and the real pairs -- the kernel gathers over exactly these ranges, so a wrong one is a wrong gradient.
Strips: how the source rows of every LOSS_EDGES map shape are cut, what a workgroup keeps in LDS, which output rows it walks and which lane serves which source column."""
import os
import subprocess

import numpy as np
import pytest

from helpers import detect_grad_cases as GC
from helpers import detect_grad_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BUDGET = 60 * 1024
STRIP = 8


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('hostdetectgrad') / 'host_detect_grad_plan')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-static-libubsan', '-o', exe,
                           os.path.join(ROOT, 'tests', 'helpers', 'host_detect_grad_plan.cpp')])
    return exe


def run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == '', (args, r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert not [l for l in lines if l.startswith('FAIL')], lines[:20]
    assert lines[-1] == 'failures 0', lines[-3:]
    return lines


def test_ranges_of_every_pair(prog):
    """Per pair: dg_first is the first output index whose lower source index reaches k; the readers of a source index are one range,
    the ranges move forward with the source index, every output index lies in the range of both indices it reads, an index nothing
    reads has an empty range, and the weights of every output index are non-negative and sum to 1 (within one rounding)."""
    lines = run(prog, 'ranges')
    assert lines[-2] == 'cases %d' % (40 * 80 + 8)


REAL_PAIRS = ((704, 1080), (1280, 1920), (160, 1080), (288, 1920), (1080, 1080), (2048, 1920), (64, 7), (50, 9))


def test_the_restatements_unread_indices_are_the_plans(prog):
    """The GPU test takes the rows and columns that must hold +0.0 from the numpy restatement (`detect_grad_ref.unread`).  Here that
    set is held to the plan's: the source indices whose `dg_readers` range is empty, for every pair of the sweep, the real pairs
    and both axes of every case whose unread rows and columns the GPU test inspects."""
    pairs = [(i, o) for i in range(1, 41) for o in range(1, 81)] + list(REAL_PAIRS)
    pairs += [axis for name in GC.UNREAD_EDGES for axis in GC.edge_axes(name)]
    r = subprocess.run([prog, 'unread'] + [str(v) for p in pairs for v in p], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == '', (r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(pairs)
    some = 0
    for (i, o), line in zip(pairs, lines):
        head, _, tail = line.partition(':')
        assert head == '%d %d' % (i, o)
        plan = [int(v) for v in tail.split()]
        assert plan == list(np.nonzero(G.unread(o, i))[0]), (i, o)
        some += bool(plan)
    assert some >= 300          # (388 of the pairs skip an index: the comparison is not one of empty sets)


def _strips(prog, h, w, out_h, out_w):
    lines = run(prog, 'strips', h, w, out_h, out_w)
    return {k: int(v) for k, v in zip(lines[0].split()[0::2], lines[0].split()[1::2])}


@pytest.mark.parametrize('name', GC.GRAD_EDGES)
def test_strips_cover_every_source_row_once(prog, name):
    """Every source row belongs to one strip; the strip's walk visits every output row that reads it (the weights it meets add up
    to the row's); the rows it keeps in LDS hold both neighbours of every output row it walks; the LDS bytes are within the budget
    every source column belongs to one lane of one wave of one group, and the group keeps it and its right neighbour."""
    (h, out_h), (w, out_w) = GC.edge_axes(name)
    p = _strips(prog, h, w, out_h, out_w)
    assert p['strip'] == min(STRIP, h) and p['nstrips'] == -(-h // p['strip'])
    nwaves = -(-w // 63)          # waves of 63 columns: the fewest groups of at most 8, then the fewest waves per group -- none is idle
    assert p['groups'] == -(-nwaves // 8) and p['waves'] == -(-nwaves // p['groups']) <= 8
    assert p['lds'] == (p['strip'] + 2) * min(w, p['waves'] * 63 + 2) * 4 <= LDS_BUDGET


def test_plans_of_the_detectors(prog):
    assert _strips(prog, 704, 1280, 1080, 1920) == dict(strip=8, nstrips=88, waves=7, groups=3, lds=17720)          # WASB / HRNet: 21 waves of 63 columns
    assert _strips(prog, 160, 288, 1080, 1920) == dict(strip=8, nstrips=20, waves=5, groups=1, lds=11520)          # ViTPose
    assert _strips(prog, 1080, 1920, 1080, 1920) == dict(strip=8, nstrips=135, waves=8, groups=4, lds=20240)
    assert _strips(prog, 8, 7680, 1080, 1920) == dict(strip=8, nstrips=1, waves=8, groups=16, lds=20240)
    assert _strips(prog, 1, 1, 1080, 1920) == dict(strip=1, nstrips=1, waves=1, groups=1, lds=12)


@pytest.mark.parametrize('shape', [(0, 4, 4, 4), (4, 0, 4, 4), (4, 4, 0, 4), (4, 4, 4, 0), (-1, 4, 4, 4)])
def test_refused_shapes(prog, shape):
    """An empty map or output has no plan (the width limit is the loss pass's, checked by the entry point)."""
    assert _strips(prog, *shape) == dict(strip=0, nstrips=0, waves=0, groups=0, lds=0)
