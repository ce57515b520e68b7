"""The heatmap-loss pass's device-free decisions (csrc/detect_loss_plan.h) on the CPU, through the stand-alone program
tests/helpers/host_detect_loss_plan.cpp built with AddressSanitizer and UndefinedBehaviorSanitizer.  The program runs as a child
process (nothing of it is loaded into python) and carries its sanitizer runtimes itself (linked statically); every run must end with
status 0 and an empty stderr, i.e. without a sanitizer report.

loss_kernel fills its LDS slots and reads them through the header's functions, and its entry points launch it with the header's
plan: what the program holds together here is what the kernel does.  Sweep: every (h, out_h) of 1 .. 40 x 1 .. 80 and the real pairs
at five widths.  Pinned plans: the values the loss pass had before the plan moved into the header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (1, 1920, 2560, 3840, 7680)
REAL_PAIRS = 8          # host_detect_grad_plan.cpp's


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('hostdetectloss') / 'host_detect_loss_plan')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-static-libubsan', '-o', exe,
                           os.path.join(ROOT, 'tests', 'helpers', 'host_detect_loss_plan.cpp')])
    return exe


def run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == '', (args, r.returncode, r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert not [l for l in lines if l.startswith('FAIL')], lines[:20]
    assert lines[-1] == 'failures 0', lines[-3:]
    return lines


def test_every_strip_of_the_sweep(prog):
    """Per shape: the strip height is the largest of 1 .. 8 whose worst strip fits the LDS budget, 0 exactly when the rows a single
    output row reads (two, one for a map of one row) do not fit; lds is slots * w * 4 within the budget.  Per strip and output row:
    both slots it reads lie inside the strip's slots, which number at most the plan's; the fill rule puts into them the two source
    rows dg_src_coord names; every filled slot's source row lies inside the map.  Both layouts are reached."""
    lines = run(prog, 'sweep')
    assert lines[-3] == 'cases %d' % (len(WIDTHS) * (40 * 80 + REAL_PAIRS))
    head, count = lines[-2].split()
    assert head == 'noncontiguous' and int(count) > 0          # not the contiguous layout alone


def _plan(prog, h, w, out_h):
    lines = run(prog, 'plan', h, w, out_h)
    return {k: int(v) for k, v in zip(lines[0].split()[0::2], lines[0].split()[1::2])}


# (h, w, out_h) -> (strip, slots, nstrips, lds, strips in the non-contiguous layout): evaluated on the CPU from the text of loss_plan
# as it stood in csrc/detect_eval.hip before this header existed
PINNED = {
    (704, 1280, 1080): (8, 7, 135, 35840, 0),          # WASB / HRNet
    (160, 288, 1080): (8, 4, 135, 4608, 0),          # ViTPose
    (1080, 1920, 1080): (7, 8, 155, 61440, 0),          # the identity
    (11, 20, 1080): (8, 3, 135, 240, 0),
    (1, 1, 1080): (8, 1, 135, 4, 0),
    (37, 53, 37): (8, 9, 5, 1908, 0),
    (22, 40, 37): (8, 6, 5, 960, 0),
    (8, 2048, 1080): (8, 3, 135, 24576, 0),
    (64, 50, 7): (8, 14, 1, 2800, 1),          # the one non-contiguous strip
    (2160, 3840, 1080): (2, 4, 540, 61440, 0),
    (8, 7680, 1080): (1, 2, 1080, 61440, 0),
}


@pytest.mark.parametrize('shape', sorted(PINNED))
def test_pinned_plans(prog, shape):
    strip, slots, nstrips, lds, noncontiguous = PINNED[shape]
    assert _plan(prog, *shape) == dict(strip=strip, slots=slots, nstrips=nstrips, lds=lds, noncontiguous=noncontiguous)


@pytest.mark.parametrize('shape', [(8, 7681, 1080), (2, 7681, 1080)])
def test_refused_widths(prog, shape):
    """Two source rows of 7681 floats do not fit 60 KB."""
    assert _plan(prog, *shape) == dict(strip=0, slots=0, nstrips=0, lds=0, noncontiguous=0)
