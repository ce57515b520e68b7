"""The certified argmax's device-free decisions (csrc/certify_plan.h) on the CPU, through the stand-alone program
tests/helpers/host_certify_plan.cpp built with AddressSanitizer and UndefinedBehaviorSanitizer.  The program runs as a child process
(nothing of it is loaded into python) and carries its sanitizer runtimes itself (linked statically); every run must end with status 0
and an empty stderr, i.e. without a sanitizer report.

Geometry: every cluster span the crop walk can produce, at every start position, on every frame extent x crop side of the list below,
one axis at a time (the rule is separable).  This is what stands where the plan kernel used to carry a fallback "that cannot happen":
the whole bounding box of a new crop's cluster lies in that crop's core, so the walk covers one more candidate per crop and ends.
Walk: the same on random clustered candidate sets in two dimensions.  Sizing: the table of ttup_wasb_set_certify's arithmetic.
Names: the counter enum against `_lib.CERT_STATS`, the status constants against `_lib`'s."""
import os
import subprocess

import pytest

from upliftingtabletennis_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
FIELDS = ('Hc', 'Wc', 'CH', 'maxc', 'maxf', 'max_crops', 'nchunks', 'budget', 'small')


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('hostcertify') / 'host_certify_plan')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-static-libubsan', '-o', exe,
                           os.path.join(ROOT, 'tests', 'helpers', 'host_certify_plan.cpp')])
    return exe


def run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == '', (args, r.returncode, r.stderr[-2000:])
    return r.stdout


def _no_failures(out):
    lines = out.splitlines()
    assert not [l for l in lines if l.startswith('FAIL')], lines[:20]
    assert lines[-1] == 'failures 0', lines[-3:]
    return lines


def test_geometry_every_span_at_every_position_per_axis(prog):
    """Extents {168, 176, 352, 640, 704, 1280} x sides {160, 168, 176, 200}, spans 0 .. side - 2 R - 10 (class 2: <= 6): the origin is
    a multiple of 8 in [0, full - crop], the bounding box lies in the core, the core keeps R + 1 from every edge that is not the image's."""
    lines = _no_failures(run(prog, 'geometry'))
    # class 1 alone: sum over the 24 pairs of sum_{span} (full - span); class 2 adds 7 spans where the side is at least 168
    want = 0
    for full in (168, 176, 352, 640, 704, 1280):
        for side in (160, 168, 176, 200):
            c = min(side, full)
            want += sum(full - s for s in range(max(0, c - 2 * 72 - 10) + 1))
            if c >= 2 * 72 + 24:
                want += sum(full - s for s in range(7))
    assert lines[-2] == 'cases %d' % want


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_crop_walk_covers_its_candidate_and_ends(prog, seed):
    """352x640 and 704x1280 frames, sides 160 and 168, 1 .. 512 candidates in up to four 40x40 boxes, the first of them anywhere, in
    each corner and on each edge: every new crop covers the candidate it was opened for, the walk needs at most `cnt` crops, and every
    candidate's in-image 3x3 neighbourhood lies inside its crop."""
    lines = _no_failures(run(prog, 'walk', seed))
    sets, crops = (int(v) for v in lines[-2].split()[1::2])
    assert sets == 2 * 2 * 9 * 24 and crops >= sets


def _sizing(prog, H, W, max_batch, n_out, crop, maxc, knobs=()):
    out = run(prog, 'sizing', H, W, max_batch, n_out, crop, maxc, *knobs).splitlines()
    rc, err = int(out[0].split('=')[1]), out[1].split('=', 1)[1]
    return rc, err, {k: int(v) for k, v in (tok.split('=') for tok in out[2].split())}


SIZING = [  # max_batch, n_out, H, W, crop, maxc -> Hc, Wc, CH, maxc, maxf, max_crops, nchunks, budget, small
    ((64, 1, 704, 1280, 0, 0), (168, 168, 64, 8, 8, 256, 4, 64, 14)),
    ((64, 13, 704, 1280, 0, 0), (168, 168, 64, 8, 32, 256, 4, 64, 14)),
    ((1, 1, 704, 1280, 0, 0), (168, 168, 1, 8, 8, 8, 8, 1, 14)),
    ((1, 13, 704, 1280, 0, 0), (168, 168, 1, 8, 32, 32, 32, 1, 14)),
    ((16, 13, 352, 640, 0, 3), (168, 168, 16, 3, 32, 64, 4, 16, 14)),
    ((12, 1, 352, 640, 0, 32), (168, 168, 12, 32, 32, 48, 4, 12, 14)),
    ((200, 1, 704, 1280, 0, 0), (168, 168, 128, 8, 8, 896, 7, 200, 14)),
    ((8, 1, 352, 640, 160, 0), (160, 160, 8, 8, 8, 32, 4, 8, 0)),
    ((4, 1, 128, 640, 0, 0), (128, 168, 4, 8, 8, 16, 4, 4, 0)),          # no cone pruning: Hc != Wc
]


@pytest.mark.parametrize('args,want', SIZING)
def test_sizing_table(prog, args, want):
    max_batch, n_out, H, W, crop, maxc = args
    rc, err, got = _sizing(prog, H, W, max_batch, n_out, crop, maxc)
    assert rc == 0 and err == ''
    assert tuple(got[k] for k in FIELDS) == want
    assert got['cone'] == (1 if got['Hc'] == got['Wc'] else 0)          # (all rows: interior crops larger than 2 R + 2)


@pytest.mark.parametrize('args,message', [
    ((704, 1280, 64, 1, 164, 0), 'ttup_wasb_set_certify: crop 164 must be a multiple of 8 and at least 160'),
    ((704, 1280, 64, 1, 152, 0), 'ttup_wasb_set_certify: crop 152 must be a multiple of 8 and at least 160'),
    ((704, 644, 64, 1, 0, 0), 'ttup_wasb_set_certify: 704x644 heatmaps with 168x168 crops cannot be certified (H*W % 4, (H-Hc) % 8, (W-Wc) % 8 must be 0)'),
    ((704, 1280, 64, 1, 0, 33), 'ttup_wasb_set_certify: bad argument'),
    ((704, 1280, 4096, 1, 0, 0), 'ttup_wasb_set_certify: max_batch 4096 too large'),          # nchunks 128 > 64
])
def test_sizing_rejects(prog, args, message):
    rc, err, _ = _sizing(prog, *args)
    assert rc == EINVAL and err == message


def test_each_knob_changes_only_what_it_names(prog):
    row = (704, 1280, 64, 1, 0, 0)
    _, _, base = _sizing(prog, *row)
    # knobs: TTUP_CERT_LIST, TTUP_CERT_CH, TTUP_CERT_SMALL=0, TTUP_NO_CONE
    _, _, ch = _sizing(prog, *row, knobs=(0, 64, 0, 0))
    assert ch == base          # (max_batch 64: the cap of 128 did not bind either)
    _, _, ch = _sizing(prog, 704, 1280, 200, 1, 0, 0, knobs=(0, 64, 0, 0))
    _, _, base200 = _sizing(prog, 704, 1280, 200, 1, 0, 0)
    assert ch == dict(base200, CH=64, nchunks=13, max_crops=832)          # the crop list in passes of 64: ceil(800 / 64)
    _, _, lst = _sizing(prog, *row, knobs=(2, 0, 0, 0))
    assert lst == dict(base, max_crops=128, nchunks=2)
    _, _, small = _sizing(prog, *row, knobs=(0, 0, 1, 0))
    assert small == dict(base, small=0)
    _, _, cone = _sizing(prog, *row, knobs=(0, 0, 0, 1))
    assert cone == dict(base, cone=0, small=0)          # class-2 crops are a form of the cone pruning


def test_names_match_the_python_mirror(prog):
    out = run(prog, 'names').splitlines()
    assert tuple(l.split()[1] for l in out if l.startswith('stat ')) == _lib.CERT_STATS and len(_lib.CERT_STATS) == 12
    st = {k: int(v) for k, v in (tok.split('=') for tok in [l for l in out if l.startswith('status ')][0].split()[1:])}
    assert (st['single'], st['resolved'], st['not_certified'], st['guard']) == (_lib.CERT_SINGLE, _lib.CERT_RESOLVED, _lib.CERT_NOT_CERTIFIED, _lib.CERT_GUARD) == (0, 1, 2, 4)
    assert (st['status_mask'], st['flags_mask']) == (_lib.CERT_STATUS_MASK, _lib.CERT_FLAGS_MASK) == (3, 7)
    assert (st['pending'], st['audit_only']) == (8, 16)
    consts = {k: int(v) for k, v in (tok.split('=') for tok in [l for l in out if l.startswith('const ')][0].split()[1:])}
    assert consts == dict(max_k=512, max_frame_crops=32, r=72, small=14, sizeof_croprec=16)
