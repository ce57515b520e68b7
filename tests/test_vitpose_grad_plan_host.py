"""The ViTPose backbone training pass's device-free decisions (csrc/vitpose_grad_plan.h) on the CPU, through the stand-alone program
tests/helpers/host_vitpose_grad_plan.cpp built with AddressSanitizer and UndefinedBehaviorSanitizer.  The program runs as a child
process (nothing of it is loaded into python) and carries its sanitizer runtimes itself (linked statically); every run must end with
status 0 and an empty stderr, i.e. without a sanitizer report.

Table: the 149 tensors against the reference's key list and shapes (weights.vitpose_schema, and the keys the reference's own ViT
gave the goldens), contiguous offsets, total size, and the Python binding's copy.  Workspace: alignment, overlap, sizing up to 2^22
tokens, the documented bytes a token.  Slices at 511 / 512 / 513 / 1024 tokens.  The attention backward's grids at 1, 63, 64, 65, 129
tokens.  Refusals: the TTUP_EINVAL list."""
import os
import subprocess

import numpy as np
import pytest

from helpers import vitpose_backbone_cases as cases
from upliftingtabletennis_amd import vitpose_backbone, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'vitpose_backbone_grad.npz')


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('hostgradplan') / 'host_vitpose_grad_plan')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-static-libubsan', '-o', exe,
                           os.path.join(ROOT, 'tests', 'helpers', 'host_vitpose_grad_plan.cpp')])
    return exe


def run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == '', (args, r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def _no_failures(lines, n_cases):
    assert not [l for l in lines if l.startswith('FAIL')], lines[:20]
    assert lines[-2:] == ['cases %d' % n_cases, 'failures 0'], lines[-3:]


@pytest.mark.parametrize('in_ch,hp,wp', [(3, 40, 72), (9, 40, 72), (1, 1, 1), (16, 5, 13)])
def test_gradient_table_is_the_references_key_list(prog, in_ch, hp, wp):
    lines = run(prog, 'table', in_ch, hp * wp)
    assert not [l for l in lines if l.startswith('FAIL')], lines[:5]
    rows = [l.split() for l in lines[:-1]]
    got = [(r[0], tuple(int(v) for v in r[2:2 + int(r[1])]), int(r[6]), int(r[7])) for r in rows]
    # the reference's keys and shapes, in state_dict order
    want = [(k[len('model.backbone.'):], tuple(s)) for k, s in weights.vitpose_schema(in_ch, 1, (16 * wp, 16 * hp)) if k.startswith('model.backbone.')]
    assert len(got) == 149 and [(k, s) for k, s, _, _ in got] == want
    assert [(k, s) for k, s, _, _ in got] == vitpose_backbone.backbone_shapes(in_ch, hp * wp)
    off = 0
    for k, s, o, n in got:          # no gap, no overlap
        assert o == off and n == int(np.prod(s)), k
        off += n
    assert lines[-1] == 'total %d' % off
    assert off == sum(int(np.prod(s)) for _, s in want)


def test_gradient_table_holds_the_keys_the_references_vit_has():
    g = np.load(GOLDEN)
    name = cases.GOLDEN_CASES[0]
    keys = sorted(k[len(name) + 1:-len('/norm')] for k in g.files if k.startswith(name + '/') and k.endswith('/norm'))
    assert keys == sorted(k for k, _ in vitpose_backbone.backbone_shapes(1, 3))


def test_workspace_is_aligned_disjoint_and_large_enough(prog):
    """max_rows {1, 2, 63, 64, 65, 511, 512, 513, 1024, 1025, 23040, 2^22} x in_ch {1, 3, 9, 16}"""
    _no_failures(run(prog, 'workspace'), 48)


def test_slices(prog):
    out = run(prog, 'slices', 511, 512, 513, 1024, *[cases.tokens(n) for n in cases.CASES])
    assert out[-1] == 'slice_tokens %d' % cases.SLICE_TOKENS
    got = [[int(v) for v in l.split()] for l in out[:-1]]
    assert got[:4] == [[511, 1, 511], [512, 1, 512], [513, 2, 1], [1024, 2, 512]]
    s = cases.SLICE_TOKENS
    for t, ns, last in got:
        assert ns == -(-t // s) and last == (t - 1) % s + 1
    by = {n: r for n, r in zip(cases.CASES, got[4:])}
    assert by['s512'] == [512, 1, 512] and by['s513'] == [513, 2, 1] and by['s1024'] == [1024, 2, 512]          # the case table reaches the three edges


def test_attention_backward_grids(prog):
    out = run(prog, 'attn', 1, 1, 63, 2, 64, 3, 65, 1, 129, 8)
    assert out[-1] == 'lds %d' % ((2 * 64 * 36 + 128) * 4) and int(out[-1].split()[1]) < 160 * 1024 // 8
    got = [[int(v) for v in l.split()] for l in out[:-1]]
    #       ntok batch  grid x (tiles) y (heads) z (samples)  tiles walked  delta grid
    assert got == [[1, 1, 1, 12, 1, 1, 1, 12], [63, 2, 1, 12, 2, 1, 2, 12], [64, 3, 1, 12, 3, 1, 3, 12], [65, 1, 2, 12, 1, 2, 2, 12],
                   [129, 8, 3, 12, 8, 3, 17, 12]]
    assert {cases.CASES[n][1] * cases.CASES[n][2] for n in cases.CASES} >= {1, 63, 64, 65, 128, 129}


def test_refusals(prog):
    _no_failures(run(prog, 'refusals'), 6)
