"""The float64 restatement of the ViTPose head's training pass (tests/helpers/vitpose_head_ref.py) on the CPU: against torch's own
operators with float64 autograd on every case of the table, and against what the reference's own head gave in float32
(tests/golden/vitpose_head_grad.npz, tools/make_goldens_vitpose_head.py).  Also what the GPU test relies on in the case table: the
seeds keep the share of undecided ReLU gates under the cap, and the special channels do what they are there for."""
import os

import numpy as np
import pytest
import torch

from helpers import vitpose_head_cases as cases
from helpers import vitpose_head_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vitpose_head_grad.npz')
UNDECIDED_CAP = 1e-3


@pytest.fixture(scope='module')
def computed():
    """name -> (feat, params, dheat, forward, grads) of the restatement, once"""
    out = {}
    for name, (_, _, _, _, _, train) in cases.CASES.items():
        feat, p, dheat = cases.make_case(name)
        f = ref.forward(feat, p, train)
        out[name] = (feat, p, dheat, f, ref.backward(f, p, dheat, train))
    return out


@pytest.mark.parametrize('name', list(cases.CASES))
def test_restatement_is_torch_float64_autograd(computed, name):
    """heat, the four running statistics, the eight parameter gradients and dfeat within 1e-10 relative"""
    feat, p, dheat, f, g = computed[name]
    train = cases.CASES[name][5]
    heat, run, grads = ref.torch_reference(feat, p, dheat, train, torch.float64)
    worst = {'heat': max(ref.rel_l2(f['heat'], heat), ref.rel_max(f['heat'], heat))}
    for k in run:
        worst[k] = max(ref.rel_l2(f[k], run[k]), ref.rel_max(f[k], run[k]))
    for k in grads:
        worst['d' + k] = max(ref.rel_l2(g[k], grads[k]), ref.rel_max(g[k], grads[k]))
    print(name, worst)
    assert max(worst.values()) <= 1e-10, worst


@pytest.mark.parametrize('name', list(cases.CASES))
def test_seed_keeps_undecided_gates_under_the_cap_and_special_channels_work(computed, name):
    _, p, _, f, g = computed[name]
    u1, u2 = ref.undecided(f, p)
    assert u1.mean() <= UNDECIDED_CAP and u2.mean() <= UNDECIDED_CAP, (u1.mean(), u2.mean())
    assert not f['z1'][:, cases.ZERO_CH].any()
    if cases.CASES[name][5]:          # batch statistics: variance 0, xhat 0 (eval mode normalises with the running statistics instead)
        assert f['var1'][cases.ZERO_CH] == 0 and not f['xhat1'][:, cases.ZERO_CH].any()
    for a, gk, bk, wk, ch in (('a1', 'g1', 'b1', 'W1', cases.DEAD1), ('a2', 'g2', 'b2', 'W2', cases.DEAD2)):
        assert not f[a][:, ch].any()
        assert g[gk][ch] == 0 and g[bk][ch] == 0 and not g[wk][:, ch].any()


def test_table_reaches_every_slice_form():
    """one slice exactly, whole slices only, a last slice of one token -- and grids below, at and above one 64-row tile"""
    t = {n: cases.tokens(n) for n in cases.CASES}
    s = cases.SLICE_TOKENS
    assert t['one_slice'] == s and t['whole_slices'] == 2 * s and t['last_of_one'] == s + 1
    assert t['g8x8'] == 64 and t['g5x13'] == 65 and t['g5x7'] == 35
    assert set(cases.GOLDEN_CASES) <= set(cases.CASES)


@pytest.mark.parametrize('name', cases.GOLDEN_CASES)
def test_restatement_against_the_reference_heads_float32(computed, name):
    """The reference's TopdownHeatmapSimpleHead in .train() / .eval(), float32 with autograd: the restatement lies within the
    distance the file itself records for each tensor (that distance was measured against this restatement when the file was
    made; here the stored values are held to it again, so a drift of either side shows), and every recorded distance is a float32
    distance: below 1e-4."""
    z = np.load(GOLDEN)
    _, _, _, f, g = computed[name]
    rule = int(z['subsample_stride'])
    mine = {'heat': f['heat'], 'rm1': f['rm1'], 'rv1': f['rv1'], 'rm2': f['rm2'], 'rv2': f['rv2'], 'dfeat': g['feat']}
    mine.update({'d' + k: g[k] for k in ref.GRADS})
    for k, v in mine.items():
        stored, dist = z['%s/%s' % (name, k)], float(z['%s/%s/dist' % (name, k)])
        assert dist < 1e-4, (k, dist)
        if k in ('dW1', 'dW2'):
            v = v.ravel()[::rule]
            norm = float(z['%s/%s/norm' % (name, k)])
            assert abs(norm - np.linalg.norm(g[k[1:]].ravel())) <= 1e-4 * norm, k
            assert stored.shape == v.shape, k
            assert np.linalg.norm(stored - v) <= 1.001 * dist * norm + 1e-30, (k, dist)          # a part's distance is at most the whole's
        else:
            assert stored.shape == v.shape, k
            assert ref.rel_l2(stored, v) <= 1.001 * dist + 1e-30, (k, ref.rel_l2(stored, v), dist)
    assert int(z['%s/num_batches_tracked' % name]) == (1 if cases.CASES[name][5] else 0)
