"""The uplift inference forward (csrc/uplift.hip) at its length, tile and mask edges: every case of tests/helpers/uplift_forward_cases.py
against the high-precision mode of the torch restatement (tests/helpers/uplift_torch_grad.py: float64, RoPE index in float32) or, for
the non-default variants, against the reference's own outputs (tests/golden/uplift_family_edges.npz), at the project's parity bar
max|out - ref| <= 1e-4 max|ref| for the spin and for ALL positions, padded rows included.  Beside each error the fp32 restatement's
own distance to the high-precision mode is printed: the noise floor of a correct fp32 forward.

Measured on an MI355X, worst over the cases (rot / pos; DESIGN.md 15 has the table per kernel form): 2.0e-6 / 1.9e-6 against the
high-precision restatement, 1.8e-6 / 2.0e-6 against the fixture, with the fp32 restatement itself at 1.8e-6 / 1.9e-6; the per-layer
kernels return the default path's bits at every short length."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from helpers import uplift_forward_cases as C
from helpers import uplift_torch_grad as R
from upliftingtabletennis_amd import uplift, weights

pytestmark = pytest.mark.gpu

BAR = 1e-4               # BASELINE.json north_star
PATHS_BAR = 2e-6         # stage kernel vs per-layer kernels: the bar of test_uplift_stage_kernel_against_the_per_layer_kernels for the same pair
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def state_dict(c):
    return weights.random_uplift_state_dict(c.seed, c.size, c.name, c.mode, c.rot)


def build(c, **kw):
    kw = dict(dict(max_batch=c.b, max_len=c.t + c.pad), **kw)
    return uplift.get_model(c.name, c.size, c.mode, c.rot, state_dict=state_dict(c), **kw)


def bits_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def reference(c):
    """-> (rot, pos) of the high-precision restatement (float64), and the fp32 restatement's distance to it (rot, pos): computed once per case"""
    sd, inputs = state_dict(c), C.make_inputs(c)
    hrot, hpos = R.forward_np(sd, c.size, *inputs, time_rotation=c.rot, high_precision=True)
    rot, pos = R.forward_np(sd, c.size, *inputs, time_rotation=c.rot)
    assert np.isfinite(hrot).all() and np.isfinite(hpos).all()
    return hrot, hpos, (C.rel(rot, hrot), C.rel(pos, hpos))


@functools.lru_cache(maxsize=None)
def on_device(c):
    """One forward of the case on the default stream, and a second one -> rot, pos (numpy), stage launches per forward, second call bit-equal"""
    net = build(c)
    args = [torch.from_numpy(a).cuda() for a in C.make_inputs(c)]
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    before = net.graph_info()['stage_launches']
    first = net(*args)
    launches = net.graph_info()['stage_launches'] - before
    second = net(*args)
    torch.cuda.synchronize()
    gi = net.graph_info()
    assert gi['replays'] == 0 and gi['stage_launches'] - before == 2 * launches          # (stream 0 is never captured)
    return first[0].cpu().numpy(), first[1].cpu().numpy(), launches, bits_equal(first, second)


@pytest.mark.parametrize('case', C.SWEEP, ids=C.key)
def test_default_variant_at_its_edges(case):
    """connectstage / dynamic: finite, repeatable to the bit, within the bar of the high-precision restatement, and -- `large` -- served
    by the stage kernel exactly where the helper's restatement of run_stage's rule says so."""
    hrot, hpos, floor = reference(case)
    rot, pos, launches, same = on_device(case)
    e_rot, e_pos = C.rel(rot, hrot), C.rel(pos, hpos)
    forms = sorted({C.attention_form(case, s) for s in C.stage_sequences(case)})
    print('\n%s [%s]: max|out - ref| / max|ref|  rot %.3e  pos %.3e   (fp32 restatement: rot %.3e  pos %.3e)' % (C.key(case), ' '.join(forms), e_rot, e_pos, floor[0], floor[1]))
    assert rot.shape == hrot.shape and pos.shape == hpos.shape and np.isfinite(rot).all() and np.isfinite(pos).all()
    assert same
    if case.size == 'large':
        assert launches == C.stage_launches(case), (launches, C.stage_launches(case))
    else:
        assert launches == 0
    assert e_rot <= BAR and e_pos <= BAR


@pytest.mark.parametrize('case', C.FAMILY, ids=C.key)
def test_variants_at_their_edges(golden, case):
    """Every case of the fixture against the reference model's own rot and pos: the 16-layer stage launch at S = 64 and the per-layer
    path with strip_cls3_kernel at S = 65, the declined S = 5 on the by-index RoPE table, embed3_cls_kernel's tile of 4 tokens,
    stacked_embed_kernel's workgroup of one token, the scalar attention of the other sizes past 128 tokens."""
    g = golden('uplift_family_edges.npz')
    k = C.key(case)
    rot, pos, launches, same = on_device(case)
    e_rot, e_pos = C.rel(rot, g[k + '/rot']), C.rel(pos, g[k + '/pos'])
    print('\n%s: max|out - ref| / max|ref|  rot %.3e  pos %.3e   (reference: the fixture)' % (k, e_rot, e_pos))
    assert np.isfinite(rot).all() and np.isfinite(pos).all() and same
    assert launches == (C.stage_launches(case) if case.size == 'large' else 0)
    assert e_rot <= BAR and e_pos <= BAR


@pytest.mark.parametrize('case', C.INERT, ids=C.key)
def test_masked_slots_are_inert_bit_for_bit(case):
    """The probability of a masked key is an exact zero in every attention kernel, so what a masked slot holds cannot move an output it
    is masked out of: other finite values in `ball` and `times` at every step with mask 0 and in the x, y of every invisible keypoint
    leave rot and the valid rows of pos bit-identical -- the spin of a trajectory that is padded throughout included."""
    ball, table, mask, times = C.make_inputs(case)
    rng = np.random.default_rng(case.seed)
    off, unseen = mask == 0, table[:, :, 2] != 1
    assert off.any() and unseen.any() and (mask[0, :case.t] == 0).any() and not mask[3].any() and unseen[0].all() and unseen[2].sum() == 12
    ball2, table2, times2 = ball.copy(), table.copy(), times.copy()
    ball2[off] = rng.uniform(0.0, 1.0, (int(off.sum()), 2)).astype(np.float32)
    times2[off] = rng.uniform(0.0, 3.0, int(off.sum())).astype(np.float32)
    table2[unseen, :2] = rng.uniform(-1.0, 2.0, (int(unseen.sum()), 2)).astype(np.float32)
    assert not np.array_equal(ball2, ball) and not np.array_equal(times2, times) and not np.array_equal(table2, table)
    net = build(case)
    rot, pos = net(*[torch.from_numpy(a) for a in (ball, table, mask, times)])
    rot2, pos2 = net(*[torch.from_numpy(a) for a in (ball2, table2, mask, times2)])
    rot, pos, rot2, pos2 = [a.cpu().numpy() for a in (rot, pos, rot2, pos2)]
    assert np.isfinite(rot2).all() and np.isfinite(pos2).all()
    on = mask == 1
    moved = sorted(set(np.nonzero((pos2 != pos).any(2) & on)[0].tolist()))
    assert np.array_equal(rot2[3], rot[3]), 'the spin of the trajectory that is padded throughout moved'
    assert np.array_equal(rot2, rot), 'spin moved: trajectories %s' % sorted(set(np.nonzero(rot2 != rot)[0].tolist()))
    assert np.array_equal(pos2[on], pos[on]), 'valid positions moved: trajectories %s' % moved
    assert not np.array_equal(pos2[off], pos[off])          # the masked rows did see the other values: the perturbation reached the kernels


CHILD = ('import sys, numpy as np, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n'
         'import test_uplift_forward_edges_gpu as t\n'
         'out = {"stage": 0}\n'
         'for c in t.C.NO_STAGE:\n'
         '    rot, pos, launches, same = t.on_device(c)\n'
         '    assert same\n'
         '    out["stage"] += launches; out["rot_" + t.C.key(c)] = rot; out["pos_" + t.C.key(c)] = pos\n'
         'np.savez(sys.argv[1], **out)')


def test_per_layer_kernels_at_the_short_lengths():
    """TTUP_UPLIFT_NO_STAGE=1 (child process): attn_block_x3_kernel at S = 1, 2, 3, 4, 5, 6, 8, 9, 16 with 64 // S sequences per tile and
    attention_mfma8_kernel<1> at S = 17, 18, 21, 22 -- lengths the default path gives to the stage kernel.  No stage launch happens;
    every case is within the bar of the reference and within 2e-6 (relative to max|ref|) of the default process."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, 'layers.npz')
        subprocess.run([sys.executable, '-c', CHILD % (ROOT, os.path.join(ROOT, 'tests')), out], check=True, env=dict(os.environ, TTUP_UPLIFT_NO_STAGE='1'), timeout=300)
        res = dict(np.load(out))
    assert int(res['stage']) == 0
    for c in C.NO_STAGE:
        hrot, hpos, _ = reference(c)
        rot, pos, launches, _ = on_device(c)
        assert launches == C.stage_launches(c) > 0
        for what, x, y, ref in (('rot', res['rot_' + C.key(c)], rot, hrot), ('pos', res['pos_' + C.key(c)], pos, hpos)):
            e, d = C.rel(x, ref), float(np.abs(x.astype(np.float64) - y).max() / np.abs(ref).max())
            print('%s %s: per-layer kernels vs reference %.3e, vs the default path %.3e' % (C.key(c), what, e, d))
            assert np.isfinite(x).all() and e <= BAR and d <= PATHS_BAR, (C.key(c), what)


def test_graph_replay_of_a_shape_the_stage_kernel_declines():
    """large 3 x 5 on a side stream: S = 5 runs in attn_block_x3_kernel inside the captured graph; the replays return the bits of the
    default stream's eager call."""
    c = C.Case('large', 'connectstage', 'dynamic', 'new', 'edge', 3, 4, 1, 455)
    assert not C.stage_accepts(c.t + c.pad)
    net = build(c)
    args = [torch.from_numpy(a).cuda() for a in C.make_inputs(c)]
    eager = [a.clone() for a in net(*args)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    outs = []
    with torch.cuda.stream(side):
        for _ in range(4):          # eager, capture + launch, replay, replay
            outs.append([a.clone() for a in net(*args)])
    side.synchronize()
    gi = net.graph_info()
    assert gi['replays'] >= 2 and not gi['off'], gi
    assert all(bits_equal(o, eager) for o in outs)


@pytest.mark.parametrize('size', ['large', 'huge'])
def test_unservable_length_is_refused_on_entry(size):
    """len + 1 tokens beyond what the attention kernels serve (the sweep's len 511 / 333 are the last that pass): ValueError before the
    memset, any launch or any capture, on the default stream and -- one trajectory, so the call would go to the graph path -- on a
    side stream.  The handle is untouched: the earlier bits for a short call, the graph path still on, and replaying."""
    limit = C.MAX_SEQ[size] - 1
    assert any(c.size == size and c.t + c.pad == limit for c in C.SWEEP)
    short = C.Case(size, 'connectstage', 'dynamic', 'new', 'edge', 3, 6, 2, 1500)
    net = build(short, max_batch=4, max_len=limit + 1)
    args = [torch.from_numpy(a).cuda() for a in C.make_inputs(short)]
    too_long = [torch.from_numpy(a).cuda() for a in C.make_inputs(short._replace(kind='ragged', b=1, t=limit - 2, pad=3))]
    assert too_long[0].shape == (1, limit + 1, 2)
    before = [a.clone() for a in net(*args)]
    launches = net.graph_info()['stage_launches']
    with pytest.raises(ValueError, match='sequence length'):
        net(*too_long)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):          # (a capture that failed would come with the second call of the shape)
            with pytest.raises(ValueError, match='sequence length'):
                net(*too_long)
        gi = net.graph_info()
        assert not gi['off'] and gi['graphs'] == 0 and gi['stage_launches'] == launches, gi
        outs = [[a.clone() for a in net(*args)] for _ in range(3)]
    side.synchronize()
    gi = net.graph_info()
    assert not gi['off'] and gi['graphs'] == 1 and gi['replays'] >= 1, gi
    assert all(bits_equal(o, before) for o in outs)
    assert bits_equal(net(*args), before)
