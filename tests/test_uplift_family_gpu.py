"""The uplift model family on the device: every variant the reference's get_model builds against the reference's own outputs
(tests/golden/uplift_family.npz, tools/make_goldens_uplift_family.py), at the project's parity bar -- max|out - ref| <= 1e-4 max|ref|
for the spin and for the positions."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from upliftingtabletennis_amd import inference, interface, synth, uplift, weights
from test_uplift_family_oracle import write_checkpoint

pytestmark = pytest.mark.gpu

BAR = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted({k.split('/')[0] for k in np.load(os.path.join(ROOT, 'tests', 'golden', 'uplift_family.npz')).files})


def load_case(g, case):
    """-> (size, name, mode, time_rotation), state_dict, [ball, table, mask, times] numpy, regenerated from the stored seeds."""
    size, name, mode, rot = [str(v) for v in g[case + '/variant']]
    seed, b, t, pad = [int(v) for v in g[case + '/meta']]
    return (size, name, mode, rot), weights.random_uplift_state_dict(seed, size, name, mode, rot), list(synth.ragged_uplift_batch(b, t, seed=seed, pad=pad))


def build(variant, sd, **kw):
    size, name, mode, rot = variant
    return uplift.get_model(name, size, mode, rot, state_dict=sd, **kw)


def rel(x, ref):
    return float(np.abs(np.asarray(x) - ref).max() / np.abs(ref).max())


def test_the_fixture_holds_the_cases_the_family_needs(golden):
    g = golden('uplift_family.npz')
    v = [tuple(str(x) for x in g[c + '/variant']) + (int(g[c + '/meta'][2] + g[c + '/meta'][3]),) for c in CASES]
    from upliftingtabletennis_amd import arch
    assert {x[1:4] for x in v if x[0] == 'small'} == set(arch.uplift_variants())
    large = [x for x in v if x[0] == 'large']
    assert {x[1:3] for x in large if x[3] == 'new'} >= {('singlestage', 'free'), ('singlestage', 'dynamic'), ('singlestage', 'stacked'), ('multistage', 'dynamic'),
                                                        ('multistage', 'stacked'), ('multistage', 'originalmethod'), ('connectstage', 'stacked'), ('connectstage', 'originalmethod')}
    assert sum(x[3] == 'old' for x in large) >= 2
    lengths = {x[4] for x in large}
    assert min(lengths) <= 15 and any(30 <= n <= 63 for n in lengths) and max(lengths) >= 121          # stage kernel, mid length, long-sequence attention
    assert {x[0] for x in v} == {'small', 'base', 'large', 'huge'}


@pytest.mark.parametrize('case', CASES)
def test_variant_matches_reference(golden, case):
    """Spin and 3-D positions within 1e-4 relative of the reference model's forward; and the bar resolves the variants: the same
    weights under the other time_rotation are at least ten bars away (distance stored by the generator)."""
    g = golden('uplift_family.npz')
    variant, sd, inputs = load_case(g, case)
    flip = g[case + '/flip']
    print('\n%s: reference new-vs-old distance rot %.3e pos %.3e' % (case, flip[0], flip[1]))
    assert flip.min() >= 10 * BAR
    net = build(variant, sd, max_batch=8, max_len=inputs[0].shape[1])
    rot, pos = net(*[torch.from_numpy(a) for a in inputs])
    rot, pos = rot.cpu().numpy(), pos.cpu().numpy()
    e_rot, e_pos = rel(rot, g[case + '/rot']), rel(pos, g[case + '/pos'])
    print('%s: max|out - ref| / max|ref|  rot %.3e  pos %.3e' % (case, e_rot, e_pos))
    assert np.isfinite(rot).all() and np.isfinite(pos).all()
    assert e_rot <= BAR and e_pos <= BAR


def test_sixteen_layer_stage_launch(golden):
    """`singlestage` at `large` runs all 16 layers in ONE stage_x3_kernel launch when the sequence fits a 64-token tile (no stage
    had more than 12 layers before): one launch per forward for 'free', and the result is the reference's."""
    g = golden('uplift_family.npz')
    case = 'large_singlestage_free_new_T11'
    variant, sd, inputs = load_case(g, case)
    net = build(variant, sd, max_batch=8, max_len=16)
    rot, pos = net(*[torch.from_numpy(a) for a in inputs])
    assert net.graph_info()['stage_launches'] == 1
    assert rel(rot.cpu().numpy(), g[case + '/rot']) <= BAR and rel(pos.cpu().numpy(), g[case + '/pos']) <= BAR


def test_every_table_input_matters_where_the_reference_reads_it(golden):
    """'stacked' feeds x, y AND visibility of the 13 keypoints to ball_embed, 'originalmethod' drops the visibility
    (model.py:345-353): a flipped visibility flag of a visible keypoint changes the first and leaves the second bit-identical; a
    moved keypoint changes both."""
    g = golden('uplift_family.npz')
    for case, reads_visibility in (('large_connectstage_stacked_new_T121', True), ('large_connectstage_originalmethod_new_T11', False)):
        variant, sd, inputs = load_case(g, case)
        net = build(variant, sd, max_batch=8, max_len=inputs[0].shape[1])
        base = [o.clone() for o in net(*[torch.from_numpy(a) for a in inputs])]
        table = inputs[1]
        kp = int(np.argmax(table[0, :, 2] == 1))          # a keypoint that IS visible in the seeded table
        assert table[0, kp, 2] == 1
        t_vis = table.copy(); t_vis[0, kp, 2] = 0
        out = net(*[torch.from_numpy(a) for a in (inputs[0], t_vis, inputs[2], inputs[3])])
        same = all(torch.equal(a[0], b[0]) for a, b in zip(out, base))
        assert same == (not reads_visibility), case
        assert all(torch.equal(a[1:], b[1:]) for a, b in zip(out, base))          # the other trajectories do not see trajectory 0's table
        t_xy = table.copy(); t_xy[0, 12, 1] += 0.05
        out = net(*[torch.from_numpy(a) for a in (inputs[0], t_xy, inputs[2], inputs[3])])
        assert not torch.equal(out[0][0], base[0][0]) and not torch.equal(out[1][0], base[1][0]), case
        assert all(torch.equal(a[1:], b[1:]) for a, b in zip(out, base))


CHILD = ('import sys, numpy as np, torch; sys.path.insert(0, %r); from upliftingtabletennis_amd import synth, uplift, weights\n'
         'out = {}\n'
         'for (name, mode, rot, seed, b, t, pad) in %r:\n'
         '    sd = weights.random_uplift_state_dict(seed, "large", name, mode, rot)\n'
         '    net = uplift.get_model(name, "large", mode, rot, state_dict=sd, max_batch=8, max_len=t + pad)\n'
         '    a = [torch.from_numpy(v).cuda() for v in synth.ragged_uplift_batch(b, t, seed=seed, pad=pad)]\n'
         '    side = torch.cuda.Stream(); side.wait_stream(torch.cuda.current_stream())\n'
         '    with torch.cuda.stream(side):\n'
         '        r = [net(*a) for _ in range(3)]\n'
         '    side.synchronize()\n'
         '    assert all(torch.equal(x[0], r[0][0]) and torch.equal(x[1], r[0][1]) for x in r)\n'
         '    gi = net.graph_info(); k = "%%s_%%s_%%s_%%d" %% (name, mode, rot, t)\n'
         '    out["rot_" + k] = r[2][0].cpu().numpy(); out["pos_" + k] = r[2][1].cpu().numpy(); out["info_" + k] = np.array([gi["replays"], gi["stage_launches"], int(gi["off"])])\n'
         'np.savez(sys.argv[1], **out)')
FAST_SHAPES = [('singlestage', 'free', 'new', 31, 3, 40, 9), ('singlestage', 'stacked', 'old', 32, 2, 8, 3), ('singlestage', 'dynamic', 'new', 33, 2, 118, 3),
               ('multistage', 'stacked', 'new', 34, 3, 40, 9), ('multistage', 'dynamic', 'old', 35, 2, 8, 3), ('connectstage', 'originalmethod', 'new', 36, 3, 40, 9)]


def test_new_variants_take_the_fast_paths():
    """Small calls of `large` variants go through the captured hipGraph and the whole-stage kernel like the default variant does:
    replays happen from the second same-shape call, a replay returns bit for bit what the eager first call returned and what a
    process without graphs (TTUP_UPLIFT_NO_GRAPH=1) returns, and the layer-by-layer path (TTUP_UPLIFT_UNFUSED=1: no stage kernel, no
    fused attention / MLP blocks) agrees within the parity bar."""
    code = CHILD % (ROOT, FAST_SHAPES)
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for tag, env in (('graph', {}), ('eager', {'TTUP_UPLIFT_NO_GRAPH': '1'}), ('unfused', {'TTUP_UPLIFT_UNFUSED': '1'})):
            e = dict(os.environ); e.update(env)
            out = os.path.join(td, tag + '.npz')
            subprocess.run([sys.executable, '-c', code, out], check=True, env=e, timeout=600)
            res[tag] = dict(np.load(out))
    for (name, mode, rot, seed, b, t, pad) in FAST_SHAPES:
        k = '%s_%s_%s_%d' % (name, mode, rot, t)
        replays, stage, off = [int(v) for v in res['graph']['info_' + k]]
        assert replays >= 1 and not off, (k, replays, off)
        if t + pad + 1 <= 64 or mode == 'dynamic':          # (sequences that fit a 64-token tile; the table stage always does)
            assert stage > 0, k
        assert int(res['eager']['info_' + k][0]) == 0 and int(res['unfused']['info_' + k][1]) == 0
        for what in ('rot_', 'pos_'):
            x = res['graph'][what + k]
            assert np.isfinite(x).all()
            assert np.array_equal(x, res['eager'][what + k]), (k, what)
            d = rel(x, res['unfused'][what + k])
            print('%s%s: fast path vs unfused per-layer path %.3e' % (what, k, d))
            assert d <= BAR, (k, what)


def test_stacked_embedding_summation_orders_both_hold_the_bar(golden):
    """stacked_embed_kernel reduces the table columns of fc1 once per workgroup and adds the two ball columns per token; a plain
    linear layer over the stacked input sums all K products per token.  The second order is kept behind
    TTUP_UPLIFT_STACKED_PER_TOKEN=1: both are within the parity bar of the reference on every `large` and `huge` stacked /
    originalmethod case (figures printed)."""
    g = golden('uplift_family.npz')
    cases = [c for c in CASES if not c.startswith('small') and str(g[c + '/variant'][2]) in ('stacked', 'originalmethod')]
    assert len(cases) >= 6
    code = ('import sys, numpy as np, torch; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_uplift_family_gpu as t\n'
            'g = np.load(%r); out = {}\n'
            'for c in %r:\n'
            '    variant, sd, inputs = t.load_case(g, c)\n'
            '    rot, pos = t.build(variant, sd, max_batch=8, max_len=inputs[0].shape[1])(*[torch.from_numpy(a) for a in inputs])\n'
            '    out[c + "/rot"] = rot.cpu().numpy(); out[c + "/pos"] = pos.cpu().numpy()\n'
            'np.savez(sys.argv[1], **out)' % (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden', 'uplift_family.npz'), cases))
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for tag, env in (('reduced', {}), ('per_token', {'TTUP_UPLIFT_STACKED_PER_TOKEN': '1'})):
            e = dict(os.environ); e.update(env)
            out = os.path.join(td, tag + '.npz')
            subprocess.run([sys.executable, '-c', code, out], check=True, env=e, timeout=600)
            res[tag] = dict(np.load(out))
    differ = False
    for c in cases:
        for k in ('/rot', '/pos'):
            a, b = rel(res['reduced'][c + k], g[c + k]), rel(res['per_token'][c + k], g[c + k])
            print('%s%s: vs reference  table columns reduced once %.3e   per token %.3e   between the two %.3e' % (c, k, a, b, rel(res['reduced'][c + k], res['per_token'][c + k])))
            assert a <= BAR and b <= BAR, (c, k)
            differ |= not np.array_equal(res['reduced'][c + k], res['per_token'][c + k])
    assert differ          # the switch is honoured: the two orders round differently somewhere


@pytest.mark.parametrize('name,mode,rot', [('singlestage', 'stacked', 'old'), ('multistage', 'originalmethod', 'new'), ('singlestage', 'free', 'new')])
def test_edge_inputs_behave_as_for_the_default_variant(name, mode, rot):
    sd = weights.random_uplift_state_dict(5, 'large', name, mode, rot)
    net = uplift.get_model(name, 'large', mode, rot, state_dict=sd, max_batch=16, max_len=64)
    assert (net.name, net.mode, net.time_rotation) == (name, mode, rot)
    ball, table, mask, times = [torch.from_numpy(a) for a in synth.synth_trajectories(12, 50, seed=9, pad=3)]
    with pytest.raises(ValueError):
        net(ball, table, torch.ones_like(mask), times)          # all-ones mask (model.py:541-546)
    with pytest.raises(ValueError):
        net(ball, table, torch.zeros_like(mask), times)
    with pytest.raises(ValueError):
        net(ball[:0], table[:0], mask[:0], times[:0])           # B = 0
    long = [torch.from_numpy(a) for a in synth.synth_trajectories(2, 64, seed=9, pad=1)]
    with pytest.raises(ValueError, match='sequence length'):
        net(*long)                                              # 65 > max_len
    rot_, pos_ = net(ball, table, mask, times)
    rot2, pos2 = net(ball[3:7], table[3:7], mask[3:7], times[3:7])
    assert torch.allclose(rot2, rot_[3:7], rtol=1e-5, atol=1e-6) and torch.allclose(pos2, pos_[3:7], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('name,mode,rot', [('connectstage', 'dynamic', 'new'), ('singlestage', 'dynamic', 'old')])
def test_two_chunks_match_one_chunk(name, mode, rot):
    """The chunk loop at small size.  A handle with max_len 4096 holds 2 097 152 // (4096 * 14) = 36 trajectories in its scratch
    (about 7.4 GB), so a batch of 40 runs as 36 + 4 and, being over one chunk, never as a graph; a handle with max_len 16 runs the
    same batch as one chunk.  Both select the same kernels for every row (only the row-tile a trajectory falls in differs), so the
    bar is that of tests/test_fullsize_configs.py for that situation.  'singlestage' / 'old' is the only cover of the position
    head's cls-row strip and of the by-index RoPE table across a chunk boundary."""
    sd = weights.random_uplift_state_dict(17, 'large', name, mode, rot)
    args = [torch.from_numpy(a).cuda() for a in synth.synth_trajectories(40, 9, seed=17, pad=3)]
    assert torch.cuda.current_stream() == torch.cuda.default_stream()
    one = uplift.get_model(name, 'large', mode, rot, state_dict=sd, max_batch=40, max_len=16)
    rot1, pos1 = one(*args)
    two = uplift.get_model(name, 'large', mode, rot, state_dict=sd, max_batch=40, max_len=4096)
    rot2, pos2 = two(*args)
    torch.cuda.synchronize()
    info1, info2 = one.graph_info(), two.graph_info()
    del two
    assert info2['stage_launches'] == 2 * info1['stage_launches'] > 0 and info1['replays'] == info2['replays'] == 0          # two chunks, no graph
    assert rot1.shape == (40, 3) and pos1.shape == (40, 12, 3) and bool(torch.isfinite(rot1).all()) and bool(torch.isfinite(pos1).all())
    assert torch.allclose(rot2, rot1, rtol=2e-6, atol=1e-7) and torch.allclose(pos2, pos1, rtol=2e-6, atol=1e-7)


def test_checkpoint_by_path_serves_a_non_default_variant(golden, tmp_path):
    """load_uplifting_model + process_trajectory_uplifting and UpliftingModel(model_path=...) on a singlestage/stacked/old
    checkpoint: with transform_mode 'local' the spin comes back as predicted (the fixture's `rot`), with 'global' turned into the
    ball's frame (`rot_local`, within the bar amplified by |pos| / |pos[1] - pos[0]| as tests/test_gpu_parity.py does)."""
    g = golden('uplift_family.npz')
    case = 'small_singlestage_stacked_old_T20'
    variant, sd, inputs = load_case(g, case)
    assert variant[1:] == ('singlestage', 'stacked', 'old')
    one = [a[:1] for a in inputs]          # trajectory 0: 17 valid steps, 3 padded
    t_valid = int(one[2].sum())
    rref, pref, lref = g[case + '/rot'][0], g[case + '/pos'][0], g[case + '/rot_local'][0]
    amp = float(np.abs(pref[:2, :2]).max() / np.linalg.norm(pref[1, :2] - pref[0, :2]))
    for transform_mode, spin_ref, tol in (('local', rref, BAR), ('global', lref, 4 * BAR * amp)):
        path = tmp_path / (transform_mode + '.pt')
        write_checkpoint(path, sd, 'singlestage', 'small', 'stacked', 'old', transform_mode)
        model, transform, mode = inference.load_uplifting_model(str(path), max_len=32)
        assert mode == transform_mode and (model.name, model.mode, model.time_rotation, model.size) == ('singlestage', 'stacked', 'old', 'small')
        spin, pos = inference.process_trajectory_uplifting(model, *[torch.from_numpy(a) for a in (one[0], one[1], one[3], one[2])], mode)
        assert pos.shape == (t_valid, 3)
        assert rel(spin, spin_ref) <= tol and rel(pos, pref[:t_valid]) <= BAR
        hub = interface.UpliftingModel(max_len=32, model_path=str(path))
        assert hub.transform_mode == transform_mode
        spin2, pos2 = hub.predict_without_normalization(one[0][0, :t_valid], one[1][0], one[2][0], one[3][0, :t_valid])
        assert pos2.shape == (t_valid, 3)
        assert rel(spin2.cpu().numpy(), spin_ref) <= tol and rel(pos2, pref[:t_valid]) <= BAR
        # predict() normalises pixel coordinates by 2560x1440 first: same result from the same points in pixels
        scale = np.array([2560.0, 1440.0])
        table_px = one[1][0].astype(np.float64).copy(); table_px[:, :2] *= scale
        spin3, pos3 = hub.predict(one[0][0, :t_valid].astype(np.float64) * scale, table_px, one[3][0, :t_valid])
        assert rel(spin3.cpu().numpy(), spin_ref) <= tol + 1e-5 and rel(pos3, pref[:t_valid]) <= BAR
