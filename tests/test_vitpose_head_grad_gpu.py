"""The ViTPose head's training-mode forward and its backward on the device (csrc/vitpose_head_grad.hip) against
the float64 restatement (tests/helpers/vitpose_head_ref.py), on the smallest shapes at which its kernels change form
(tests/helpers/vitpose_head_cases.py).

Comparison rule.  Every tensor -- heat, the running statistics, the eight parameter gradients, dfeat -- is compared with the
restatement in relative L2 and in max |diff| over the tensor's largest magnitude.  The bar of a tensor is ten times the distance of
a float32 CPU run of the same definition (torch's operators with autograd, run here; for the golden cases the recorded distance of
the reference's own head) from the restatement, capped at 1e-4: ten times is the project's allowance for summation order.
Measured worst ratio device / float32 over all cases and tensors (MI355X): see DESIGN.md section 29.

ReLU gates.  An element is undecided where the restatement has |y| <= 1e-4 (|gamma| + |beta|); there the restatement's backward
takes the gate the device took (read_tap a1 / a2 > 0), everywhere else the device's gate must equal the float64 gate exactly."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from helpers import vitpose_head_cases as cases
from helpers import vitpose_head_ref as ref
from upliftingtabletennis_amd import _lib, detect_eval, synth, weights

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vitpose_head_grad.npz')
ALLOWANCE, CAP = 10.0, 1e-4
FOLDED_BAR = 5.3e-6          # the folded inference forward's own bar, of the heatmap range
PREFIX = 'model.keypoint_head.'
KEYS = {'W1': 'deconv_layers.0.weight', 'g1': 'deconv_layers.1.weight', 'b1': 'deconv_layers.1.bias', 'rm1': 'deconv_layers.1.running_mean',
        'rv1': 'deconv_layers.1.running_var', 'W2': 'deconv_layers.3.weight', 'g2': 'deconv_layers.4.weight', 'b2': 'deconv_layers.4.bias',
        'rm2': 'deconv_layers.4.running_mean', 'rv2': 'deconv_layers.4.running_var', 'Wf': 'final_layer.weight', 'bf': 'final_layer.bias'}


def state_dict(p):
    sd = {PREFIX + KEYS[k]: np.asarray(v, np.float32) for k, v in p.items()}
    sd[PREFIX + KEYS['Wf']] = sd[PREFIX + KEYS['Wf']][:, :, None, None]
    return sd


def make_head(name, max_rows=None):
    from upliftingtabletennis_amd.vitpose_head import ViTPoseHead
    _, p, _ = cases.make_case(name)
    return ViTPoseHead(state_dict(p), cases.CASES[name][3], max_rows=max_rows or cases.tokens(name))


def nchw(t):
    return t.double().cpu().numpy().transpose(0, 3, 1, 2)


def run_device(name):
    """One forward + backward of the case -> (head, heat, grads by short name incl. 'feat', gates (a1 > 0, a2 > 0) NCHW)"""
    b, hp, wp, c, _, train = cases.CASES[name]
    feat, p, dheat = cases.make_case(name)
    head = make_head(name)
    heat = head.forward(torch.tensor(feat, dtype=torch.float32), (hp, wp), train=train)
    grads, dfeat = head.backward(torch.tensor(dheat, dtype=torch.float32))
    out = {k: grads[PREFIX + KEYS[k]].double().cpu().numpy() for k in ref.GRADS}
    out['Wf'] = out['Wf'][:, :, 0, 0]
    out['feat'] = dfeat.double().cpu().numpy()
    return head, heat.double().cpu().numpy(), out, (nchw(head.read_tap('a1')) > 0, nchw(head.read_tap('a2')) > 0)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize('name', list(cases.CASES))
def test_case_against_the_restatement(golden, name):
    b, hp, wp, c, _, train = cases.CASES[name]
    feat, p, dheat = cases.make_case(name)
    f = ref.forward(feat, p, train)
    head, heat, got, (gate1, gate2) = run_device(name)

    # gates: exact where float32 can be held to them, the device's own where it cannot
    u1, u2 = ref.undecided(f, p)
    assert u1.mean() <= 1e-3 and u2.mean() <= 1e-3
    assert np.array_equal(gate1[~u1], (f['y1'] > 0)[~u1]) and np.array_equal(gate2[~u2], (f['y2'] > 0)[~u2])
    g = ref.backward(f, p, dheat, train, np.where(u1, gate1, f['y1'] > 0), np.where(u2, gate2, f['y2'] > 0))

    # what float32 costs on this case
    heat32, run32, grads32 = ref.torch_reference(feat, p, dheat, train, torch.float32)
    want = {'heat': f['heat'], 'rm1': f['rm1'], 'rv1': f['rv1'], 'rm2': f['rm2'], 'rv2': f['rv2']}
    want.update({'d' + k: g[k] for k in g})
    cpu32 = {'heat': heat32, **run32, **{'d' + k: v for k, v in grads32.items()}}
    sd = head.state_dict()
    have = {'heat': heat, **{k: sd[PREFIX + KEYS[k]].double().cpu().numpy() for k in ('rm1', 'rv1', 'rm2', 'rv2')}, **{'d' + k: v for k, v in got.items()}}
    worst = {}
    for k, w in want.items():
        assert have[k].shape == w.shape, (k, have[k].shape, w.shape)
        d32_l2, d32_max = ref.rel_l2(cpu32[k], w), ref.rel_max(cpu32[k], w)
        if name in cases.GOLDEN_CASES:
            d32_l2 = float(golden['%s/%s/dist' % (name, k)])          # the reference's own head, recorded
        l2, mx = ref.rel_l2(have[k], w), ref.rel_max(have[k], w)
        bar_l2, bar_max = min(ALLOWANCE * d32_l2, CAP), min(ALLOWANCE * d32_max, CAP)
        print('%s %-5s l2 %.3g (float32 %.3g, bar %.3g)  max %.3g (float32 %.3g, bar %.3g)' % (name, k, l2, d32_l2, bar_l2, mx, d32_max, bar_max))
        worst[k] = (l2, bar_l2, mx, bar_max)
    bad = {k: v for k, v in worst.items() if v[0] > v[1] or v[2] > v[3]}
    assert not bad, bad

    # the statistics the BN used, and the running statistics' bookkeeping
    for l in ('1', '2'):
        for s in ('mean', 'var'):
            have_s = head.read_tap(s + l).double().cpu().numpy()
            assert ref.rel_max(have_s, f[s + l]) <= CAP, (s + l, ref.rel_max(have_s, f[s + l]))
        assert int(sd[PREFIX + 'deconv_layers.%d.num_batches_tracked' % (1 if l == '1' else 4)]) == (1 if train else 0)
    # the special channels: exact zeros
    z1 = nchw(head.read_tap('z1'))
    assert not z1[:, cases.ZERO_CH].any()
    if train:
        assert float(head.read_tap('var1')[cases.ZERO_CH]) == 0.0
    for l, ch in (('1', cases.DEAD1), ('2', cases.DEAD2)):
        assert got['g' + l][ch] == 0 and got['b' + l][ch] == 0 and not got['W' + l][:, ch].any(), l


def test_two_calls_give_the_same_bits():
    name = 'g5x7'
    b, hp, wp, c, _, train = cases.CASES[name]
    feat, p, dheat = cases.make_case(name)
    runs = []
    for _ in range(2):
        head = make_head(name)
        heat = head.forward(torch.tensor(feat, dtype=torch.float32), (hp, wp), train=True)
        grads, dfeat = head.backward(torch.tensor(dheat, dtype=torch.float32))
        runs.append([heat, dfeat] + [grads[k] for k in sorted(grads)] + [v for k, v in sorted(head.state_dict().items())])
    # and a second backward on the same forward, and a second forward on the same handle (the running statistics move on; nothing else does)
    grads2, dfeat2 = head.backward(torch.tensor(dheat, dtype=torch.float32))
    heat3 = head.forward(torch.tensor(feat, dtype=torch.float32), (hp, wp), train=True)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert torch.equal(dfeat2, runs[1][1]) and all(torch.equal(grads2[k], v) for k, v in zip(sorted(grads2), runs[1][2:]))
    assert torch.equal(heat3, runs[1][0])
    assert int(head.state_dict()[PREFIX + 'deconv_layers.1.num_batches_tracked']) == 2


def test_nchw_features_give_nchw_gradient():
    name = 'g1x3'
    b, hp, wp, c, _, _ = cases.CASES[name]
    feat, p, dheat = cases.make_case(name)
    x = torch.tensor(feat, dtype=torch.float32)
    head = make_head(name)
    heat_a = head.forward(x, (hp, wp))
    dfeat_a = head.backward(torch.tensor(dheat, dtype=torch.float32))[1]
    head = make_head(name)
    heat_b = head.forward(x.permute(0, 2, 3, 1).reshape(-1, 384), (hp, wp))
    dfeat_b = head.backward(torch.tensor(dheat, dtype=torch.float32))[1]
    assert tuple(dfeat_a.shape) == tuple(x.shape) and tuple(dfeat_b.shape) == (b * hp * wp, 384)
    assert torch.equal(heat_a, heat_b) and torch.equal(dfeat_a.permute(0, 2, 3, 1).reshape(-1, 384), dfeat_b)


@pytest.mark.parametrize('name', ['g2x2_eval', 'g5x7_eval'])
def test_eval_mode_is_the_folded_inference_head(name):
    """train=False on last_norm's output as the inference handle leaves it ('ln' tap of stage 13) against that handle's own
    BN-folded head ('heat' tap), within the folded forward's bar of the heatmap range"""
    from upliftingtabletennis_amd.vitpose import ViTPoseNet
    b, hp, wp, c, seed, _ = cases.CASES[name]
    _, p, _ = cases.make_case(name)
    sd = weights.random_vitpose_state_dict(seed, in_ch=3, out_ch=c, resolution=(16 * wp, 16 * hp), planted=False)
    sd.update(state_dict(p))
    net = ViTPoseNet(sd, in_ch=3, out_ch=c, resolution=(16 * wp, 16 * hp), max_batch=b, micro_batch=b)
    x = torch.tensor(np.random.default_rng(seed).standard_normal((b * hp * wp, 384)), dtype=torch.float32)
    net.run_stage(13, x)
    feat, folded = net.read_tap('ln'), net.read_tap('heat')
    head = make_head(name)
    heat = head.forward(feat, (hp, wp), train=False)
    rng = float(folded.max() - folded.min())
    err = float((heat - folded).abs().max())
    print(name, 'max |diff| / range', err / rng)
    assert err <= FOLDED_BAR * rng, (err, rng)


def test_features_is_the_ln_tap_bit_for_bit():
    """a 2x3-token handle, three samples in micro-batches of two, against the stages chained by hand per micro-batch"""
    from upliftingtabletennis_amd.vitpose import ViTPoseNet
    h, w = 32, 48
    sd = weights.random_vitpose_state_dict(5, in_ch=3, out_ch=2, resolution=(w, h), planted=False)
    net = ViTPoseNet(sd, in_ch=3, out_ch=2, resolution=(w, h), max_batch=4, micro_batch=2)
    x = torch.tensor(np.random.default_rng(6).standard_normal((3, 3, h, w)), dtype=torch.float32)
    got = net.features(x)
    want = []
    for b0 in (0, 2):
        net.run_stage(0, x[b0:b0 + 2])
        s = net.read_tap('x')
        for stage in range(1, 13):
            net.run_stage(stage, s)
            s = net.read_tap('x')
        net.run_stage(13, s)
        want.append(net.read_tap('ln'))
    want = torch.cat(want)
    assert tuple(got.shape) == (3 * 6, 384) and torch.equal(got, want)
    assert torch.equal(net.features(x), got)
    bf = ViTPoseNet(sd, in_ch=3, out_ch=2, resolution=(w, h), max_batch=2, dtype='bf16')
    with pytest.raises(ValueError, match='f32'):
        bf.features(x[:1])


@pytest.fixture(scope='module')
def synthetic_weights():
    old = os.environ.get('TTUP_SYNTHETIC_WEIGHTS')
    os.environ['TTUP_SYNTHETIC_WEIGHTS'] = '1'
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        yield
    if old is None:
        os.environ.pop('TTUP_SYNTHETIC_WEIGHTS', None)
    else:
        os.environ['TTUP_SYNTHETIC_WEIGHTS'] = old


def test_head_loss_and_grad_is_the_four_steps_by_hand(synthetic_weights):
    from upliftingtabletennis_amd import wasb
    from upliftingtabletennis_amd.interface import BallDetector, TableDetector
    from upliftingtabletennis_amd.vitpose_head import ViTPoseHead
    frames = [f for f in synth.synth_frames(4, 360, 640, seed=11)[0]]
    det = BallDetector('vitpose', max_batch=2, dtype='f32')
    triples = [[frames[i], frames[i + 1], frames[i + 2]] for i in range(2)]
    gt, vis = np.array([[400.0, 300.0], [1500.0, 800.0]]), np.array([1, 0])
    before = det.predict(triples)[1]
    for train in (True, False):
        loss, grads, dfeat = det.head_loss_and_grad(triples, gt, vis, sigma=6, weighted=True, train=train)
        # by hand
        x = torch.cat([wasb.preprocess_triples(det._upload(t), det.model_resolution) for t in triples])
        feat = det.model.features(x)
        head = ViTPoseHead(det._head_state, 1, max_rows=feat.shape[0])
        heat = head.forward(feat, (det.model.H // 16, det.model.W // 16), train=train)
        sums, g = detect_eval.heatmap_loss_grad_device(heat, gt.reshape(2, 1, 2), (vis != 0).astype(np.int32).reshape(2, 1), 6, True, (1080, 1920),
                                                       1.0 / (2 * 1080 * 1920))
        want_grads, want_dfeat = head.backward(g)
        assert loss == detect_eval.loss_from_sums(sums.cpu().numpy(), (1080, 1920))
        assert sorted(grads) == sorted(want_grads) and all(torch.equal(grads[k], want_grads[k]) for k in grads)
        assert torch.equal(dfeat, want_dfeat) and tuple(dfeat.shape) == (2 * 40 * 72, 384) and float(dfeat.abs().max()) > 0
        if not train:          # the running statistics: heat is the detector's own heatmap within the folded forward's bar
            rng = float(before.max() - before.min())
            assert float((heat.cpu() - torch.tensor(before)).abs().max()) <= FOLDED_BAR * rng
    assert np.array_equal(det.predict(triples)[1], before)          # the detector itself is untouched


def test_head_loss_and_grad_refusals(synthetic_weights):
    from upliftingtabletennis_amd.interface import BallDetector, TableDetector
    frames = [f for f in synth.synth_frames(3, 360, 640, seed=11)[0]]
    triples, gt, vis = [frames], np.array([[400.0, 300.0]]), np.array([1])
    with pytest.raises(NotImplementedError):
        BallDetector('wasb', max_batch=2, dtype='f32').head_loss_and_grad(triples, gt, vis)
    with pytest.raises(NotImplementedError):
        TableDetector('hrnet', max_batch=2, dtype='f32').head_loss_and_grad(frames[:1], np.zeros((1, 13, 3)))
    with pytest.raises(ValueError, match='f32'):
        BallDetector('vitpose', max_batch=2, dtype='bf16').head_loss_and_grad(triples, gt, vis)


def test_table_head_loss_and_grad(synthetic_weights):
    from upliftingtabletennis_amd.interface import TableDetector
    frames = [f for f in synth.synth_frames(2, 360, 640, seed=12)[0]]
    det = TableDetector('vitpose', max_batch=2, dtype='f32')
    rng = np.random.default_rng(4)
    coords = np.concatenate([np.floor(rng.uniform(50, 1000, (2, 13, 2))), rng.choice([1.0, 1.0, 0.0], (2, 13, 1))], 2)
    loss, grads, dfeat = det.head_loss_and_grad(frames, coords, sigma=6)
    loss2, grad_heat = det.heatmap_loss_grad(frames, coords, sigma=6)
    assert len(grads) == 8 and tuple(grads[PREFIX + 'final_layer.weight'].shape) == (13, 256, 1, 1) and tuple(dfeat.shape) == (2 * 40 * 72, 384)
    assert all(bool(torch.isfinite(v).all()) for v in grads.values()) and float(dfeat.abs().max()) > 0
    assert np.isfinite(loss) and loss > 0 and loss != loss2          # batch statistics: not the inference heatmaps' loss


def test_refusals():
    from upliftingtabletennis_amd.vitpose_head import ViTPoseHead
    name = 'g2x2'
    b, hp, wp, c, _, _ = cases.CASES[name]
    feat, p, dheat = cases.make_case(name)
    sd = state_dict(p)
    x = torch.tensor(feat, dtype=torch.float32)
    for bad_c in (0, 17):
        with pytest.raises(ValueError):
            ViTPoseHead(sd, bad_c)
    head = make_head(name)
    with pytest.raises(ValueError, match='forward'):
        head.backward(torch.zeros((b, c, 4 * hp, 4 * wp)))
    for grid in ((0, 2), (2, -1)):
        with pytest.raises(ValueError):
            head.forward(x, grid)
    with pytest.raises(ValueError):
        head.forward(torch.cat([x, x]), (hp, wp))          # rows beyond what the handle was sized for
    with pytest.raises(ValueError):
        head.read_tap('z1')                                 # nothing has run
    head.forward(x, (hp, wp))
    with pytest.raises(ValueError):
        head.backward(torch.zeros((b - 1, c, 4 * hp, 4 * wp)))          # another batch than the forward's
    with pytest.raises(ValueError):
        head.read_tap('nope')
    # the C boundary itself: every refusal comes back as TTUP_EINVAL
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.ttup_vitpose_head_create(0, 8, ctypes.byref(h)) == _lib.EINVAL and lib.ttup_vitpose_head_create(17, 8, ctypes.byref(h)) == _lib.EINVAL
    assert lib.ttup_vitpose_head_create(1, 0, ctypes.byref(h)) == _lib.EINVAL and lib.ttup_vitpose_head_create(1, 8, None) == _lib.EINVAL
    assert lib.ttup_vitpose_head_workspace_bytes(0, 8) == 0 and lib.ttup_vitpose_head_workspace_bytes(1, 8) == head._lib.ttup_vitpose_head_workspace_bytes(1, 8) > 0
    from upliftingtabletennis_amd.vitpose_head import _Grads, _Params
    pp, gg = _Params(), _Grads()
    hd = head._handle
    assert lib.ttup_vitpose_head_forward(None, _lib.ptr(x), b, hp, wp, ctypes.byref(pp), 1, _lib.ptr(x), None) == _lib.EINVAL
    assert lib.ttup_vitpose_head_forward(hd, None, b, hp, wp, ctypes.byref(pp), 1, _lib.ptr(x), None) == _lib.EINVAL
    assert lib.ttup_vitpose_head_forward(hd, _lib.ptr(x), b, hp, wp, ctypes.byref(pp), 1, _lib.ptr(x), None) == _lib.EINVAL          # null parameters
    assert lib.ttup_vitpose_head_backward(hd, None, b, hp, wp, ctypes.byref(gg), None) == _lib.EINVAL
    assert lib.ttup_vitpose_head_backward(hd, _lib.ptr(x), b, hp, wp, ctypes.byref(gg), None) == _lib.EINVAL          # null outputs
    d = torch.zeros((b, c, 4 * hp, 4 * wp), device='cuda')
    outs = [torch.empty(16 * 384 * 256, device='cuda') for _ in range(9)]
    gg = _Grads(*[t.data_ptr() for t in outs])
    for args in ((b + 1, hp, wp), (b, wp + 1, hp), (b, hp, wp + 1), (0, hp, wp)):
        assert lib.ttup_vitpose_head_backward(hd, _lib.ptr(d), *args, ctypes.byref(gg), None) == _lib.EINVAL, args
    assert lib.ttup_vitpose_head_backward(hd, _lib.ptr(d), b, hp, wp, ctypes.byref(gg), _lib.stream_ptr()) == _lib.OK
    assert lib.ttup_vitpose_head_read_tap(hd, b'z1', _lib.ptr(outs[0]), 12) == _lib.EINVAL
    torch.cuda.synchronize()
