"""The ViTPose backbone's training-mode forward and its backward on the device (csrc/vitpose_grad.hip) against the
float64 restatement with torch autograd (tests/helpers/vitpose_backbone_ref.py), on the smallest shapes at which its kernels change
form (tests/helpers/vitpose_backbone_cases.py).

Comparison rule (section 29's).  feat and each of the 149 gradients is compared with the restatement in relative L2 and in
max |diff| over the tensor's largest magnitude.  The bar of a tensor is ten times the distance of a float32 CPU run of the same
helper (run here; in relative L2 for the golden cases the recorded distance of the reference's own ViT) from the restatement, never
below 10 * 2^-24 and capped at 1e-4: ten times is the project's allowance for summation order.  A tensor whose float64 value is
identically 0 must be exactly 0.  Measured worst ratios device / float32 per tensor family (MI355X): DESIGN.md section 30."""
import ctypes
import functools
import os
import warnings

import numpy as np
import pytest
import torch

from helpers import vitpose_backbone_cases as cases
from helpers import vitpose_backbone_ref as ref
from upliftingtabletennis_amd import _lib, detect_eval, synth, weights

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vitpose_backbone_grad.npz')
ALLOWANCE, FLOOR, CAP = 10.0, 10.0 * 2.0 ** -24, 1e-4
PREFIX = 'model.backbone.'


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """-> (feat64, grads64, feat32, grads32) of the case: computed once, shared, never written to"""
    x, sd, dfeat = cases.make_case(name)
    s = cases.scales(name, golden())
    return ref.forward_backward(x, sd, dfeat, s, dtype=torch.float64) + ref.forward_backward(x, sd, dfeat, s, dtype=torch.float32)


def make_backbone(name, max_batch=None):
    from upliftingtabletennis_amd.vitpose_backbone import ViTPoseBackbone
    b, hp, wp, c = cases.CASES[name][:4]
    _, sd, _ = cases.make_case(name)
    return ViTPoseBackbone(sd, c, (16 * wp, 16 * hp), max_batch=max_batch or b)


def run_device(name):
    x, _, dfeat = cases.make_case(name)
    s = cases.scales(name, golden())
    net = make_backbone(name)
    feat = net.forward(torch.tensor(x), None if s is None else torch.tensor(s))
    grads = net.backward(torch.tensor(dfeat))
    return net, feat, grads


def bar(d32):
    return min(max(ALLOWANCE * d32, FLOOR), CAP)


@pytest.mark.parametrize('name', list(cases.CASES))
def test_case_against_the_restatement(name):
    feat64, g64, feat32, g32 = oracle(name)
    net, feat, grads = run_device(name)
    assert list(grads) == list(g64) and len(grads) == 149
    want = {'feat': feat64, **g64}
    cpu32 = {'feat': feat32, **g32}
    have = {'feat': feat.double().cpu().numpy(), **{k: v.double().cpu().numpy() for k, v in grads.items()}}
    bad, worst = {}, {}
    for k, w in want.items():
        assert have[k].shape == w.shape, (k, have[k].shape, w.shape)
        assert np.isfinite(have[k]).all(), k
        if not w.any():
            assert not have[k].any(), '%s is identically 0 in float64' % k
            continue
        d32_l2, d32_max = ref.rel_l2(cpu32[k], w), ref.rel_max(cpu32[k], w)
        if name in cases.GOLDEN_CASES:
            d32_l2 = float(golden()['%s/%s/dist' % (name, k[len(PREFIX):] if k != 'feat' else 'feat')])          # the reference's own ViT, recorded
        l2, mx = ref.rel_l2(have[k], w), ref.rel_max(have[k], w)
        fam = ref.family(k)
        worst[fam] = max(worst.get(fam, 0.0), l2 / max(d32_l2, 2.0 ** -24), mx / max(d32_max, 2.0 ** -24))
        if l2 > bar(d32_l2) or mx > bar(d32_max):
            bad[k] = (l2, bar(d32_l2), mx, bar(d32_max))
    for fam, m in sorted(worst.items()):
        print('%s %-24s worst device / float32 %.2f' % (name, fam, m))
    assert not bad, bad
    if cases.CASES[name][5] == 'drop5':          # the dropped block: its twelve gradients are exactly 0 (and the oracle agrees)
        dropped = [k for k in g64 if '.blocks.%d.' % cases.DROPPED_BLOCK in k]
        assert len(dropped) == 12 and not any(g64[k].any() for k in dropped) and not any(bool(grads[k].any()) for k in dropped)


@pytest.mark.parametrize('name,mode', [('g5x13', None), ('g5x13', 'ones'), ('g8x8', None), ('s513', 'ones'), ('g1x1', None)])
def test_feat_is_the_inference_backbone_bit_for_bit(name, mode):
    from upliftingtabletennis_amd.vitpose import ViTPoseNet
    b, hp, wp, c = cases.CASES[name][:4]
    x, sd, _ = cases.make_case(name)
    x = torch.tensor(x)
    want = ViTPoseNet(sd, in_ch=c, out_ch=1, resolution=(16 * wp, 16 * hp), max_batch=b, micro_batch=b).features(x)
    got = make_backbone(name).forward(x, None if mode is None else torch.ones((12, 2, b)))
    assert tuple(got.shape) == (b * hp * wp, 384) and torch.equal(got, want)


def test_two_calls_give_the_same_bits():
    name = 'g3x43'
    x, _, dfeat = cases.make_case(name)
    x, dfeat, s = torch.tensor(x), torch.tensor(dfeat), torch.tensor(cases.scales(name))
    runs = []
    for _ in range(2):
        net = make_backbone(name)
        feat = net.forward(x, s)
        grads = net.backward(dfeat)
        runs.append([feat] + [grads[k] for k in grads])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    # a second backward on the same forward; another forward in between; and a backward after a second forward on the same handle
    again = net.backward(dfeat)
    assert all(torch.equal(again[k], v) for k, v in zip(again, runs[1][1:]))
    net.forward(x, None)
    feat3 = net.forward(x, s)
    third = net.backward(dfeat)
    assert torch.equal(feat3, runs[1][0]) and all(torch.equal(third[k], v) for k, v in zip(third, runs[1][1:]))


def test_batch_composition_is_bit_neutral_for_feat():
    name = 'g2x3_one'
    b, hp, wp = cases.CASES[name][:3]
    x, _, _ = cases.make_case(name)
    x, s = torch.tensor(x), torch.tensor(cases.scales(name))
    net = make_backbone(name)
    whole = net.forward(x, s).clone()
    n = hp * wp
    for i in range(b):
        alone = net.forward(x[i:i + 1], s[:, :, i:i + 1])
        assert torch.equal(alone, whole[i * n:(i + 1) * n]), i


def test_one_token_attention_has_no_dq_and_no_dk():
    """N = 1: the softmax is the constant 1, so dq = dk = 0 exactly and dv = d att"""
    net, _, grads = run_device('g1x1')
    dqkv = net.read_tap('dqkv')
    assert tuple(dqkv.shape) == (1, 1152) and not bool(dqkv[:, :768].any()) and bool(dqkv[:, 768:].any())
    lse, qkv = net.read_tap('lse', 3), net.read_tap('qkv', 3)
    assert tuple(lse.shape) == (1, 12)
    s = (qkv[0, :384].view(12, 32) * (32 ** -0.5) * qkv[0, 384:768].view(12, 32)).double().sum(1)
    assert float((lse[0].double() - s).abs().max()) <= 1e-5 * max(1.0, float(s.abs().max()))
    assert torch.equal(net.read_tap('att', 3), qkv[:, 768:])          # one key: att = v


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


def test_loss_and_grad_is_the_five_steps_by_hand(synthetic_weights):
    from upliftingtabletennis_amd import wasb
    from upliftingtabletennis_amd.interface import BallDetector
    from upliftingtabletennis_amd.vitpose_backbone import ViTPoseBackbone, sample_drop_scale
    from upliftingtabletennis_amd.vitpose_head import ViTPoseHead
    frames = [f for f in synth.synth_frames(4, 360, 640, seed=11)[0]]
    det = BallDetector('vitpose', max_batch=2, dtype='f32')
    triples = [[frames[i], frames[i + 1], frames[i + 2]] for i in range(2)]
    gt, vis = np.array([[400.0, 300.0], [1500.0, 800.0]]), np.array([1, 0])
    before = det.predict(triples)[1]
    drop = sample_drop_scale(2, generator=torch.Generator().manual_seed(5))
    assert bool((drop == 0).any())
    for scale in (None, drop):
        loss, grads = det.loss_and_grad(triples, gt, vis, sigma=6, weighted=True, train=True, drop_scale=scale)
        # by hand
        x = torch.cat([wasb.preprocess_triples(det._upload(t), det.model_resolution) for t in triples])
        backbone = ViTPoseBackbone(det._backbone_state, 9, (det.model.W, det.model.H), max_batch=2)
        feat = backbone.forward(x, scale)
        head = ViTPoseHead(det._head_state, 1, max_rows=feat.shape[0])
        heat = head.forward(feat, (det.model.H // 16, det.model.W // 16), train=True)
        sums, g = detect_eval.heatmap_loss_grad_device(heat, gt.reshape(2, 1, 2), (vis != 0).astype(np.int32).reshape(2, 1), 6, True, (1080, 1920),
                                                       1.0 / (2 * 1080 * 1920))
        want, dfeat = head.backward(g)
        want.update(backbone.backward(dfeat))
        assert loss == detect_eval.loss_from_sums(sums.cpu().numpy(), (1080, 1920))
        assert sorted(grads) == sorted(want) and all(torch.equal(grads[k], want[k]) for k in grads)
        # the 157 keys and shapes are the checkpoint's parameters
        params = {k: tuple(s) for k, s in weights.vitpose_schema(9, 1, det.model_resolution) if not k.endswith(('running_mean', 'running_var'))}
        assert len(grads) == 157 and {k: tuple(v.shape) for k, v in grads.items()} == params
        assert all(bool(torch.isfinite(v).all()) for v in grads.values()) and float(grads[PREFIX + 'patch_embed.proj.weight'].abs().max()) > 0
        if scale is None:          # the head's share is head_loss_and_grad's
            loss_h, grads_h, _ = det.head_loss_and_grad(triples, gt, vis, sigma=6, weighted=True, train=True)
            assert loss_h == loss and all(torch.equal(grads[k], v) for k, v in grads_h.items())
    assert np.array_equal(det.predict(triples)[1], before)          # the detector itself is untouched


def test_table_loss_and_grad(synthetic_weights):
    from upliftingtabletennis_amd.interface import TableDetector
    frames = [f for f in synth.synth_frames(2, 360, 640, seed=12)[0]]
    det = TableDetector('vitpose', max_batch=2, dtype='f32')
    rng = np.random.default_rng(4)
    coords = np.concatenate([np.floor(rng.uniform(50, 1000, (2, 13, 2))), rng.choice([1.0, 1.0, 0.0], (2, 13, 1))], 2)
    loss, grads = det.loss_and_grad(frames, coords, sigma=6)
    loss_h, grads_h, _ = det.head_loss_and_grad(frames, coords, sigma=6)
    assert len(grads) == 157 and tuple(grads[PREFIX + 'patch_embed.proj.weight'].shape) == (384, 3, 16, 16)
    assert loss == loss_h and all(torch.equal(grads[k], v) for k, v in grads_h.items())
    assert all(bool(torch.isfinite(v).all()) for v in grads.values()) and float(grads[PREFIX + 'pos_embed'].abs().max()) > 0


def test_loss_and_grad_refusals(synthetic_weights):
    from upliftingtabletennis_amd.interface import BallDetector, TableDetector
    frames = [f for f in synth.synth_frames(3, 360, 640, seed=11)[0]]
    triples, gt, vis = [frames], np.array([[400.0, 300.0]]), np.array([1])
    with pytest.raises(NotImplementedError):
        BallDetector('wasb', max_batch=2, dtype='f32').loss_and_grad(triples, gt, vis)
    with pytest.raises(NotImplementedError):
        TableDetector('hrnet', max_batch=2, dtype='f32').loss_and_grad(frames[:1], np.zeros((1, 13, 3)))
    with pytest.raises(ValueError, match='f32'):
        BallDetector('vitpose', max_batch=2, dtype='bf16').loss_and_grad(triples, gt, vis)
    with pytest.raises(ValueError, match='drop_scale'):
        BallDetector('vitpose', max_batch=2, dtype='f32').loss_and_grad(triples, gt, vis, drop_scale=torch.ones((12, 2, 2)))


def test_sample_drop_scale():
    from upliftingtabletennis_amd.vitpose_backbone import keep_probabilities, sample_drop_scale
    s = sample_drop_scale(64, generator=torch.Generator().manual_seed(1))
    assert tuple(s.shape) == (12, 2, 64) and s.dtype == torch.float32 and bool((s[0] == 1).all())
    keep = keep_probabilities()
    assert keep[0] == 1.0 and abs(keep[11] - 0.7) < 1e-12
    for i in range(12):
        assert set(s[i].unique().tolist()) <= {0.0, float(np.float32(1.0 / keep[i]))}, i
    assert 0.5 < float((s[11] > 0).float().mean()) < 0.9          # keep 0.7 over 128 draws
    assert torch.equal(s, sample_drop_scale(64, generator=torch.Generator().manual_seed(1)))


def test_refusals():
    from upliftingtabletennis_amd.vitpose_backbone import ViTPoseBackbone, _Ptrs
    name = 'g1x3'
    b, hp, wp, c = cases.CASES[name][:4]
    x, sd, dfeat = cases.make_case(name)
    x, dfeat = torch.tensor(x), torch.tensor(dfeat)
    for bad_c in (0, 17):
        with pytest.raises(ValueError):
            ViTPoseBackbone(sd, bad_c, (16 * wp, 16 * hp))
    with pytest.raises(ValueError):
        ViTPoseBackbone(sd, c, (16 * wp + 8, 16 * hp))
    with pytest.raises(ValueError):
        ViTPoseBackbone({k: v for k, v in sd.items() if 'last_norm.bias' not in k}, c, (16 * wp, 16 * hp))
    net = make_backbone(name)
    assert net.workspace_bytes() > 0
    with pytest.raises(ValueError, match='forward'):
        net.backward(dfeat)
    with pytest.raises(ValueError):
        net.read_tap('x')                                   # nothing has run
    with pytest.raises(ValueError):
        net.forward(torch.cat([x, x]))                      # more samples than the handle was sized for
    for bad in (torch.ones((12, 2, b + 1)), torch.ones((12, b)), torch.ones((11, 2, b))):
        with pytest.raises(ValueError, match='drop_scale'):
            net.forward(x, bad)
    net.forward(x)
    with pytest.raises(ValueError):
        net.backward(dfeat[:-1])
    with pytest.raises(ValueError):
        net.read_tap('nope')
    with pytest.raises(ValueError):
        net.read_tap('x_mid', 12)
    assert sorted(net.state_dict()) == sorted(k for k in sd if '.backbone.' in k)
    # the C boundary itself: every refusal comes back as TTUP_EINVAL, before any device call
    lib = _lib.load()
    h = ctypes.c_void_p()
    for args in ((0, 1, 3, 2), (17, 1, 3, 2), (1, 0, 3, 2), (1, 1, -3, 2), (1, 1, 3, 0), (1, 4096, 4096, 1)):
        assert lib.ttup_vitpose_grad_create(*args, ctypes.byref(h)) == _lib.EINVAL, args
        assert lib.ttup_vitpose_grad_workspace_bytes(*args) == 0
    assert lib.ttup_vitpose_grad_create(1, 1, 3, 2, None) == _lib.EINVAL
    assert lib.ttup_vitpose_grad_workspace_bytes(c, hp, wp, b) == net.workspace_bytes()
    hd, pp, null = net._handle, net._param_ptrs(), _Ptrs()
    xd, fd, sc = x.cuda(), torch.empty((b * hp * wp, 384), device='cuda'), torch.ones((12, 2, b), device='cuda')
    fwd = lib.ttup_vitpose_grad_forward
    assert fwd(None, _lib.ptr(xd), b, ctypes.byref(pp), None, 0, _lib.ptr(fd), None) == _lib.EINVAL
    assert fwd(hd, None, b, ctypes.byref(pp), None, 0, _lib.ptr(fd), None) == _lib.EINVAL
    assert fwd(hd, _lib.ptr(xd), b, ctypes.byref(pp), None, 0, None, None) == _lib.EINVAL
    assert fwd(hd, _lib.ptr(xd), b, ctypes.byref(null), None, 0, _lib.ptr(fd), None) == _lib.EINVAL          # null parameters
    for nb in (0, -1, b + 1):
        assert fwd(hd, _lib.ptr(xd), nb, ctypes.byref(pp), None, 0, _lib.ptr(fd), None) == _lib.EINVAL, nb
    for n in (24 * b - 1, 24 * b + 24, 12 * b):
        assert fwd(hd, _lib.ptr(xd), b, ctypes.byref(pp), _lib.ptr(sc), n, _lib.ptr(fd), None) == _lib.EINVAL, n
    assert fwd(hd, _lib.ptr(xd), b, ctypes.byref(pp), None, 24 * b, _lib.ptr(fd), None) == _lib.EINVAL
    fresh = make_backbone(name)
    bwd = lib.ttup_vitpose_grad_backward
    gd = torch.empty((1 << 20,), device='cuda')
    gg = _Ptrs((ctypes.c_void_p * 149)(*[gd.data_ptr()] * 149))          # a refused call writes nothing
    dd = dfeat.cuda()
    assert bwd(fresh._handle, _lib.ptr(dd), b, ctypes.byref(pp), ctypes.byref(gg), None) == _lib.EINVAL          # no forward yet
    assert bwd(hd, None, b, ctypes.byref(pp), ctypes.byref(gg), None) == _lib.EINVAL
    assert bwd(hd, _lib.ptr(dd), b, ctypes.byref(pp), ctypes.byref(null), None) == _lib.EINVAL          # null outputs
    assert bwd(hd, _lib.ptr(dd), b - 1, ctypes.byref(pp), ctypes.byref(gg), None) == _lib.EINVAL          # another batch
    assert lib.ttup_vitpose_grad_read_tap(hd, b'x', 0, _lib.ptr(fd), 12) == _lib.EINVAL
    assert lib.ttup_vitpose_grad_read_tap(hd, b'x', 13, _lib.ptr(fd), fd.numel() * 4) == _lib.EINVAL
    torch.cuda.synchronize()
