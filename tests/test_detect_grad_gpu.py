"""The gradient of the detectors' heatmap loss on the device (csrc/detect_eval.hip grad_kernel, detect_eval.heatmap_loss_grad,
BallDetector.heatmap_loss_grad / TableDetector.heatmap_loss_grad).

Bars.  Against the float64 restatement every element lies within one fp32 unit in the last place of the restatement's value plus
1e-10 of the tensor's largest |gradient| (the device rounds once, on the store).  Against the reference's fp32 autograd the bar is
`GC.reference_bar`: ten times the largest relative-L2 distance between a reference gradient and the restatement, measured on the CPU
from the fixture alone (9.1e-6, so the bar is 9.1e-5; it may never exceed the project's 1e-4).  Sums are those of the loss pass, bit
for bit."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

from helpers import detect_eval_cases as C
from helpers import detect_grad_cases as GC
from helpers import detect_grad_ref as G
from upliftingtabletennis_amd import _lib, detect_eval, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g(golden):
    return golden('detect_grad.npz')


def bits(t):
    return t.cpu().numpy().tobytes()


def within_one_ulp(have, want):
    """have (float32 from the device) against the float64 restatement: |diff| <= ulp32(want) + 1e-10 max |want|, per element."""
    have = np.asarray(have, np.float64)
    excess = np.abs(have - want) - (GC.ulp32(want) + C.RESTATEMENT_BAR * np.abs(want).max())
    return float(excess.max()), float((np.abs(have - want) / GC.ulp32(want)).max())


@pytest.mark.parametrize('name', GC.GRAD_EDGES)
def test_edges_against_the_restatement(name):
    pred, centres, has, sigma, size = GC.edge(name)
    dev = torch.from_numpy(pred).cuda()
    # the rows / columns the plan marks unread: tests/test_detect_grad_plan_host.py holds G.unread to the plan's empty ranges
    rows, cols = G.unread(size[0], pred.shape[2]), G.unread(size[1], pred.shape[3])
    for weighted in (False, True):
        want = GC.restated_edge(name, weighted)
        sums, grad = detect_eval.heatmap_loss_grad_device(dev, centres, has, sigma, weighted, size)
        assert grad.shape == dev.shape and grad.dtype == torch.float32 and sums.shape == has.shape and sums.dtype == torch.float64
        excess, ulps = within_one_ulp(grad.cpu().numpy(), want)
        print('%s weighted=%d: at most %.3f fp32 ulp from the restatement, max |grad| %.3e' % (name, weighted, ulps, np.abs(want).max()))
        assert excess <= 0
        # the loss pass's sums, bit for bit; a second call, bit for bit
        assert bits(sums) == bits(detect_eval.heatmap_loss_device(dev, centres, has, sigma, weighted, size))
        sums2, grad2 = detect_eval.heatmap_loss_grad_device(dev, centres, has, sigma, weighted, size)
        assert bits(sums2) == bits(sums) and bits(grad2) == bits(grad)
        if name in GC.UNREAD_EDGES:          # what the plan marks unread holds +0.0: every bit clear
            have = grad.cpu().numpy()
            assert (rows.any() and cols.any()) == (name != 'wide')
            assert not have.view(np.uint32)[:, :, rows].any() and not have.view(np.uint32)[:, :, :, cols].any()
            if name in ('wide', 'shrink'):          # and nothing else is 0 (no output index of these two reads a neighbour with weight 0)
                assert have[:, :, ~rows][:, :, :, ~cols].all()
    if name == 'no_target':          # the gradient of a zero target: a Gaussian so far away that its float32 values are all 0
        far = np.full_like(centres, 1e6)
        _, zero = detect_eval.heatmap_loss_grad_device(dev, far, np.ones_like(has), sigma, True, size)
        assert bits(zero) == bits(grad)


@pytest.mark.parametrize('name,key', GC.FIXTURE_CASES)
def test_fixture_against_the_references_autograd(g, name, key):
    bar, loss_bar = GC.reference_bar(g), GC.loss_bar(g)
    pred, centres, has, sigma, size = GC.fixture_inputs(g, name)
    loss, grad = detect_eval.heatmap_loss_grad(pred, centres, has, sigma=sigma, weighted=key == 'weighted', size=size)
    have, ref = grad.cpu().numpy(), g['%s/grad_%s' % (name, key)]
    ref_loss = float(g['%s/loss_%s' % (name, key)])
    excess, ulps = within_one_ulp(have, GC.restated_fixture(g, name, key))
    print('%s %s: relative L2 %.3e from the reference (bar %.3e), %.3f ulp from the restatement; loss %.9g, reference %.9g (bar %.3e)'
          % (name, key, GC.rel_l2(have, ref), bar, ulps, loss, ref_loss, loss_bar))
    assert have.shape == ref.shape and have.dtype == np.float32
    assert GC.rel_l2(have, ref) <= bar and C.rel(loss, ref_loss) <= loss_bar
    assert excess <= 0 and C.rel(loss, GC.restated_loss(g, name, key)) <= C.RESTATEMENT_BAR
    assert loss == detect_eval.heatmap_loss(pred, centres, has, sigma=sigma, weighted=key == 'weighted', size=size)['loss']


def test_scale(g):
    pred, centres, has, sigma, size = GC.fixture_inputs(g, 'table_b')
    mean = 1.0 / (has.size * size[0] * size[1])
    s0, g0 = detect_eval.heatmap_loss_grad_device(pred, centres, has, sigma, True, size)
    s1, g1 = detect_eval.heatmap_loss_grad_device(pred, centres, has, sigma, True, size, scale=mean)
    s2, g2 = detect_eval.heatmap_loss_grad_device(pred, centres, has, sigma, True, size, scale=2 * mean)
    assert bits(g0) == bits(g1) and bits(s0) == bits(s1) == bits(s2)          # scale=None is the element mean; the sums do not depend on it
    assert bits(g2) == bits(2 * g1) and g1.abs().max() > 0
    _, gm = detect_eval.heatmap_loss_grad_device(pred, centres, has, sigma, True, size, scale=-mean)
    assert bits(gm) == bits(-g1)


def test_refusals_leave_the_gradient_untouched():
    """Every refusal of the C entry point with real device buffers: TTUP_EINVAL, and the sentinel-filled gradient is unchanged."""
    lib = _lib.load()
    n, c, h, w, size = 2, 1, 22, 40, (37, 53)
    # pred and grad hold the largest shape asked for below: a refusal that failed would still stay inside them
    pred = torch.zeros((n, c, 22, 9000), dtype=torch.float32, device='cuda')
    centres = torch.zeros((n, c, 2), dtype=torch.float64, device='cuda')
    has = torch.ones((n, c), dtype=torch.int32, device='cuda')
    sums = torch.full((n, c), -7.0, dtype=torch.float64, device='cuda')
    grad = torch.full((n, c, 22, 9000), -7.0, dtype=torch.float32, device='cuda')
    need = int(lib.ttup_detect_loss_grad_workspace_bytes(n * c, h, w, *size))
    ws = torch.zeros((need // 8 + 2,), dtype=torch.float64, device='cuda')
    P = _lib.ptr

    def call(pred_p=P(pred), centres_p=P(centres), has_p=P(has), n=n, c=c, h=h, w=w, sigma=6.0, size=size, scale=1e-3, ws_p=P(ws), nbytes=need, sums_p=P(sums),
             grad_p=P(grad)):
        return lib.ttup_detect_heatmap_loss_grad(pred_p, centres_p, has_p, n, c, h, w, sigma, size[0], size[1], 1, scale, ws_p, nbytes, sums_p, grad_p, _lib.stream_ptr())

    refusals = [dict(pred_p=None), dict(centres_p=None), dict(has_p=None), dict(ws_p=None), dict(grad_p=None),
                dict(n=0), dict(n=-1), dict(c=0), dict(h=0), dict(w=0), dict(size=(0, 53)), dict(size=(37, 0)), dict(size=(-1, 53)),
                dict(sigma=0.0), dict(sigma=-2.0), dict(sigma=float('nan')),
                dict(scale=float('inf')), dict(scale=float('-inf')), dict(scale=float('nan')),
                dict(h=2, w=7681), dict(h=22, w=9000),          # two source rows beyond the 60 KB of LDS the loss pass keeps them in
                dict(nbytes=need - 1), dict(nbytes=0), dict(ws_p=ctypes.c_void_p(ws.data_ptr() + 4))]
    for kw in refusals:
        assert call(**kw) == _lib.EINVAL and lib.ttup_last_error(), kw
    torch.cuda.synchronize()
    assert bool((grad == -7.0).all()) and bool((sums == -7.0).all())
    # the same buffers are served once the arguments are right; sums_dev may be null: no sums wanted
    assert call(sums_p=None) == _lib.OK
    torch.cuda.synchronize()
    assert bool((sums == -7.0).all()) and not bool((grad.reshape(-1)[:n * c * h * w] == -7.0).any()) and bool((grad.reshape(-1)[n * c * h * w:] == -7.0).all())


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


N_FRAMES = 5


@pytest.fixture(scope='module')
def frames():
    return [f for f in synth.synth_frames(N_FRAMES, 720, 1280, seed=11)[0]]


@pytest.mark.parametrize('model_name', ['wasb', 'vitpose'])
def test_ball_detector_surface_is_forward_then_the_function(synthetic_weights, frames, model_name):
    """max_batch 2 on three triples: two chunks, the second not full, each with the whole batch's scale."""
    from upliftingtabletennis_amd.interface import BallDetector
    det = BallDetector(model_name, max_batch=2, dtype='f32')
    triples = [[frames[i], frames[i + 1], frames[i + 2]] for i in range(N_FRAMES - 2)]
    n = len(triples)
    rng = np.random.default_rng(3)
    gt = np.stack([rng.uniform(100, 1800, n), rng.uniform(100, 1000, n)], 1)
    vis = np.array([1, 0, 1])
    heat = det.predict(triples)[1]
    for weighted in (True, False):
        loss, grad = det.heatmap_loss_grad(triples, gt, vis, sigma=6, weighted=weighted)
        want_loss, want = detect_eval.heatmap_loss_grad(heat, gt.reshape(n, 1, 2), (vis != 0).reshape(n, 1), sigma=6, weighted=weighted)
        assert grad.is_cuda and tuple(grad.shape) == heat.shape and bits(grad) == bits(want) and loss == want_loss
        assert loss == detect_eval.heatmap_loss(heat, gt.reshape(n, 1, 2), (vis != 0).reshape(n, 1), sigma=6, weighted=weighted)['loss']
        assert float(grad.abs().max()) > 0
    assert loss == det.val(triples, gt, gt, gt, vis, sigma=6)['loss']          # the ball val()'s loss is the unweighted one
    assert np.array_equal(det.predict(triples)[1], heat)          # predict returns what it returned before


def test_table_detector_surface_is_forward_then_the_function(synthetic_weights, frames):
    from upliftingtabletennis_amd.interface import TableDetector
    det = TableDetector('hrnet', max_batch=2, dtype='f32')
    images = frames[:3]
    rng = np.random.default_rng(4)
    coords = np.concatenate([np.floor(rng.uniform(50, 1000, (3, 13, 2))), rng.choice([1.0, 1.0, 0.0], (3, 13, 1))], 2)
    heat = det.predict(images)[1][:, 0]
    for weighted in (True, False):
        loss, grad = det.heatmap_loss_grad(images, coords, sigma=6, weighted=weighted)
        want_loss, want = detect_eval.heatmap_loss_grad(heat, coords[..., :2], coords[..., 2] == 1, sigma=6, weighted=weighted)
        assert grad.is_cuda and tuple(grad.shape) == heat.shape and bits(grad) == bits(want) and loss == want_loss
        assert loss == detect_eval.heatmap_loss(heat, coords[..., :2], coords[..., 2] == 1, sigma=6, weighted=weighted)['loss']
        if weighted:
            assert loss == det.val(images, coords, sigma=6)['loss']          # the table val()'s loss is the weighted one
