"""The gradient of the detectors' heatmap loss without a GPU: the float64 restatement (tests/helpers/detect_grad_ref.py) against what
the reference's autograd returned on recorded heatmaps (tests/golden/detect_grad.npz, tools/make_goldens_detect_grad.py) and against
torch's float64 autograd through F.interpolate on every LOSS_EDGES shape and two more downsampling shapes; the fixture's conditions; the C-ABI's argument checks.

Measured here (printed by test_reference_rounding_sets_the_gpu_bar): the reference's fp32 gradients lie within 9.1e-6 relative L2 of
the restatement (1.0e-6 .. 2.4e-6 at 1080x1920, 9.1e-6 on the (44, 80) -> (135, 241) ball: torch's fp32 kernels hold the source
coordinate and lambda in fp32 too), so the GPU test's bar against the reference is 9.1e-5 (ten times that, under the 1e-4 cap)."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from upliftingtabletennis_amd import _lib, detect_eval
from helpers import detect_eval_cases as C
from helpers import detect_eval_ref as R
from helpers import detect_grad_cases as GC
from helpers import detect_grad_ref as G

NEW_SYMBOLS = ('ttup_detect_loss_grad_workspace_bytes', 'ttup_detect_heatmap_loss_grad')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def g(golden):
    return golden('detect_grad.npz')


def test_fixture_meets_its_conditions(g):
    assert float(g['target_margin']) >= 1e-6
    for name, key in GC.FIXTURE_CASES:
        GC.restated_loss(g, name, key)
        assert GC._cache[('loss', name)]['margin'] >= 1e-6, name          # no weight can flip between fp32 and fp64 evaluation of the target
        assert g['%s/grad_%s' % (name, key)].dtype == np.float32 and g['%s/grad_%s' % (name, key)].shape == GC.fixture_inputs(g, name)[0].shape
    # what the kernel must serve: two heatmap sizes, two output sizes (one small and odd), a ball without target, a ball outside the
    # image, keypoints without target
    assert g['ball_a/pred'].shape == (3, 1, 22, 40) and g['ball_b/pred'].shape == (1, 1, 44, 80) and g['table_a/pred'].shape == (1, 13, 22, 40)
    assert tuple(g['ball_a/size']) == tuple(g['table_a/size']) == (1080, 1920) and tuple(g['ball_b/size']) == tuple(g['table_b/size']) == (135, 241)
    assert g['ball_a/vis'][1] == 0 and g['ball_a/gt'][2, 0] > 1920 and g['ball_a/gt'][2, 1] < 0
    assert (g['table_a/gt'][..., 2] == 0).sum() == 2 and (g['table_b/gt'][..., 2] == 0).sum() == 2


@pytest.mark.parametrize('name,key', GC.FIXTURE_CASES)
def test_restatement_reproduces_the_references_gradients(g, name, key):
    want = g['%s/grad_%s' % (name, key)]
    have = GC.restated_fixture(g, name, key)
    print('%s %s: relative L2 %.3e, max |diff| / max |grad| %.3e' % (name, key, GC.rel_l2(want, have), np.abs(want - have).max() / np.abs(have).max()))
    assert GC.rel_l2(want, have) <= C.PARITY_BAR
    assert C.rel(GC.restated_loss(g, name, key), float(g['%s/loss_%s' % (name, key)])) <= C.PARITY_BAR
    pred, centres, has, sigma, size = GC.fixture_inputs(g, name)
    for i, j in zip(*np.nonzero(has == 0)):          # without target the gradient is that of up(pred)^2, weighted or not
        zero = G.heatmap_loss_grad(pred[i:i + 1, j:j + 1], [[(0.0, 0.0)]], [[0]], sigma, False, size, scale=1.0 / (has.size * size[0] * size[1]))
        assert np.array_equal(have[i, j], zero[0, 0])


def test_reference_rounding_sets_the_gpu_bar(g):
    worst = GC.reference_rounding(g)
    print('reference fp32 gradients against the float64 restatement: %.3e relative L2 -> bar %.3e; losses: bar %.3e' % (worst, GC.reference_bar(g), GC.loss_bar(g)))
    assert 0 < worst <= C.PARITY_BAR / 10          # ten times the rounding stays under the parity cap: the bar is the measured one
    assert GC.reference_bar(g) == 10 * worst and 0 < GC.loss_bar(g) <= C.PARITY_BAR


def torch_grad(pred, centres, has, sigma, weighted, size):
    """torch's float64 autograd through F.interpolate and the loss (element mean), against the restatement's float32 target."""
    p = torch.from_numpy(np.asarray(pred, np.float32).astype(np.float64)).requires_grad_(True)
    n, c = p.shape[:2]
    t = np.zeros((n, c) + tuple(size), np.float32)
    for i in range(n):
        for j in range(c):
            if has[i][j]:
                t[i, j] = R.target(centres[i][j], sigma, size)
    wgt = np.where(t > np.float32(0.1), 100.0, 1.0) if weighted else np.ones(t.shape)
    up = F.interpolate(p, size=tuple(size), mode='bilinear')
    (torch.from_numpy(wgt) * (up - torch.from_numpy(t.astype(np.float64))) ** 2).mean().backward()
    return p.grad.numpy()


@pytest.mark.parametrize('name', GC.GRAD_EDGES)
def test_restatement_against_torch_float64_autograd(name):
    pred, centres, has, sigma, size = GC.edge(name)
    if name in GC.SKIP_EDGES:          # (the LOSS_EDGES cases' margins: tests/test_detect_eval_gpu.py)
        assert R.heatmap_loss_sums_both(pred, centres, has, sigma, size)[2] >= 1e-6          # no weight can flip between two evaluations of the target
    for weighted in (False, True):
        have, want = GC.restated_edge(name, weighted), torch_grad(pred, centres, has, sigma, weighted, size)
        err = np.abs(have - want).max() / np.abs(want).max()
        print('%s weighted=%d: max |diff| / max |grad| %.3e' % (name, weighted, err))
        assert have.shape == want.shape == pred.shape and err <= C.RESTATEMENT_BAR
    if name in GC.UNREAD_EDGES:          # a source row / column nothing reads has no gradient
        rows, cols = G.unread(size[0], pred.shape[2]), G.unread(size[1], pred.shape[3])
        assert (rows.any() and cols.any()) == (name != 'wide')          # (wide: 2048 -> 1920 still reads every column, some with one neighbour's weight alone)
        assert not have[:, :, rows].any() and not have[:, :, :, cols].any() and not want[:, :, rows].any() and not want[:, :, :, cols].any()


def test_read_weights_are_the_interpolation():
    """a^T applied from the left and b from the right IS the upsampling: the gradient's weights are the forward's, transposed."""
    rng = np.random.default_rng(2)
    for (h, w), size in (((22, 40), (37, 53)), ((64, 50), (7, 9)), ((1, 7), (5, 30)), ((9, 9), (9, 9))):
        p = rng.normal(0, 1, (h, w)).astype(np.float32)
        a, b = G.read_weights(size[0], h), G.read_weights(size[1], w)
        assert np.allclose(a.sum(1), 1.0, rtol=0, atol=3e-16) and np.allclose(b.sum(1), 1.0, rtol=0, atol=3e-16)
        assert np.abs(a @ p.astype(np.float64) @ b.T - R.upsample(p, size)).max() <= 1e-14
        assert (a[:, G.unread(size[0], h)] == 0).all() and (b[:, G.unread(size[1], w)] == 0).all()


def test_python_surface():
    from upliftingtabletennis_amd import interface, wasb
    for mod in (interface, wasb):
        assert mod.heatmap_loss_grad is detect_eval.heatmap_loss_grad and mod.heatmap_loss_grad_device is detect_eval.heatmap_loss_grad_device
    for cls in (interface.BallDetector, interface.TableDetector, interface.ViTPoseBallDetector, interface.ViTPoseTableDetector):
        assert callable(cls.heatmap_loss_grad)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from upliftingtabletennis_amd import build
        build.build()
    return _lib.load()


def test_new_symbols_are_declared_bound_and_built(lib):
    hdr = open(os.path.join(ROOT, 'include', 'ttup.h')).read()
    for name in NEW_SYMBOLS:
        assert name + '(' in hdr and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.ttup_detect_loss_grad_workspace_bytes(0, 22, 40, 1080, 1920) == 0 and lib.ttup_detect_loss_grad_workspace_bytes(2, 0, 40, 1080, 1920) == 0
    assert lib.ttup_detect_loss_grad_workspace_bytes(2, 22, 40, 0, 1920) == 0
    assert lib.ttup_detect_loss_grad_workspace_bytes(3, 22, 40, 1080, 1920) >= 3 * (1080 + 1920) * 8          # the Gaussian factors of every map at least


def test_new_symbols_refuse_bad_arguments_before_any_device_call(lib):
    """Every refusal is TTUP_EINVAL with a message; this machine may have no device at all.  The non-null pointers are host
    addresses nothing dereferences: the checks come first."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    big = 1 << 30

    def grad(ptrs, n=2, c=1, h=22, w=40, sigma=6.0, size=(1080, 1920), scale=1e-6, ws=p, nbytes=big, sums=p, out=p):
        return lib.ttup_detect_heatmap_loss_grad(*ptrs, n, c, h, w, sigma, size[0], size[1], 1, scale, ws, nbytes, sums, out, None)

    for hole in range(3):
        assert grad([None if i == hole else p for i in range(3)]) == _lib.EINVAL and b'null pointer' in lib.ttup_last_error()
    assert grad([p] * 3, ws=None) == _lib.EINVAL and b'null pointer' in lib.ttup_last_error()
    assert grad([p] * 3, out=None) == _lib.EINVAL and b'null pointer' in lib.ttup_last_error()
    for kw in (dict(n=0), dict(n=-1), dict(c=0), dict(h=0), dict(w=0), dict(w=-2), dict(size=(0, 1920)), dict(size=(1080, 0))):
        assert grad([p] * 3, **kw) == _lib.EINVAL and lib.ttup_last_error(), kw
    for sigma in (0.0, -1.0, float('nan')):
        assert grad([p] * 3, sigma=sigma) == _lib.EINVAL and b'sigma' in lib.ttup_last_error()
    for scale in (float('inf'), -float('inf'), float('nan')):
        assert grad([p] * 3, scale=scale) == _lib.EINVAL and b'scale' in lib.ttup_last_error()
    assert grad([p] * 3, h=8, w=7681) == _lib.EINVAL and b'LDS' in lib.ttup_last_error()          # the loss pass's limit: two rows of 7681 floats exceed 60 KB
    assert grad([p] * 3, nbytes=8) == _lib.EINVAL and b'workspace' in lib.ttup_last_error()
    need = lib.ttup_detect_loss_grad_workspace_bytes(2, 22, 40, 1080, 1920)
    assert grad([p] * 3, nbytes=need - 1) == _lib.EINVAL and b'workspace' in lib.ttup_last_error()
    assert grad([p] * 3, ws=odd) == _lib.EINVAL and b'aligned' in lib.ttup_last_error()
