"""Detector evaluation without a GPU: the float64 restatement (tests/helpers/detect_eval_ref.py) against what the reference's own
functions returned on recorded predictions (tests/golden/detect_eval.npz, tools/make_goldens_detect_eval.py), the fixture's
conditions, the host half of upliftingtabletennis_amd.detect_eval and the C-ABI's argument checks.

Measured here (printed by test_reference_rounding_sets_the_gpu_bar): the reference's fp32 values lie within 4.6e-7 relative of the
restatement, so the GPU test's bar against the reference is 4.6e-6 (ten times that, under the 1e-4 cap)."""
import ctypes
import os

import numpy as np
import pytest

from upliftingtabletennis_amd import _lib, detect_eval
from helpers import detect_eval_cases as C
from helpers import detect_eval_ref as R

NEW_SYMBOLS = ('ttup_detect_loss_workspace_bytes', 'ttup_detect_metrics_workspace_bytes', 'ttup_detect_heatmap_loss', 'ttup_detect_ball_metrics',
               'ttup_detect_table_metrics')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BALL_KEYS = tuple('pck@%d' % t for t in C.TOLERANCES) + ('avg_dist', 'dist_streak')
TABLE_KEYS = tuple('pck@%d' % t for t in C.TOLERANCES) + ('avg_dist', 'ratio_detected')


@pytest.fixture(scope='module')
def g(golden):
    return golden('detect_eval.npz')


def test_fixture_meets_its_conditions(g):
    assert tuple(g['tolerances']) == C.TOLERANCES
    assert float(g['target_margin']) >= 1e-6
    for name, (_, _, margin) in C.restated_losses(g).items():
        assert margin >= 1e-6, name          # no weight can flip between fp32 and fp64 evaluation of the target
    for label, _, (pred, gt, lo, hi, vis) in C.ball_items(g):
        m = np.asarray(vis) == 1
        for a, b in ((lo, gt), (gt, hi), (gt, lo), (lo, hi)):
            dist, l2, _ = R.segment_distance(pred[m][:, :2], np.asarray(a)[m], np.asarray(b)[m])
            assert not np.any((l2 != 0) & (l2 > 1e-13) & (l2 < 1e-11)), label
        d = np.minimum(R.segment_distance(pred[m][:, :2], lo[m], gt[m])[0], R.segment_distance(pred[m][:, :2], gt[m], hi[m])[0])
        assert all(np.abs(d - t).min() >= 1e-3 for t in C.TOLERANCES if d.size), label
    for label, _, (pred, gt) in C.table_items(g):
        both = (pred[..., 2] == 1) & (gt[..., 2] == 1)
        d = np.sqrt(((pred[..., :2].astype(np.float32).astype(np.float64) - gt[..., :2]) ** 2).sum(-1))[both]
        assert all(np.abs(d - t).min() >= 1e-3 for t in C.TOLERANCES if d.size), label
    # what the kernels must serve: two heatmap sizes, unequal last batches, an invisible and an occluded ball, invisible keypoints,
    # zero-length streaks, t clamped at both ends
    assert g['ball_a/pred'].shape == (11, 1, 22, 40) and g['ball_b/pred'].shape == (5, 1, 44, 80) and g['table_a/pred'].shape == (3, 13, 22, 40)
    assert set(g['ball_a/vis']) == {1, 0, -1} and (g['table_a/gt'][..., 2] == 0).sum() == 3
    assert np.array_equal(g['ball_a/gt_min'][::4], g['ball_a/gt'][::4].astype(np.float32)) and np.array_equal(g['ball_a/gt_max'][::4], g['ball_a/gt_min'][::4])
    pred, gt, lo, hi, _ = C.ball_inputs(g, 'ball_clamp')
    assert R.segment_distance(pred[:, :2], lo, gt)[2].min() < 0 and R.segment_distance(pred[:, :2], gt, hi)[2].max() > 1


def test_reference_rounding_sets_the_gpu_bar(g):
    worst = C.reference_rounding(g)
    print('reference fp32 rounding against the float64 restatement: %.3e relative -> bar %.3e' % (worst, C.reference_bar(g)))
    assert 0 < worst <= C.PARITY_BAR / 10          # ten times the rounding stays under the parity cap: the bar is the measured one
    assert C.reference_bar(g) == 10 * worst


def test_restatement_reproduces_the_references_losses(g):
    for name, (mse, wgt, _) in C.restated_losses(g).items():
        batches = [int(b) for b in g[name + '/batches']]
        for key, sums in (('mse', mse), ('weighted', wgt)):
            want = g['%s/sums_%s' % (name, key)]
            assert sums.shape == want.shape and np.max(np.abs(sums - want) / want) <= C.PARITY_BAR, (name, key)
            for fn in (R.loss_from_sums, detect_eval.loss_from_sums):          # the package's host half computes the same figure
                assert C.rel(C.batched_loss(sums, batches, fn), float(g['%s/loss_%s' % (name, key)])) <= C.PARITY_BAR, (name, key)
        assert np.all(wgt >= mse)


def test_loss_from_sums_averages_batch_means_not_samples():
    sums = np.array([[4.0], [8.0], [30.0]])
    size = (1, 2)
    assert detect_eval.loss_from_sums(sums, size) == R.loss_from_sums(sums, size) == 42.0 / 6
    assert detect_eval.loss_from_sums(sums, size, batch_size=2) == R.loss_from_sums(sums, size, batch_size=2) == (12.0 / 4 + 30.0 / 2) / 2
    with pytest.raises(ValueError, match='batch_size'):
        detect_eval.loss_from_sums(sums, size, batch_size=0)


def test_restatement_reproduces_the_references_ball_metrics(g):
    for label, prefix, inputs in C.ball_items(g):
        C.check_metrics(R.ball_metrics(*inputs, tolerances=C.TOLERANCES), g, prefix, BALL_KEYS, C.PARITY_BAR)


def test_restatement_reproduces_the_references_table_metrics(g):
    for label, prefix, inputs in C.table_items(g):
        C.check_metrics(R.table_metrics(*inputs, tolerances=C.TOLERANCES), g, prefix, TABLE_KEYS, C.PARITY_BAR)


def test_each_sentinel_has_a_case_of_its_own(g):
    m = lambda k: float(g[k])          # noqa: E731
    assert (m('ball_none_visible/metric/pck@5'), m('ball_none_visible/metric/avg_dist'), m('ball_none_visible/metric/dist_streak')) == (-1, 10000, 10000)
    assert m('ball_none_flagged/metric/pck@5') == -1 and m('ball_none_flagged/metric/avg_dist') < 10000
    assert m('ball_none_detected/metric/avg_dist') == m('ball_none_detected/metric/dist_streak') == 10000 and m('ball_none_detected/metric/pck@5') >= 0
    assert (m('table_none_valid/metric/pck@5'), m('table_none_valid/metric/avg_dist'), m('table_none_valid/metric/ratio_detected')) == (-1, 10000, 0)
    assert np.isnan(m('table_only_invisible/metric/pck@5')) and np.isnan(m('table_only_invisible/metric/avg_dist'))


def test_host_finish_applies_the_sentinels():
    tol = [2.0, 5.0]
    d = detect_eval.finish_ball(np.array([12.0, 6.0]), np.array([4, 3, 2, 1, 3, 9]), tol)
    assert (d['pck@2'], d['pck@5'], d['avg_dist'], d['dist_streak']) == (1 / 3, 1.0, 6.0, 3.0)
    assert (d['number'], d['visible'], d['valid'], d['detected'], d['correct@5']) == (9, 4, 3, 2, 3)
    d = detect_eval.finish_ball(np.array([0.0, 0.0]), np.array([0, 0, 0, 0, 0, 9]), tol)
    assert (d['pck@2'], d['avg_dist'], d['dist_streak']) == (-1, 10000, 10000)
    d = detect_eval.finish_table(np.array([10.0, 0.0]), np.array([5, 4, 0, 2, 4, 26]), tol)
    assert (d['pck@2'], d['pck@5'], d['avg_dist'], d['ratio_detected']) == (0.5, 1.0, 2.5, 5 / 26)
    d = detect_eval.finish_table(np.array([0.0, 0.0]), np.array([0, 0, 0, 0, 0, 26]), tol)
    assert (d['pck@2'], d['avg_dist'], d['ratio_detected']) == (-1, 10000, 0.0)
    d = detect_eval.finish_table(np.array([0.0, 0.0]), np.array([3, 0, 0, 0, 0, 26]), tol)
    assert np.isnan(d['pck@2']) and np.isnan(d['avg_dist']) and d['ratio_detected'] == 3 / 26


def test_python_surface_refuses_bad_arguments_before_the_library():
    with pytest.raises(ValueError, match='tolerances'):
        detect_eval.ball_val_metrics(None, None, None, None, None, tolerances=())
    with pytest.raises(ValueError, match='tolerances'):
        detect_eval.table_val_metrics(None, None, tolerances=range(9))
    with pytest.raises(ValueError, match='refine'):
        detect_eval.refine_variant('gaussian')
    assert detect_eval.refine_variant('ball') == _lib.REFINE_BALL and detect_eval.refine_variant('table') == _lib.REFINE_TABLE
    from upliftingtabletennis_amd import interface, wasb
    for mod in (interface, wasb):
        assert mod.heatmap_loss is detect_eval.heatmap_loss and mod.ball_val_metrics is detect_eval.ball_val_metrics
        assert mod.table_val_metrics is detect_eval.table_val_metrics
    for cls in (interface.BallDetector, interface.TableDetector, interface.ViTPoseBallDetector, interface.ViTPoseTableDetector):
        assert callable(cls.val)


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from upliftingtabletennis_amd import build
        build.build()
    return _lib.load()


def test_new_symbols_are_declared_bound_and_built(lib):
    hdr = open(os.path.join(ROOT, 'include', 'ttup.h')).read()
    from upliftingtabletennis_amd import build
    assert 'detect_eval.hip' in build.SOURCES
    for name in NEW_SYMBOLS:
        assert name + '(' in hdr and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert '#define TTUP_DETECT_MAX_TOLERANCES %d' % detect_eval.MAX_TOLERANCES in hdr
    assert lib.ttup_detect_metrics_workspace_bytes(0) == 0 and lib.ttup_detect_metrics_workspace_bytes(-3) == 0
    assert lib.ttup_detect_metrics_workspace_bytes(1) == lib.ttup_detect_metrics_workspace_bytes(256) < lib.ttup_detect_metrics_workspace_bytes(257)
    assert lib.ttup_detect_loss_workspace_bytes(0, 1080, 1920) == 0 and lib.ttup_detect_loss_workspace_bytes(2, 0, 1920) == 0
    assert lib.ttup_detect_loss_workspace_bytes(3, 1080, 1920) == 3 * (2 * 1080 + 1920) * 8


def test_new_symbols_refuse_bad_arguments_before_any_device_call(lib):
    """Null pointers, n <= 0, sigma <= 0, an empty tolerance list and a short workspace are TTUP_EINVAL with a message; this machine may
    have no device at all.  The non-null pointers are host addresses nothing dereferences: the checks come first."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    tol = (ctypes.c_double * 3)(2.0, 5.0, 10.0)
    big = 1 << 30

    def loss(ptrs, n=2, c=1, h=22, w=40, sigma=6.0, ws=p, nbytes=big, out=p, size=(1080, 1920)):
        return lib.ttup_detect_heatmap_loss(*ptrs, n, c, h, w, sigma, size[0], size[1], 0, ws, nbytes, out, None)

    def ball(ptrs, n=4, t=tol, nt=3, ws=p, nbytes=big, sums=p, counts=p):
        return lib.ttup_detect_ball_metrics(*ptrs, n, t, nt, ws, nbytes, sums, counts, None)

    def table(ptrs, n=4, k=13, t=tol, nt=3, ws=p, nbytes=big, sums=p, counts=p):
        return lib.ttup_detect_table_metrics(*ptrs, n, k, t, nt, ws, nbytes, sums, counts, None)

    for fn, k in ((loss, 3), (ball, 5), (table, 2)):
        for hole in range(k):
            assert fn([None if i == hole else p for i in range(k)]) == _lib.EINVAL
            assert b'null pointer' in lib.ttup_last_error()
        assert fn([p] * k, ws=None) == _lib.EINVAL and b'null pointer' in lib.ttup_last_error()
        assert fn([p] * k, n=0) == _lib.EINVAL and b'at least one sample' in lib.ttup_last_error()
        assert fn([p] * k, n=-1) == _lib.EINVAL
        assert fn([p] * k, nbytes=8) == _lib.EINVAL and b'workspace' in lib.ttup_last_error()
    assert loss([p] * 3, out=None) == _lib.EINVAL
    assert loss([p] * 3, c=0) == _lib.EINVAL
    for sigma in (0.0, -1.0, float('nan')):
        assert loss([p] * 3, sigma=sigma) == _lib.EINVAL and b'sigma' in lib.ttup_last_error()
    assert loss([p] * 3, h=0) == _lib.EINVAL and loss([p] * 3, size=(0, 1920)) == _lib.EINVAL
    assert loss([p] * 3, h=8, w=7681) == _lib.EINVAL and b'LDS' in lib.ttup_last_error()          # two rows of 7681 floats exceed 60 KB
    for fn, k in ((ball, 5), (table, 2)):
        assert fn([p] * k, nt=0) == _lib.EINVAL and b'tolerances' in lib.ttup_last_error()
        assert fn([p] * k, nt=detect_eval.MAX_TOLERANCES + 1) == _lib.EINVAL
        assert fn([p] * k, t=None) == _lib.EINVAL
        assert fn([p] * k, sums=None) == _lib.EINVAL and fn([p] * k, counts=None) == _lib.EINVAL
    assert table([p] * 2, k=0) == _lib.EINVAL
