"""Detector evaluation on the device (csrc/detect_eval.hip, upliftingtabletennis_amd.detect_eval, BallDetector.val / TableDetector.val).

Bars.  Counts are exact and ratios of counts agree with the reference's to 1e-12.  Distances and losses are compared with the
reference's fp32 values within `C.reference_bar`: ten times the largest distance between a reference value and the float64
restatement, measured on the CPU from the fixture alone (4.6e-7 relative, so the bar is 4.6e-6; it may never exceed the project's
1e-4).  Against the float64 restatement the bar is 1e-10 relative."""
import os
import warnings

import numpy as np
import pytest
import torch

from helpers import detect_eval_cases as C
from helpers import detect_eval_ref as R
from upliftingtabletennis_amd import detect_eval, synth

pytestmark = pytest.mark.gpu

BALL_KEYS = tuple('pck@%d' % t for t in C.TOLERANCES) + ('avg_dist', 'dist_streak')
TABLE_KEYS = tuple('pck@%d' % t for t in C.TOLERANCES) + ('avg_dist', 'ratio_detected')
BALL_COUNTS = ('number', 'visible', 'valid', 'detected') + tuple('correct@%d' % t for t in C.TOLERANCES)
TABLE_COUNTS = ('number', 'valid', 'valid_visible') + tuple('correct@%d' % t for t in C.TOLERANCES)


@pytest.fixture(scope='module')
def g(golden):
    return golden('detect_eval.npz')


def close(have, want, bar):
    return np.max(np.abs(np.asarray(have) - np.asarray(want)) / np.abs(np.asarray(want))) <= bar


def against_restatement(d, want, keys, counts):
    for k in counts:
        assert d[k] == want[k], (k, d[k], want[k])
    for k in keys:
        assert R.same(d[k], want[k], C.RESTATEMENT_BAR), (k, d[k], want[k])


@pytest.mark.parametrize('name', C.BALL_SETS + C.TABLE_SETS)
def test_fixture_loss(g, name):
    bar = C.reference_bar(g)
    pred, centres, has, sigma, batches = C.loss_inputs(g, name)
    mse, wgt, _ = C.restated_losses(g)[name]
    for key, weighted, restated in (('mse', False, mse), ('weighted', True, wgt)):
        d = detect_eval.heatmap_loss(pred, centres, has, sigma=sigma, weighted=weighted, batch_size=batches[0])
        ref_sums, ref_loss = g['%s/sums_%s' % (name, key)], float(g['%s/loss_%s' % (name, key)])
        want_loss = C.batched_loss(restated, batches, R.loss_from_sums)
        print('%s %s: sums within %.3e of the reference (bar %.3e) and %.3e of the restatement; loss %.9g, reference %.9g'
              % (name, key, np.max(np.abs(d['sums'] - ref_sums) / ref_sums), bar, np.max(np.abs(d['sums'] - restated) / restated), d['loss'], ref_loss))
        assert d['sums'].shape == ref_sums.shape and d['sums'].dtype == np.float64
        assert close(d['sums'], ref_sums, bar) and C.rel(d['loss'], ref_loss) <= bar
        assert close(d['sums'], restated, C.RESTATEMENT_BAR) and C.rel(d['loss'], want_loss) <= C.RESTATEMENT_BAR


def test_fixture_ball_metrics(g):
    bar = C.reference_bar(g)
    for label, prefix, inputs in C.ball_items(g):
        d = detect_eval.ball_val_metrics(*inputs, tolerances=C.TOLERANCES)
        C.check_metrics(d, g, prefix, BALL_KEYS, bar)
        against_restatement(d, R.ball_metrics(*inputs, tolerances=C.TOLERANCES), BALL_KEYS, BALL_COUNTS)
    d = detect_eval.ball_val_metrics(*C.ball_inputs(g, 'ball_a'))          # the default tolerances are val()'s
    assert [k for k in d if k.startswith('pck@')] == ['pck@2', 'pck@5', 'pck@10']


def test_fixture_table_metrics(g):
    bar = C.reference_bar(g)
    for label, prefix, inputs in C.table_items(g):
        d = detect_eval.table_val_metrics(*inputs, tolerances=C.TOLERANCES)
        C.check_metrics(d, g, prefix, TABLE_KEYS, bar)
        against_restatement(d, R.table_metrics(*inputs, tolerances=C.TOLERANCES), TABLE_KEYS, TABLE_COUNTS)


@pytest.mark.parametrize('name', sorted(C.LOSS_EDGES))
def test_loss_edges(name):
    pred, centres, has, sigma, size = C.loss_edge(name)
    mse, wgt, margin = R.heatmap_loss_sums_both(pred, centres, has, sigma, size)
    assert margin >= 1e-6          # no weight can flip between the two evaluations of the target
    dev = torch.from_numpy(pred).cuda()
    for weighted, want in ((False, mse), (True, wgt)):
        d = detect_eval.heatmap_loss(dev, centres, has, sigma=sigma, weighted=weighted, size=size, batch_size=2)
        print('%s weighted=%d: within %.3e of the restatement' % (name, weighted, np.max(np.abs(d['sums'] - want) / want)))
        assert close(d['sums'], want, C.RESTATEMENT_BAR)
        assert C.rel(d['loss'], R.loss_from_sums(want, size, batch_size=2)) <= C.RESTATEMENT_BAR          # three samples: batches of 2 and 1
    if name == 'no_target':          # the loss is the mean of up(pred)^2, weighted or not
        up2 = np.array([[(R.upsample(pred[0, j], size) ** 2).sum() for j in range(pred.shape[1])]])
        assert np.array_equal(mse, wgt) and close(d['sums'], up2, C.RESTATEMENT_BAR) and C.rel(d['loss'], up2.mean() / (size[0] * size[1])) <= C.RESTATEMENT_BAR
    if name.startswith('identity'):          # up is the identity: the unweighted sum is that of (pred - target)^2
        direct = np.array([[((pred[i, j].astype(np.float64) - R.target(centres[i, j], sigma, size)) ** 2).sum() for j in range(pred.shape[1])] for i in range(pred.shape[0])])
        assert close(mse, direct, 1e-13)


@pytest.mark.parametrize('n', [1, 300, 1000])          # one sample; 300 balls: two blocks, the last not full; 13 000 keypoints: 51 blocks
def test_metric_edges(n):
    ball, table = C.metric_edges(n, seed=n)
    for tol in ((2, 5, 10), C.TOLERANCES, (2.5,)):
        d = detect_eval.ball_val_metrics(*ball, tolerances=tol)
        against_restatement(d, R.ball_metrics(*ball, tolerances=tol), ['pck@%g' % t for t in tol] + ['avg_dist', 'dist_streak'],
                            ['number', 'visible', 'valid', 'detected'] + ['correct@%g' % t for t in tol])
        d = detect_eval.table_val_metrics(*table, tolerances=tol)
        against_restatement(d, R.table_metrics(*table, tolerances=tol), ['pck@%g' % t for t in tol] + ['avg_dist', 'ratio_detected'],
                            ['number', 'valid', 'valid_visible'] + ['correct@%g' % t for t in tol])
    pred, gt, lo, hi, vis = ball
    d = detect_eval.ball_val_metrics(pred, gt, lo, hi, np.zeros_like(vis))          # no sample visible: every sentinel
    assert (d['pck@5'], d['avg_dist'], d['dist_streak'], d['visible'], d['number']) == (-1, 10000, 10000, 0, n)
    d = detect_eval.ball_val_metrics(pred, gt, gt, gt, np.ones_like(vis))          # zero-length segments: the plain distance
    want = R.ball_metrics(pred, gt, gt, gt, np.ones_like(vis))
    against_restatement(d, want, ['pck@2', 'pck@5', 'pck@10', 'avg_dist', 'dist_streak'], ['visible', 'valid', 'detected', 'correct@2', 'correct@5', 'correct@10'])
    assert R.same(d['avg_dist'], d['dist_streak'], 1e-15)


def test_two_calls_return_the_same_bits(g):
    pred, centres, has, sigma, _ = C.loss_inputs(g, 'table_a')
    a, b = (detect_eval.heatmap_loss(pred, centres, has, sigma=sigma, weighted=True) for _ in range(2))
    assert a['sums'].tobytes() == b['sums'].tobytes() and a['loss'] == b['loss']
    ball, table = C.metric_edges(1000, seed=5)
    a, b = (detect_eval.ball_metrics_device(*ball, tolerances=C.TOLERANCES) for _ in range(2))
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
    a, b = (detect_eval.table_metrics_device(*table, tolerances=C.TOLERANCES) for _ in range(2))
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


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


def same_dict(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (k, a[k], b[k])


@pytest.mark.parametrize('model_name', ['wasb', 'vitpose'])
def test_ball_detector_val_is_predict_then_the_functions(synthetic_weights, frames, model_name):
    """max_batch 2 on three triples: two chunks, the second not full."""
    from upliftingtabletennis_amd.interface import BallDetector
    det = BallDetector(model_name, max_batch=2, dtype='f32')
    triples = [[frames[i], frames[i + 1], frames[i + 2]] for i in range(N_FRAMES - 2)]
    n = len(triples)
    rng = np.random.default_rng(3)
    gt = np.stack([rng.uniform(100, 1800, n), rng.uniform(100, 1000, n)], 1)
    lo, hi = gt - rng.uniform(0, 20, (n, 2)), gt + rng.uniform(0, 20, (n, 2))
    vis = np.array([1, 0, 1])
    pos0, heat0 = det.predict(triples)
    out = det.val(triples, gt, lo, hi, vis, sigma=6, refine='table', tolerances=C.TOLERANCES, batch_size=2)
    pos1, heat1 = det.predict(triples)
    assert np.array_equal(pos0, pos1) and np.array_equal(heat0, heat1)          # predict returns what it returned before
    loss = detect_eval.heatmap_loss(heat0, gt.reshape(n, 1, 2), (vis != 0).reshape(n, 1), sigma=6, weighted=False, batch_size=2)
    want = detect_eval.ball_val_metrics(pos0, gt, lo, hi, vis, tolerances=C.TOLERANCES)
    want.update(loss=loss['loss'], loss_sums=loss['sums'])
    same_dict(out, want)
    # refine='ball' (the default, what val() refines with) moves the positions alone: the ball fit on the same heatmaps
    from upliftingtabletennis_amd import refine
    out = det.val(triples, gt, lo, hi, vis)
    want = detect_eval.ball_val_metrics(refine.extract_position_ball(heat0, 1920, 1080), gt, lo, hi, vis)
    want.update(loss=detect_eval.loss_from_sums(loss['sums']), loss_sums=loss['sums'])
    same_dict(out, want)


@pytest.mark.parametrize('model_name', ['hrnet', 'vitpose'])
def test_table_detector_val_is_predict_then_the_functions(synthetic_weights, frames, model_name):
    from upliftingtabletennis_amd.interface import TableDetector
    det = TableDetector(model_name, max_batch=2, dtype='f32')
    images = frames[:3]
    rng = np.random.default_rng(4)
    coords = np.concatenate([np.floor(rng.uniform(50, 1000, (3, 13, 2))), rng.choice([1.0, 1.0, 0.0], (3, 13, 1))], 2)
    pos0, heat0 = det.predict(images)
    out = det.val(images, coords, sigma=6, tolerances=C.TOLERANCES, batch_size=2)
    pos1, heat1 = det.predict(images)
    assert np.array_equal(pos0, pos1) and np.array_equal(heat0, heat1)
    loss = detect_eval.heatmap_loss(heat0[:, 0], coords[..., :2], coords[..., 2] == 1, sigma=6, weighted=True, batch_size=2)
    want = detect_eval.table_val_metrics(pos0, coords, tolerances=C.TOLERANCES)
    want.update(loss=loss['loss'], loss_sums=loss['sums'])
    same_dict(out, want)
