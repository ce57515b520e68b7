"""The evaluation metrics without a GPU: the float64 restatement (tests/helpers/uplift_eval_ref.py) against what the reference's own
val() / val_real() produced (tests/golden/uplift_eval.npz, tools/make_goldens_eval.py), the host-side pieces of
upliftingtabletennis_amd.uplift (roc_auc, CheckpointSelector) and the C-ABI's argument checks."""
import ctypes
import os

import numpy as np
import pytest

from upliftingtabletennis_amd import _lib, uplift
from helpers import uplift_eval_ref as R

MODES = ('global', 'local')
SETS = ('a', 'b')
RTOL = 1e-4          # the project's parity bar; the reference sums <= 165 fp32 terms, its own error is about 1e-5
NEW_SYMBOLS = ('ttup_uplift_eval_workspace_bytes', 'ttup_uplift_val_metrics', 'ttup_uplift_val_real_metrics')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def g(golden):
    return golden('uplift_eval.npz')


def rel(a, b):
    return abs(a - b) / abs(b)


def val_ref(g, mode):
    return R.val_metrics(g['val/%s/pred_rotation' % mode], g['val/pred_position'], g['val/r_world'], g['val/rotation'], g['val/mask'], mode)


def real_ref(g, s, mode):
    p = 'real_%s/' % s
    return R.val_real_metrics(g[p + mode + '/pred_rotation'], g[p + 'pred_position'], g[p + 'r_img'], g[p + 'mask'], g[p + 'Mint'], g[p + 'Mext'],
                              g[p + 'spin_class'], mode)


@pytest.mark.parametrize('mode', MODES)
def test_fixture_satisfies_the_input_conditions(g, mode):
    c = R.input_conditions(g, mode)
    assert 1.0 <= c['val_angle'].min() and c['val_angle'].max() <= 179.0
    assert c['val_component'] >= 1e-3 and c['val_step'] >= 1e-3 and c['val_mask_rows'] >= 1
    for s in SETS:
        p = 'real_%s/' % s
        assert c[p + 'component'] >= 1e-3 and c[p + 'step'] >= 1e-3 and c[p + 'mask_rows'] >= 1
        assert c[p + 'depth'] >= 0.5
        assert c[p + 'classes'] == {0, R.TOPSPIN_CLASS, R.BACKSPIN_CLASS}
    assert g['val/mask'].shape == (64 + 64 + 37, 50) and g['real_a/mask'].shape[0] == 4 + 4 + 3 and g['real_b/mask'].shape[0] == 64 + 5
    # the mask kinds the kernels must serve: all ones, a single 1, a hole inside the track
    m = g['val/mask']
    assert (m.sum(1) == 50).any() and (m.sum(1) == 1).any()
    assert any(np.any(np.diff(np.flatnonzero(row)) > 1) for row in m)


@pytest.mark.parametrize('mode', MODES)
def test_restatement_reproduces_the_references_val(g, mode):
    d = val_ref(g, mode)
    tags = {'metric': 'metric', 'metric abs': 'metric_abs', 'metric angle': 'metric_angle', 'metric position': 'metric_position'}
    for tag, key in tags.items():
        want = float(g['val/%s/scalar/val0/%s' % (mode, tag)])
        assert rel(d[key], want) <= RTOL, (tag, d[key], want)
    assert rel(d['metric'], float(g['val/%s/return' % mode])) <= RTOL
    for k in ('TP', 'TN', 'FP', 'FN'):
        assert np.array_equal(d[k], g['val/%s/%s' % (mode, k)]), k
    assert int((d['TP'] + d['TN'] + d['FP'] + d['FN']).min()) == d['number'] == 165          # no zero component under the input conditions
    assert d['FP'].sum() + d['FN'].sum() > 0                                                  # the swap of FP and FN is exercised
    for i, ax in enumerate('xyz'):
        assert abs(d['accuracy'][i] - float(g['val/%s/scalar/val0/accuracy %s' % (mode, ax)])) <= 1e-6          # fp32 in the reference


def test_fp_and_fn_are_swapped_as_the_reference_swaps_them(g):
    """train.py:181 hands (prediction, target) to binary_metrics(rot_gt, rot_pred): its 'FP' counts prediction < 0 with target > 0."""
    d = val_ref(g, 'global')
    pred, gt = R.local_spins(g['val/global/pred_rotation'], g['val/r_world'], g['val/rotation'], 'global')
    assert np.array_equal(d['FP'], ((pred < 0) & (gt > 0)).sum(0)) and np.array_equal(d['FN'], ((pred > 0) & (gt < 0)).sum(0))
    assert not np.array_equal(d['FP'], d['FN'])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('s', SETS)
def test_restatement_reproduces_the_references_val_real(g, s, mode):
    d = real_ref(g, s, mode)
    p = 'real_%s/%s/' % (s, mode)
    for tag, key in (('metric 2D', 'metric_2D'), ('metric 2D normed', 'metric_2D_normed')):
        want = float(g[p + 'scalar/val real/' + tag])
        assert rel(d[key], want) <= RTOL, (tag, d[key], want)
    ret = g[p + 'return']
    assert rel(d['metric_2D_normed'], ret[0]) <= RTOL and abs(d['macro_f1'] - ret[1]) <= 1e-12
    # the reference's counts, from the labels and fp32 scores it handed to roc_auc_score (train.py:265-280)
    labels, scores = g[p + 'labels'], g[p + 'scores']
    want = {'TP': int(((labels == 1) & (scores > 0)).sum()), 'FN': int(((labels == 1) & ~(scores > 0)).sum()),
            'TN': int(((labels == 0) & (scores < 0)).sum()), 'FP': int(((labels == 0) & ~(scores < 0)).sum())}
    assert {k: d[k] for k in want} == want
    assert min(want.values()) > 0 or s == 'a'          # the larger set has all four outcomes
    assert np.array_equal(d['labels'], labels)
    assert np.abs(d['scores'] - scores).max() <= RTOL * np.abs(scores).max()
    assert abs(d['accuracy'] - float(g[p + 'scalar/val real/accuracy'])) <= 1e-12
    assert abs(d['macro_f1'] - float(g[p + 'scalar/val real/macro f1'])) <= 1e-12
    assert abs(d['roc_auc'] - float(g[p + 'scalar/val real/ROC AUC'])) <= 1e-12
    assert abs(uplift.roc_auc(labels, scores) - float(g[p + 'scalar/val real/ROC AUC'])) <= 1e-12


def test_roc_auc_equals_sklearns_with_ties():
    metrics = pytest.importorskip('sklearn.metrics')
    rng = np.random.default_rng(7)
    for trial in range(200):
        n = int(rng.integers(2, 80))
        y = rng.integers(0, 2, n)
        if y.min() == y.max():
            y[0] = 1 - y[0]
        s = rng.normal(size=n)
        if trial % 2:
            s = np.round(s * (1 + trial % 5))          # many ties
        if trial % 7 == 0:
            s[:] = 0.25                                # every score equal: 0.5
        want = metrics.roc_auc_score(y, s)
        assert abs(uplift.roc_auc(y, s) - want) <= 1e-12 and abs(R.roc_auc(y, s) - want) <= 1e-12, trial


def test_roc_auc_errors():
    with pytest.raises(ValueError, match='one class'):
        uplift.roc_auc([1, 1, 1], [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match='one class'):
        uplift.roc_auc([], [])
    with pytest.raises(ValueError, match='NaN'):
        uplift.roc_auc([0, 1], [0.1, float('nan')])


def test_checkpoint_selector_follows_the_references_rules():
    """uplifting/train.py:75-102 on a hand-written epoch table: (trajectory, spin, synthetic) -> files."""
    T, S, Y, M = 'model_trajectory.pt', 'model_spin.pt', 'model_synthetic.pt', 'model.pt'
    table = [
        ((0.020, 0.50, 3.0), (T, S, Y)),          # first epoch: every simple rule fires; above the threshold: no model.pt
        ((0.030, 0.40, 4.0), ()),                 # all worse
        ((0.015, 0.40, 4.0), (T,)),               # trajectory alone
        ((0.030, 0.60, 4.0), (S,)),               # spin alone
        ((0.030, 0.60, 4.0), (S,)),               # a spin tie saves again (>=)
        ((0.030, 0.10, 2.0), (Y,)),               # synthetic alone
        ((0.0071, 0.90, 4.0), (T, S)),            # the gate: 0.0071 > 0.007 keeps model.pt unwritten, however good the spin
        ((0.0070, 0.70, 4.0), (T, M)),            # <= threshold and spin 0.7 > 0: the mixed rule's `>` branch
        ((0.0065, 0.60, 4.0), (T,)),              # under the threshold, spin worse than the mixed best: nothing mixed
        ((0.0069, 0.70, 4.0), (M,)),              # `==` branch with a better trajectory metric than at the last save (0.0070)
        ((0.0069, 0.70, 4.0), ()),                # `==` branch without
        ((0.0068, 1.00, 4.0), (S, M)),            # `>` again: 100 %
        ((0.0069, 1.00, 4.0), (S,)),              # `==`, trajectory worse than the saved 0.0068
        ((0.0060, 1.00, 4.0), (T, S, M)),         # `==`, better
    ]
    sel = uplift.CheckpointSelector()
    assert sel.threshold_trajectory_metric == 0.007
    for epoch, (metrics, want) in enumerate(table):
        assert sel.update(*metrics) == want, (epoch, metrics)
    assert (sel.best_metric_trajectory, sel.best_metric_spin, sel.best_metric_synthetic) == (0.0060, 1.00, 2.0)
    assert (sel.best_metric_spin_mixed, sel.best_metric_trajectory_mixed) == (1.00, 0.0060)
    # the `==` branch compares with the value at the last SAVE, which the `>` branch set
    sel = uplift.CheckpointSelector(threshold_trajectory_metric=0.5)
    assert sel.update(0.4, 0.8, 1.0) == (T, S, Y, M)
    assert sel.update(0.45, 0.8, 1.0) == (S,)
    assert sel.update(0.39, 0.8, 1.0) == (T, S, M)
    assert sel.update(0.6, 0.9, 1.0) == (S,)          # over the gate


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from upliftingtabletennis_amd import build
        build.build()
    return _lib.load()


def test_new_symbols_are_declared_bound_and_built(lib):
    hdr = open(os.path.join(ROOT, 'include', 'ttup.h')).read()
    from upliftingtabletennis_amd import build
    assert 'uplift_eval.hip' in build.SOURCES
    for name in NEW_SYMBOLS:
        assert name + '(' in hdr and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.ttup_version() == 103
    assert lib.ttup_uplift_eval_workspace_bytes(0) == 0 and lib.ttup_uplift_eval_workspace_bytes(-5) == 0
    assert lib.ttup_uplift_eval_workspace_bytes(1) == lib.ttup_uplift_eval_workspace_bytes(16) < lib.ttup_uplift_eval_workspace_bytes(17)


def test_new_symbols_refuse_bad_arguments_before_any_device_call(lib):
    """Null pointers, n = 0 and t = 1 are TTUP_EINVAL with a message; this machine may have no device at all.  The non-null
    pointers are host addresses nothing dereferences: the checks come first."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    val = lambda ptrs, n, t, ws=p, nbytes=1 << 20: lib.ttup_uplift_val_metrics(*ptrs, n, t, 1, ws, nbytes, p, p, None)          # noqa: E731
    real = lambda ptrs, n, t, ws=p, nbytes=1 << 20: lib.ttup_uplift_val_real_metrics(*ptrs, n, t, 1, ws, nbytes, p, p, p, p, None)          # noqa: E731
    for fn, k in ((val, 5), (real, 7)):
        for hole in range(k):
            assert fn([None if i == hole else p for i in range(k)], 4, 50) == _lib.EINVAL
            assert b'null pointer' in lib.ttup_last_error()
        assert fn([p] * k, 4, 50, ws=None) == _lib.EINVAL and b'null pointer' in lib.ttup_last_error()
        assert fn([p] * k, 0, 50) == _lib.EINVAL and b'at least one sample' in lib.ttup_last_error()
        assert fn([p] * k, -1, 50) == _lib.EINVAL
        assert fn([p] * k, 4, 1) == _lib.EINVAL and b'two time steps' in lib.ttup_last_error()
        assert fn([p] * k, 4, 50, nbytes=8) == _lib.EINVAL and b'workspace' in lib.ttup_last_error()
    assert lib.ttup_uplift_val_metrics(p, p, p, p, p, 4, 50, 1, p, 1 << 20, None, p, None) == _lib.EINVAL
    assert lib.ttup_uplift_val_real_metrics(p, p, p, p, p, p, p, 4, 50, 1, p, 1 << 20, p, p, p, None, None) == _lib.EINVAL


def test_python_surface_refuses_bad_modes_before_the_library():
    with pytest.raises(ValueError, match='transform_mode'):
        uplift.val_metrics(None, None, None, None, None, transform_mode='world')
    with pytest.raises(ValueError, match='transform_mode'):
        uplift.val_real_metrics(None, None, None, None, None, None, None, transform_mode='world')
