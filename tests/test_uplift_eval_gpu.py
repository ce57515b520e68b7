"""The evaluation metrics on the MI355X (csrc/uplift_eval.hip, uplift.val_metrics / val_real_metrics, MultiStageModel.val / .val_real).

Two references, neither read from the reference project here:
  * tests/golden/uplift_eval.npz -- what the reference's own val() / val_real() produced on the recorded predictions (fp32 sums of
    at most 165 terms, its own error about 1e-5): bar 1e-4 relative, the project's parity bar; integer counts exact;
  * tests/helpers/uplift_eval_ref.py -- the float64 restatement: bar 1e-10 relative.  All summed terms are non-negative, there are
    at most 2^17 of them, each is a handful of fp64 operations whose condition stays below 1e3 under the input conditions, so the
    error stays below about 1e-11.  Measured worst on the MI355X: 9.1e-16 on the fixture, 2.4e-15 over the shape edges (N = 1, T = 2;
    DESIGN 25; every run prints its own).  Each test asks for at least 10 x of headroom under the bar.

Shapes: EV_SAMPLES = 16 samples per block (the first level of the tree across samples), 256 threads per block, 256 partials per
thread of the final block (the second level: 4096 samples)."""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from helpers import uplift_eval_cases as C
from helpers import uplift_eval_ref as R

pytestmark = pytest.mark.gpu
if has_gpu():
    from upliftingtabletennis_amd import dataset, trajgen, uplift, weights

MODES = ('global', 'local')
GOLDEN_BAR, F64_BAR = 1e-4, 1e-10
VAL_FLOATS = ('metric', 'metric_x', 'metric_y', 'metric_z', 'metric_abs', 'metric_angle', 'metric_position', 'mse')
REAL_FLOATS = ('metric_2D', 'metric_2D_normed')
# N: 1; one block -1 / exact / +1 (16 samples); a wave of lanes-per-sample groups; the block size in threads +- 1;
# 4096 = 256 blocks, one partial per thread of the final block, and one more
EDGE_N = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097)


@pytest.fixture(scope='module')
def g(golden):
    return golden('uplift_eval.npz')


def cuda(d):
    return {k: (torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def fixture_val(g, mode):
    return {'pred_rotation': g['val/%s/pred_rotation' % mode], 'pred_position': g['val/pred_position'], 'r_world': g['val/r_world'], 'rotation': g['val/rotation'],
            'mask': g['val/mask'], 'transform_mode': mode}


def fixture_real(g, s, mode):
    p = 'real_%s/' % s
    d = {k: g[p + k] for k in ('pred_position', 'r_img', 'mask', 'Mint', 'Mext', 'spin_class')}
    d.update(pred_rotation=g[p + mode + '/pred_rotation'], transform_mode=mode)
    return d


def rel(a, b):
    return abs(a - b) / abs(b)


def bits(d):
    """Every entry of a result dict as bytes (floats as float64, integers as int64): equal bytes = equal bits, NaNs included."""
    return {k: (np.asarray(v, np.float64) if np.asarray(v).dtype.kind == 'f' else np.asarray(v, np.int64)).tobytes() for k, v in d.items()}


def check_val(got, ref, bar=F64_BAR, what=''):
    worst = 0.0
    for k in VAL_FLOATS:
        e = rel(got[k], ref[k])
        worst = max(worst, e)
        assert e <= bar, (what, k, got[k], ref[k], e)
    for k in ('TP', 'TN', 'FP', 'FN'):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), (what, k, got[k], ref[k])
    assert got['number'] == ref['number']
    assert np.array_equal(got['accuracy'], ref['accuracy'], equal_nan=True), (what, got['accuracy'], ref['accuracy'])
    return worst


def check_real(got, ref, bar=F64_BAR, what=''):
    worst = 0.0
    for k in REAL_FLOATS:
        e = rel(got[k], ref[k])
        worst = max(worst, e)
        assert e <= bar, (what, k, got[k], ref[k], e)
    for k in ('TP', 'TN', 'FP', 'FN', 'number'):
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    assert np.array_equal(got['labels'], ref['labels'])
    if len(ref['scores']):
        e = float((np.abs(got['scores'] - ref['scores']) / np.abs(ref['scores'])).max())
        worst = max(worst, e)
        assert e <= bar, (what, 'scores', e)
    return worst


# ------------------------------------------------------------------------------------------ the fixture's recorded predictions
@pytest.mark.parametrize('mode', MODES)
def test_val_metrics_match_the_reference_and_the_restatement(g, mode):
    d = fixture_val(g, mode)
    got = uplift.val_metrics(**cuda(d))
    assert sorted(got) == sorted(VAL_FLOATS + ('accuracy', 'TP', 'TN', 'FP', 'FN', 'number'))
    for tag, key in (('metric', 'metric'), ('metric abs', 'metric_abs'), ('metric angle', 'metric_angle'), ('metric position', 'metric_position')):
        want = float(g['val/%s/scalar/val0/%s' % (mode, tag)])
        print('val %s %-16s device %.12g reference %.12g rel %.2e' % (mode, tag, got[key], want, rel(got[key], want)))
        assert rel(got[key], want) <= GOLDEN_BAR, (tag, got[key], want)
    assert rel(got['metric'], float(g['val/%s/return' % mode])) <= GOLDEN_BAR
    for k in ('TP', 'TN', 'FP', 'FN'):
        assert np.array_equal(got[k], g['val/%s/%s' % (mode, k)]), k
    for i, ax in enumerate('xyz'):
        assert abs(got['accuracy'][i] - float(g['val/%s/scalar/val0/accuracy %s' % (mode, ax)])) <= 1e-6
    worst = check_val(got, R.val_metrics(**d), what=mode)
    print('val %s: worst relative deviation from the float64 restatement %.2e (bar %.0e)' % (mode, worst, F64_BAR))
    assert worst <= F64_BAR / 10, 'less than 10 x under the bar: find out why before anything is widened'


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('s', ('a', 'b'))
def test_val_real_metrics_match_the_reference_and_the_restatement(g, s, mode):
    d = fixture_real(g, s, mode)
    got = uplift.val_real_metrics(**cuda(d))
    assert sorted(got) == sorted(REAL_FLOATS + ('accuracy', 'macro_f1', 'roc_auc', 'TP', 'TN', 'FP', 'FN', 'scores', 'labels', 'number'))
    p = 'real_%s/%s/' % (s, mode)
    for tag, key in (('metric 2D', 'metric_2D'), ('metric 2D normed', 'metric_2D_normed')):
        want = float(g[p + 'scalar/val real/' + tag])
        print('val_real %s %s %-16s device %.12g reference %.12g rel %.2e' % (s, mode, tag, got[key], want, rel(got[key], want)))
        assert rel(got[key], want) <= GOLDEN_BAR
    ret = g[p + 'return']
    assert rel(got['metric_2D_normed'], ret[0]) <= GOLDEN_BAR and abs(got['macro_f1'] - ret[1]) <= 1e-12
    labels, scores = g[p + 'labels'], g[p + 'scores']
    assert got['TP'] == int(((labels == 1) & (scores > 0)).sum()) and got['FN'] == int(((labels == 1) & ~(scores > 0)).sum())
    assert got['TN'] == int(((labels == 0) & (scores < 0)).sum()) and got['FP'] == int(((labels == 0) & ~(scores < 0)).sum())
    assert np.array_equal(got['labels'], labels) and got['labels'].dtype == np.int64 and got['scores'].dtype == np.float64
    assert np.abs(got['scores'] - scores).max() <= GOLDEN_BAR * np.abs(scores).max()
    for tag, key in (('accuracy', 'accuracy'), ('macro f1', 'macro_f1'), ('ROC AUC', 'roc_auc')):
        assert abs(got[key] - float(g[p + 'scalar/val real/' + tag])) <= 1e-12, tag
    ref = R.val_real_metrics(**d)
    worst = check_real(got, ref, what=(s, mode))
    assert got['accuracy'] == ref['accuracy'] and got['macro_f1'] == ref['macro_f1'] and abs(got['roc_auc'] - ref['roc_auc']) <= 1e-12
    print('val_real %s %s: worst relative deviation from the float64 restatement %.2e (bar %.0e)' % (s, mode, worst, F64_BAR))
    assert worst <= F64_BAR / 10, 'less than 10 x under the bar: find out why before anything is widened'


# ------------------------------------------------------------------------------------------ shape edges against the restatement
@pytest.mark.parametrize('t', (2, 50))
@pytest.mark.parametrize('n', EDGE_N)
def test_val_metrics_shape_edges(n, t):
    for k, mode in enumerate(MODES):
        d = C.val_inputs(1000 * t + n + 7 * k, n, t, mode)
        worst = check_val(uplift.val_metrics(**cuda(d)), R.val_metrics(**d), what=(n, t, mode))
        print('val N %d T %d %s: worst relative deviation from the float64 restatement %.2e' % (n, t, mode, worst))
        assert worst <= F64_BAR / 10


@pytest.mark.parametrize('t', (2, 50))
@pytest.mark.parametrize('n', EDGE_N)
def test_val_real_metrics_shape_edges(n, t):
    for k, mode in enumerate(MODES):
        d = C.real_inputs(2000 * t + n + 7 * k, n, t, mode)
        worst = check_real(uplift.val_real_counts(**cuda(d)), R.val_real_counts(**d), what=(n, t, mode))
        print('val_real N %d T %d %s: worst relative deviation from the float64 restatement %.2e' % (n, t, mode, worst))
        assert worst <= F64_BAR / 10


def test_mask_rows_of_every_kind_are_served():
    """All ones, a single 1, holes inside the track -- each kind alone, so that none hides behind the others."""
    d = C.val_inputs(31, 33, 50, 'global')
    r = C.real_inputs(32, 33, 50, 'global')
    rng = np.random.default_rng(5)
    ones = np.ones((33, 50), np.float32)
    single = np.zeros((33, 50), np.float32)
    single[np.arange(33), rng.integers(0, 50, 33)] = 1
    holes = ones.copy()
    holes[:, 40:] = 0
    for i in range(33):
        holes[i, rng.choice(np.arange(1, 39), size=5, replace=False)] = 0
    for name, m in (('ones', ones), ('single', single), ('holes', holes)):
        dv, dr = dict(d, mask=m), dict(r, mask=m)
        check_val(uplift.val_metrics(**cuda(dv)), R.val_metrics(**dv), what=name)
        check_real(uplift.val_real_counts(**cuda(dr)), R.val_real_counts(**dr), what=name)


def test_a_non_finite_value_in_a_masked_slot_changes_no_bit():
    """Time steps 0 and 1 build the local frame whatever the mask says, so the poison goes into masked slots from step 2 on."""
    d = C.val_inputs(41, 65, 50, 'global')
    r = C.real_inputs(42, 65, 50, 'global')
    for inputs, fn, fields in ((d, uplift.val_metrics, ('pred_position', 'r_world')), (r, uplift.val_real_counts, ('pred_position', 'r_img'))):
        masked = inputs['mask'] == 0
        masked[:, :2] = False
        assert masked.sum() > 100
        clean = fn(**cuda(inputs))
        assert all(np.isfinite(clean[k]) for k in (VAL_FLOATS if fn is uplift.val_metrics else REAL_FLOATS))
        for poison in (np.nan, np.inf, -np.inf):
            bad = dict(inputs)
            for f in fields:
                a = inputs[f].copy()
                a[masked] = poison
                bad[f] = a
            assert bits(fn(**cuda(bad))) == bits(clean), poison


def test_val_real_a_masked_slot_behind_the_camera_is_inert():
    r = C.real_inputs(51, 37, 50, 'global')
    clean = uplift.val_real_counts(**cuda(r))
    pos = r['pred_position'].copy()
    hit = 0
    for i in range(37):
        slots = np.flatnonzero(r['mask'][i, 2:] == 0) + 2
        if slots.size < 2:
            continue
        rot, tr = r['Mext'][i, :3, :3].astype(np.float64), r['Mext'][i, :3, 3].astype(np.float64)
        centre = -rot.T @ tr
        pos[i, slots[0]] = centre                           # depth 0: a division by zero in cam2img
        pos[i, slots[1]] = centre - 3.0 * rot[2]            # 3 m behind the camera
        hit += 1
    assert hit >= 10
    _, depth = R.project(pos, r['Mint'], r['Mext'])
    assert (depth < 0).sum() >= 10
    assert bits(uplift.val_real_counts(**cuda(dict(r, pred_position=pos)))) == bits(clean)
    # the same points in VALID slots do change the result: the test would notice a kernel that ignores them
    assert bits(uplift.val_real_counts(**cuda(dict(r, pred_position=pos, mask=np.ones_like(r['mask']))))) != bits(uplift.val_real_counts(**cuda(dict(r, mask=np.ones_like(r['mask'])))))


def test_val_real_cameras_are_per_sample():
    r = C.real_inputs(61, 21, 50, 'local')
    assert np.abs(r['Mext'][1:] - r['Mext'][:1]).max() > 1 and np.abs(r['Mint'][1:] - r['Mint'][:1]).max() > 10
    own = uplift.val_real_counts(**cuda(r))
    check_real(own, R.val_real_counts(**r))
    first = dict(r, Mint=np.repeat(r['Mint'][:1], 21, 0), Mext=np.repeat(r['Mext'][:1], 21, 0))
    shared = uplift.val_real_counts(**cuda(first))
    check_real(shared, R.val_real_counts(**first))
    assert rel(shared['metric_2D'], own['metric_2D']) > 0.1
    rolled = dict(r, Mint=np.roll(r['Mint'], 1, 0), Mext=np.roll(r['Mext'], 1, 0))
    check_real(uplift.val_real_counts(**cuda(rolled)), R.val_real_counts(**rolled))


# ------------------------------------------------------------------------------------------ deviations and errors
def test_coincident_first_step_gives_nan_where_the_reference_does_and_nowhere_else():
    """r_world[b, 1, :2] == r_world[b, 0, :2]: e_x = 0 / 0 (helper.py:412).  Local components 0 and 1 of that sample are NaN, so
    every metric that reads them is; component 2 = rotation . e_z is not (metric_z), nor is metric_position."""
    d = C.val_inputs(71, 20, 50, 'global')
    d['r_world'] = d['r_world'].copy()
    d['r_world'][7, 1, :2] = d['r_world'][7, 0, :2]
    got = uplift.val_metrics(**cuda(d))
    ref = R.val_metrics(**d)
    for k in ('metric', 'metric_x', 'metric_y', 'metric_abs', 'metric_angle', 'mse'):
        assert np.isnan(got[k]) and np.isnan(ref[k]), k
    for k in ('metric_z', 'metric_position'):
        assert np.isfinite(got[k]) and rel(got[k], ref[k]) <= F64_BAR, k
    for k in ('TP', 'TN', 'FP', 'FN'):
        assert np.array_equal(got[k], ref[k])
    assert list(got['TP'] + got['TN'] + got['FP'] + got['FN']) == [19, 19, 20]          # sign(NaN) matches neither +1 nor -1
    # 'local': only the target goes through the frame
    d2 = dict(C.val_inputs(72, 20, 50, 'local'))
    d2['r_world'] = d2['r_world'].copy()
    d2['r_world'][0, 1, :2] = d2['r_world'][0, 0, :2]
    got2 = uplift.val_metrics(**cuda(d2))
    assert np.isnan(got2['metric']) and np.isnan(got2['metric_x']) and np.isfinite(got2['metric_z']) and np.isfinite(got2['metric_position'])
    # val_real, 'global': an unannotated sample with coincident PREDICTED positions has a NaN score nobody reads
    r = C.real_inputs(73, 20, 50, 'global')
    assert r['spin_class'][2] == 0
    r['pred_position'] = r['pred_position'].copy()
    r['pred_position'][2, 1, :2] = r['pred_position'][2, 0, :2]
    check_real(uplift.val_real_metrics(**cuda(r)), R.val_real_metrics(**r))


def test_cosine_past_one_is_clamped():
    """Parallel spins: fp rounding can push the cosine past 1, where the reference's acos returns NaN; here the angle is 0 (or 180)."""
    d = C.val_inputs(81, 64, 50, 'local')
    gt = R.transform_rotationaxes(d['rotation'], d['r_world'])
    d['pred_rotation'] = C.f32(gt * np.where(np.arange(64) % 2, -3.0, 3.0)[:, None])
    got = uplift.val_metrics(**cuda(d))
    assert np.isfinite(got['metric_angle']) and abs(got['metric_angle'] - 90.0) < 0.05


def test_val_real_errors_are_the_references():
    r = C.real_inputs(91, 24, 50, 'global')
    with pytest.raises(ZeroDivisionError):
        uplift.val_real_metrics(**cuda(dict(r, spin_class=np.zeros(24, np.int64))))          # no annotated sample: (TP + TN) / 0
    for cls in (R.TOPSPIN_CLASS, R.BACKSPIN_CLASS):
        one = dict(r, spin_class=np.full(24, cls, np.int64))
        c = uplift.val_real_counts(**cuda(one))
        assert c['TP'] + c['FN'] == (24 if cls == R.TOPSPIN_CLASS else 0) and min(c['TP'] + c['TN'], c['FP'] + c['FN']) > 0          # some right, some wrong
        with pytest.raises(ValueError, match='one class'):
            uplift.val_real_metrics(**cuda(one))
    with pytest.raises(ValueError):
        uplift.val_metrics(*[torch.zeros(s).cuda() for s in ((4, 3), (4, 1, 3), (4, 1, 3), (4, 3), (4, 1))])          # t = 1
    with pytest.raises(ValueError):
        uplift.val_metrics(*[torch.zeros(s).cuda() for s in ((0, 3), (0, 5, 3), (0, 5, 3), (0, 3), (0, 5))])          # n = 0


# ------------------------------------------------------------------------------------------ bit-reproducibility
def test_two_calls_return_equal_bits():
    d, r = cuda(C.val_inputs(101, 4097, 50, 'global')), cuda(C.real_inputs(102, 4097, 50, 'global'))
    first_v, first_r = uplift.val_metrics(**d), uplift.val_real_metrics(**r)
    junk = torch.full((1 << 20,), float('nan'), device='cuda')          # the next workspace is not the last one's leftovers
    del junk
    assert bits(uplift.val_metrics(**d)) == bits(first_v)
    assert bits(uplift.val_real_metrics(**r)) == bits(first_r)


# ------------------------------------------------------------------------------------------ through the model
@pytest.fixture(scope='module')
def small_model():
    return uplift.MultiStageModel(weights.random_uplift_state_dict(11, 'small'), size='small', max_batch=8, max_len=64)


def model_inputs(n, t, seed):
    rng = np.random.default_rng(seed)
    r_img = C.f32(rng.uniform(0.1, 0.9, (n, t, 2)))
    table = C.f32(np.concatenate([rng.uniform(0.1, 0.9, (n, 13, 2)), np.ones((n, 13, 1))], -1))
    mask = np.ones((n, t), np.float32)
    for i in range(n):
        mask[i, int(rng.integers(t // 2, t)):] = 0          # every row ends in padding: every chunk has both mask values
    times = C.f32(np.tile(np.arange(t) * 0.02, (n, 1)) * mask)
    return [torch.from_numpy(a).cuda() for a in (r_img, table, mask, times)]


@pytest.mark.parametrize('mode', MODES)
def test_model_val_equals_the_metrics_of_its_forward_chunks(small_model, mode):
    n, t, chunk = 19, 50, 8
    r_img, table, mask, times = model_inputs(n, t, 3)
    d = cuda(C.val_inputs(111, n, t, mode))
    outs = [small_model.forward(r_img[i:i + chunk], table[i:i + chunk], mask[i:i + chunk], times[i:i + chunk]) for i in range(0, n, chunk)]
    rot, pos = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    want = uplift.val_metrics(rot, pos, d['r_world'], d['rotation'], mask, mode)
    got = small_model.val(r_img, table, mask, times, d['r_world'], d['rotation'], transform_mode=mode, batch_size=chunk)
    assert bits(got) == bits(want)
    assert bits(small_model.val(r_img, table, mask, times, d['r_world'], d['rotation'], mode)) == bits(want)          # default: max_batch = 8
    assert np.isfinite(got['metric']) and np.isfinite(got['metric_position']) and got['number'] == n
    with pytest.raises(ValueError, match='batch_size'):
        small_model.val(r_img, table, mask, times, d['r_world'], d['rotation'], batch_size=9)
    with pytest.raises(ValueError, match='transform_mode'):
        small_model.val(r_img, table, mask, times, d['r_world'], d['rotation'], transform_mode='world')


@pytest.mark.parametrize('mode', MODES)
def test_model_val_real_equals_the_metrics_of_its_forward_chunks(small_model, mode):
    n, t, chunk = 19, 50, 8
    r_img, table, mask, times = model_inputs(n, t, 4)
    r = cuda(C.real_inputs(112, n, t, mode))
    outs = [small_model.forward(r_img[i:i + chunk], table[i:i + chunk], mask[i:i + chunk], times[i:i + chunk]) for i in range(0, n, chunk)]
    rot, pos = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
    want = uplift.val_real_counts(rot, pos, r_img, mask, r['Mint'], r['Mext'], r['spin_class'], mode)
    assert bits(uplift.val_real_counts(*small_model._predict(r_img, table, mask, times, chunk, True)[2:], r_img, mask, r['Mint'], r['Mext'], r['spin_class'], mode)) == bits(want)
    try:
        ratios = uplift.val_real_metrics(rot, pos, r_img, mask, r['Mint'], r['Mext'], r['spin_class'], mode)
    except (ZeroDivisionError, ValueError) as e:          # random weights may put every score on one side
        with pytest.raises(type(e)):
            small_model.val_real(r_img, table, mask, times, r['Mint'], r['Mext'], r['spin_class'], transform_mode=mode, batch_size=chunk)
        return
    got = small_model.val_real(r_img, table, mask, times, r['Mint'], r['Mext'], r['spin_class'], transform_mode=mode, batch_size=chunk)
    assert bits(got) == bits(ratios) and got['number'] == n
    assert (got['metric_2D_normed'], got['macro_f1']) == (ratios['metric_2D_normed'], ratios['macro_f1'])


def test_chain_from_the_generator_to_the_metrics():
    """trajgen -> TableTennisDataset('test') -> model.val: finite metrics on a few dozen samples."""
    import types
    cfg = types.SimpleNamespace(blur_strength=0.4, randomize_std=8, stop_prob=0.5, randdet_prob=0.05, randmiss_prob=0.05, tablemiss_prob=0.05)
    tr = trajgen.get_valid_trajectories(48, 16, 'intermediate', 'left_to_right', as_numpy=False)
    ds = dataset.TableTennisDataset('test', dataset.get_transforms(cfg, 'test'), trajectories=tr)
    b = ds.batch(np.arange(len(ds)))
    model = uplift.MultiStageModel(weights.random_uplift_state_dict(12, 'small'), size='small', max_batch=16, max_len=64)
    # a 'test' track of 50 frames or more has the reference's all-ones mask, which the forward's own mask check refuses
    d = model.val(b.r_img, b.table_img, b.mask, b.times, b.r_world, b.rotation, check_mask=False)
    assert d['number'] == 48 and all(np.isfinite(d[k]) for k in VAL_FLOATS), d
    assert np.isfinite(d['accuracy']).all() and int((d['TP'] + d['TN'] + d['FP'] + d['FN']).max()) <= 48
    assert d['metric'] > 0 and d['metric_position'] > 0
