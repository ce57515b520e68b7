"""What tests/test_detect_eval_host.py and tests/test_detect_eval_gpu.py share: the cases of tests/golden/detect_eval.npz, the float64
restatement evaluated on them (once per process) and the reference's own fp32 rounding measured from the two."""
import numpy as np

from . import detect_eval_ref as R

BALL_SETS = ('ball_a', 'ball_b')
TABLE_SETS = ('table_a',)
BALL_CASES = BALL_SETS + ('ball_clamp', 'ball_none_visible', 'ball_none_flagged', 'ball_none_detected', 'ball_single')
TABLE_CASES = TABLE_SETS + ('table_none_valid', 'table_only_invisible', 'table_single')
TOLERANCES = (2, 5, 10, 20)
PARITY_BAR = 1e-4          # the project's parity bar: the reference-rounding bar never exceeds it
RESTATEMENT_BAR = 1e-10    # device against the float64 restatement (DESIGN.md section 25's bar for the same comparison)
DISTANCE_KEYS = ('avg_dist', 'dist_streak')

_cache = {}


def loss_inputs(g, name):
    """-> (pred, centres (N, C, 2) float64, has_target (N, C), sigma, batches) of a loss set of the fixture."""
    pred, gt = g[name + '/pred'], g[name + '/gt']
    if name in BALL_SETS:
        centres, has = gt.reshape(-1, 1, 2), (g[name + '/vis'] != 0).astype(np.int32).reshape(-1, 1)
    else:
        centres, has = np.ascontiguousarray(gt[..., :2]), (gt[..., 2] == 1).astype(np.int32)
    return pred, centres, has, float(g[name + '/sigma']), [int(b) for b in g[name + '/batches']]


def batched_loss(sums, batches, loss_from_sums):
    """The accumulated loss over the fixture's (unequal) batches: loss_from_sums takes a batch size, the fixture's batches are
    `batch_size` samples each but for the last."""
    assert all(b == batches[0] for b in batches[:-1]) and batches[-1] <= batches[0]
    return loss_from_sums(sums, batch_size=batches[0])


def restated_losses(g):
    """{set: (unweighted sums, weighted sums, margin)} of the float64 restatement on the fixture's heatmaps."""
    if 'loss' not in _cache:
        _cache['loss'] = {}
        for name in BALL_SETS + TABLE_SETS:
            pred, centres, has, sigma, _ = loss_inputs(g, name)
            _cache['loss'][name] = R.heatmap_loss_sums_both(pred, centres, has, sigma)
    return _cache['loss']


def ball_inputs(g, name, degenerate=False):
    gt = g[name + '/gt']
    if degenerate:          # inference_balldetection.py:94-106: table-variant positions, the streak (gt, gt, gt), every sample
        return g[name + '/pred_pos_table'], gt, gt, gt, np.ones(len(gt), np.int64)
    return g[name + '/pred_pos'], gt, g[name + '/gt_min'], g[name + '/gt_max'], g[name + '/vis']


def ball_items(g):
    """(case label, metric prefix in the fixture, inputs)"""
    items = [(name, name + '/metric/', ball_inputs(g, name)) for name in BALL_CASES]
    return items + [(name + ' degenerate', name + '/degenerate/', ball_inputs(g, name, True)) for name in BALL_SETS]


def table_items(g):
    return [(name, name + '/metric/', (g[name + '/pred_pos'], g[name + '/gt'])) for name in TABLE_CASES]


FULL = (R.HEIGHT, R.WIDTH)
# name -> (n, c, h, w, output size, sigma, centres): the loss kernel's edges.  'corner' / 'outside' / 'inside' / 'integer' place the
# targets; 'none' has no target anywhere.  Strips are 8 output rows: 37 and 7 rows do not fill the last one.
LOSS_EDGES = {
    'one_pixel': (1, 1, 1, 1, FULL, 6.0, 'inside'),                  # every output pixel reads the one source pixel
    'one_row': (1, 1, 1, 7, FULL, 2.5, 'corner'),
    'coarse_13': (1, 13, 11, 20, FULL, 6.0, 'integer'),              # 13 channels, a strip lies inside one source row
    'vitpose': (2, 1, 160, 288, FULL, 6.0, 'corner_outside'),        # ratio 6.75
    'wasb': (1, 1, 704, 1280, FULL, 2.5, 'inside'),                  # ratio 1.534: 7 source rows per strip
    'identity': (1, 1, 1080, 1920, FULL, 6.0, 'inside'),             # up is the identity; 9 rows would not fit, the strip shrinks to 7
    'identity_small': (2, 3, 37, 53, (37, 53), 2.5, 'inside'),
    'wide': (1, 2, 8, 2048, FULL, 6.0, 'inside'),                    # wider than the output: columns are skipped
    'odd_output': (3, 2, 22, 40, (37, 53), 2.5, 'inside'),           # 37 = 4 strips of 8 + 5; three samples for batch_size 2
    'shrink': (2, 2, 64, 50, (7, 9), 6.0, 'inside'),                 # far-apart source rows: every output row keeps its own pair
    'no_target': (1, 2, 11, 20, FULL, 6.0, 'none'),
}


def loss_edge(name):
    """-> (pred (n, c, h, w) float32, centres (n, c, 2) float64, has_target (n, c) int32, sigma, size), seeded by the name."""
    n, c, h, w, size, sigma, where = LOSS_EDGES[name]
    rng = np.random.default_rng(sum(name.encode()))
    pred = rng.normal(0.2, 0.3, (n, c, h, w)).astype(np.float32)
    centres = np.stack([rng.uniform(0.1 * size[1], 0.9 * size[1], (n, c)), rng.uniform(0.1 * size[0], 0.9 * size[0], (n, c))], -1)
    has = np.ones((n, c), np.int32)
    if where == 'integer':
        centres = np.floor(centres)
        has[0, 5] = 0
    elif where == 'corner':
        centres[0, 0] = (0.0, 0.0)
    elif where == 'corner_outside':
        centres[0, 0] = (size[1] - 1.0, size[0] - 1.0)
        centres[1, 0] = (-7.3, size[0] + 4.6)          # the Gaussian's flank alone reaches into the image
    elif where == 'none':
        has[:] = 0
    return pred, centres, has, sigma, size


def metric_edges(n, seed):
    """Seeded ball and table inputs of n samples: detections scattered 0 .. 30 px around the annotations, every visibility state,
    zero-length streaks, undetected and unflagged predictions."""
    rng = np.random.default_rng(seed)
    gt = np.stack([rng.uniform(50, 1870, n), rng.uniform(50, 1030, n)], 1).astype(np.float32)
    d = rng.normal(0, 1, (n, 2))
    lo = (gt - d * rng.uniform(0, 30, (n, 1))).astype(np.float32)
    hi = (gt + d * rng.uniform(0, 30, (n, 1))).astype(np.float32)
    lo[::5], hi[::5] = gt[::5], gt[::5]
    pred = np.concatenate([gt + rng.normal(0, 1, (n, 2)) * rng.uniform(0, 30, (n, 1)), np.ones((n, 1))], 1)
    pred[1::7, 2] = 0
    pred[3::11, :2] = -1000.0
    vis = rng.choice([1, 1, 1, 0, -1], n)
    tgt = np.concatenate([np.floor(rng.uniform(0, 1900, (n, 13, 2))), rng.choice([1.0, 1.0, 0.0], (n, 13, 1))], 2)
    tpred = np.concatenate([tgt[..., :2] + rng.normal(0, 1, (n, 13, 2)) * rng.uniform(0, 15, (n, 13, 1)), rng.choice([1.0, 1.0, 1.0, 0.0], (n, 13, 1))], 2)
    return (pred, gt, lo, hi, vis), (tpred, tgt)


def rel(a, b):
    return abs(a - b) / abs(b)


def reference_rounding(g):
    """The largest relative distance between a value the reference computed in fp32 (per-map sums, accumulated losses, distances) and
    the float64 restatement of it: the reference's own rounding, from the fixture alone."""
    if 'rounding' not in _cache:
        worst = 0.0
        for name, (mse, wgt, _) in restated_losses(g).items():
            batches = [int(b) for b in g[name + '/batches']]
            for key, sums in (('mse', mse), ('weighted', wgt)):
                worst = max(worst, float(np.max(np.abs(sums - g['%s/sums_%s' % (name, key)]) / np.abs(g['%s/sums_%s' % (name, key)]))))
                worst = max(worst, rel(batched_loss(sums, batches, R.loss_from_sums), float(g['%s/loss_%s' % (name, key)])))
        for _, prefix, inputs in ball_items(g):
            d = R.ball_metrics(*inputs, tolerances=TOLERANCES)
            for k in DISTANCE_KEYS:
                if d['detected']:
                    worst = max(worst, rel(d[k], float(g[prefix + k])))
        for _, prefix, inputs in table_items(g):
            d = R.table_metrics(*inputs, tolerances=TOLERANCES)
            if d['valid_visible']:
                worst = max(worst, rel(d['avg_dist'], float(g[prefix + 'avg_dist'])))
        _cache['rounding'] = worst
    return _cache['rounding']


def reference_bar(g):
    """Ten times the reference's own rounding, never above the project's parity bar."""
    return min(10.0 * reference_rounding(g), PARITY_BAR)


def check_metrics(d, g, prefix, keys, bar):
    """A metrics dict against the reference's returns: ratios of counts to 1e-12, distances to `bar`, sentinels and NaN exactly."""
    for k in keys:
        want, have = float(g[prefix + k]), d[k]
        if np.isnan(want) or want in (-1.0, 10000.0):
            assert R.same(have, want), (prefix, k, have, want)
        elif k in DISTANCE_KEYS:
            assert R.same(have, want, bar), (prefix, k, have, want)
        else:
            assert abs(have - want) <= 1e-12, (prefix, k, have, want)
