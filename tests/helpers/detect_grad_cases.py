"""What tests/test_detect_grad_host.py and tests/test_detect_grad_gpu.py share: the cases of tests/golden/detect_grad.npz, the float64
restatement (tests/helpers/detect_grad_ref.py) evaluated on them and on the LOSS_EDGES shapes (once per process, never modified),
and the reference's own fp32 rounding measured from the fixture."""
import numpy as np

from . import detect_eval_cases as C
from . import detect_eval_ref as R
from . import detect_grad_ref as G

# (set, loss key) of the fixture: the reference's loss.item() and pred_seg.grad of each
FIXTURE_CASES = (('ball_a', 'weighted'), ('ball_a', 'mse'), ('ball_b', 'weighted'), ('ball_b', 'mse'), ('table_a', 'weighted'), ('table_a', 'mse'),
                 ('table_b', 'weighted'))
PRED_OF = {'table_b': 'table_a'}          # table_b evaluates table_a's recorded heatmaps at the small size

_cache = {}


def fixture_inputs(g, name):
    """-> (pred, centres (N, C, 2) float64, has_target (N, C) int32, sigma, size) of a set of the fixture."""
    pred, gt = g[PRED_OF.get(name, name) + '/pred'], g[name + '/gt']
    if name.startswith('ball'):
        centres, has = gt.reshape(-1, 1, 2), (g[name + '/vis'] != 0).astype(np.int32).reshape(-1, 1)
    else:
        centres, has = np.ascontiguousarray(gt[..., :2]), (gt[..., 2] == 1).astype(np.int32)
    return pred, centres, has, float(g[name + '/sigma']), tuple(int(v) for v in g[name + '/size'])


def restated_fixture(g, name, key):
    """The float64 restatement's gradient (of the element mean) of a fixture case, read-only."""
    k = ('fixture', name, key)
    if k not in _cache:
        pred, centres, has, sigma, size = fixture_inputs(g, name)
        _cache[k] = G.heatmap_loss_grad(pred, centres, has, sigma, key == 'weighted', size)
        _cache[k].setflags(write=False)
    return _cache[k]


# Downsampling shapes beside LOSS_EDGES, name -> (n, c, h, w, output size, sigma): ratios at which (dst + 0.5) in / out - 0.5 is an
# integer for some dst in exact arithmetic (17 -> 7: dst 3 -> 8; 34 -> 14, 39 -> 9 likewise).  With in / out rounded, the three
# separately rounded operations and a fused multiply-subtract land on different sides of that integer and read different source
# indices, so these shapes tell a kernel that contracts the coordinate from the plan the host checks.
SKIP_EDGES = {
    'skip_17_34': (2, 2, 17, 34, (7, 14), 2.5),
    'skip_39_34': (1, 3, 39, 34, (9, 14), 6.0),
}
GRAD_EDGES = tuple(sorted(C.LOSS_EDGES)) + tuple(sorted(SKIP_EDGES))
UNREAD_EDGES = ('wide', 'shrink') + tuple(sorted(SKIP_EDGES))          # the cases whose unread rows / columns are checked bit by bit


def edge(name):
    """-> (pred, centres, has_target, sigma, size) of a LOSS_EDGES or SKIP_EDGES case, seeded by the name."""
    if name in C.LOSS_EDGES:
        return C.loss_edge(name)
    n, c, h, w, size, sigma = SKIP_EDGES[name]
    rng = np.random.default_rng(sum(name.encode()))
    pred = rng.normal(0.2, 0.3, (n, c, h, w)).astype(np.float32)
    centres = np.stack([rng.uniform(0.1 * size[1], 0.9 * size[1], (n, c)), rng.uniform(0.1 * size[0], 0.9 * size[0], (n, c))], -1)
    return pred, centres, np.ones((n, c), np.int32), sigma, size


def edge_axes(name):
    """-> ((h, out_h), (w, out_w)) of a case: the (in, out) pair of each axis."""
    pred, _, _, _, size = edge(name)
    return (pred.shape[2], size[0]), (pred.shape[3], size[1])


def restated_edge(name, weighted):
    """The restatement's gradient (of the element mean) of a LOSS_EDGES or SKIP_EDGES case, read-only."""
    k = ('edge', name, bool(weighted))
    if k not in _cache:
        pred, centres, has, sigma, size = edge(name)
        _cache[k] = G.heatmap_loss_grad(pred, centres, has, sigma, weighted, size)
        _cache[k].setflags(write=False)
    return _cache[k]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def reference_rounding(g):
    """The largest relative-L2 distance, over the fixture's tensors, between the gradient the reference computed in fp32 and the
    float64 restatement of it: the reference's own rounding, from the fixture alone."""
    if 'rounding' not in _cache:
        _cache['rounding'] = max(rel_l2(g['%s/grad_%s' % (name, key)], restated_fixture(g, name, key)) for name, key in FIXTURE_CASES)
    return _cache['rounding']


def reference_bar(g):
    """Ten times the reference's own rounding, never above the project's parity bar."""
    return min(10.0 * reference_rounding(g), C.PARITY_BAR)


def restated_loss(g, name, key):
    """The restatement's loss (element mean) of a fixture case."""
    k = ('loss', name)
    if k not in _cache:
        pred, centres, has, sigma, size = fixture_inputs(g, name)
        mse, wgt, margin = R.heatmap_loss_sums_both(pred, centres, has, sigma, size)
        _cache[k] = {'mse': R.loss_from_sums(mse, size), 'weighted': R.loss_from_sums(wgt, size), 'margin': margin}
    return _cache[k][key]


def loss_bar(g):
    """detect_eval_cases.reference_bar's rule on this fixture's losses: ten times the largest relative distance between a loss the
    reference computed in fp32 and the restatement's, never above the parity bar."""
    worst = max(C.rel(restated_loss(g, name, key), float(g['%s/loss_%s' % (name, key)])) for name, key in FIXTURE_CASES)
    return min(10.0 * worst, C.PARITY_BAR)


def ulp32(x):
    """One float32 unit in the last place at each |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)
