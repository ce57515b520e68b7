"""A float64 numpy restatement of what the reference computes when it evaluates a detector: the heatmap loss at the evaluation
resolution (balldetection/train.py:177-179, tabledetection/train.py:154-156, both weighted_mse_loss) and the position metrics
(helper_balldetection.py:205-458, helper_tabledetection.py:279-382).  tests/test_detect_eval_host.py pins it to what the reference's
own functions returned (tests/golden/detect_eval.npz); the GPU tests use it for the shapes the fixture does not hold.

Inputs are rounded to float32 where the reference holds float32 (heatmaps, positions, annotations) and every operation after that
is float64, which is what csrc/detect_eval.hip does."""
import numpy as np

HEIGHT, WIDTH = 1080, 1920
VISIBLE = 1
TOLERANCES = (2, 5, 10, 20)


def src_coords(out, inp):
    """torch's bilinear source coordinates, align_corners=False: (i0, i1, lambda) per output index."""
    s = np.maximum((np.arange(out, dtype=np.float64) + 0.5) * (np.float64(inp) / np.float64(out)) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), inp - 1)
    i1 = np.minimum(i0 + 1, inp - 1)
    return i0, i1, s - i0


def upsample(pred, size):
    """F.interpolate(pred, size, mode='bilinear') of one (h, w) map, in float64."""
    p = np.asarray(pred, np.float32).astype(np.float64)
    y0, y1, ly = src_coords(size[0], p.shape[0])
    x0, x1, lx = src_coords(size[1], p.shape[1])
    top = p[y0][:, x0] * (1.0 - lx) + p[y0][:, x1] * lx
    bot = p[y1][:, x0] * (1.0 - lx) + p[y1][:, x1] * lx
    return top * (1.0 - ly)[:, None] + bot * ly[:, None]


def target(centre, sigma, size):
    """dataset.create_heatmap followed by torch.tensor(...).float(): one float32 rounding of the float64 exp."""
    y, x = np.ogrid[:size[0], :size[1]]
    return np.exp(-((x - np.float64(centre[0])) ** 2 + (y - np.float64(centre[1])) ** 2) / (2 * np.float64(sigma) ** 2)).astype(np.float32)


def heatmap_loss_sums_both(pred, centres, has_target, sigma=6, size=(HEIGHT, WIDTH)):
    """-> (unweighted sums (N, C), weighted sums (N, C), the smallest |target - 0.1| over all target pixels: how far a weight is
    from flipping)."""
    pred = np.asarray(pred, np.float32)
    n, c = pred.shape[:2]
    mse, wgt, margin = np.zeros((n, c)), np.zeros((n, c)), np.inf
    for i in range(n):
        for j in range(c):
            up = upsample(pred[i, j], size)
            if has_target[i][j]:
                t = target(centres[i][j], sigma, size)
                margin = min(margin, float(np.abs(t.astype(np.float64) - np.float64(np.float32(0.1))).min()))
                d2 = (up - t.astype(np.float64)) ** 2
                mse[i, j], wgt[i, j] = d2.sum(), (np.where(t > np.float32(0.1), 100.0, 1.0) * d2).sum()
            else:
                mse[i, j] = wgt[i, j] = (up ** 2).sum()
    return mse, wgt, margin


def heatmap_loss_sums(pred, centres, has_target, sigma=6, weighted=False, size=(HEIGHT, WIDTH)):
    """-> (sums (N, C) float64, margin) of one of the two losses."""
    mse, wgt, margin = heatmap_loss_sums_both(pred, centres, has_target, sigma, size)
    return (wgt if weighted else mse), margin


def loss_from_sums(sums, size=(HEIGHT, WIDTH), batch_size=None):
    """`loss += loss_fn(pred, heatmap).item() / len(valloader)` over batches of batch_size samples, the last one maybe smaller."""
    sums = np.asarray(sums, np.float64)
    n, c = sums.shape
    bs = n if batch_size is None else batch_size
    means = [sums[b:b + bs].sum() / (sums[b:b + bs].shape[0] * c * size[0] * size[1]) for b in range(0, n, bs)]
    return float(sum(m / len(means) for m in means))


def segment_distance(p, a, b):
    """_batched_distance_point_to_segment: (N, 2) points against the segments a -> b.  -> (distance, L^2, unclamped t)."""
    p, a, b = (np.asarray(v, np.float32).astype(np.float64).reshape(-1, 2) for v in (p, a, b))
    seg = b - a
    l2 = (seg ** 2).sum(1)
    dot = ((p - a) * seg).sum(1)
    t = np.zeros_like(l2)
    nz = l2 > 1e-12
    t[nz] = dot[nz] / l2[nz]
    closest = a + np.clip(t, 0, 1)[:, None] * seg
    return np.sqrt(((p - closest) ** 2).sum(1)), l2, t


def _div(num, den):
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.float64(num) / np.float64(den))


def ball_metrics(pred_pos, gt_pos, gt_min, gt_max, vis, tolerances=(2, 5, 10)):
    """The ball val()'s metric block (train.py:207-220) over the samples with vis == 1, with detect_eval.ball_val_metrics' keys."""
    sel = np.asarray(vis).reshape(-1) == VISIBLE
    pred = np.asarray(pred_pos, np.float32).astype(np.float64).reshape(-1, 3)[sel]
    gt, lo, hi = (np.asarray(v, np.float32).astype(np.float64).reshape(-1, 2)[sel] for v in (gt_pos, gt_min, gt_max))
    flagged = pred[:, 2] == VISIBLE
    detected = (pred[:, 0] > -100) & (pred[:, 1] > -100)
    d_pck = np.minimum(segment_distance(pred[:, :2], lo, gt)[0], segment_distance(pred[:, :2], gt, hi)[0])
    # train.py:220: distance_to_streak(pred, gt, gt_min, gt_max) into (r_pred, r_min, r_b, r_max)
    d_streak = np.minimum(segment_distance(pred[:, :2], gt, lo)[0], segment_distance(pred[:, :2], lo, hi)[0])
    d_gt = np.sqrt(((pred[:, :2] - gt) ** 2).sum(1))
    out = {}
    for t in tolerances:
        correct = int((flagged & (d_pck <= t)).sum())
        out['pck@%g' % t] = _div(correct, flagged.sum()) if flagged.any() else -1
        out['correct@%g' % t] = correct
    out['avg_dist'] = _div(d_gt[detected].sum(), detected.sum()) if detected.any() else 10000
    out['dist_streak'] = _div(d_streak[detected].sum(), detected.sum()) if detected.any() else 10000
    out.update(number=int(np.asarray(vis).size), visible=int(sel.sum()), valid=int(flagged.sum()), detected=int(detected.sum()))
    return out


def table_metrics(pred_pos, gt_pos, tolerances=(2, 5, 10)):
    """The table val()'s metric block (train.py:180-187), with detect_eval.table_val_metrics' keys."""
    pred = np.asarray(pred_pos, np.float32).astype(np.float64)
    gt = np.asarray(gt_pos, np.float32).astype(np.float64)
    valid = pred[..., 2] == VISIBLE
    both = valid & (gt[..., 2] == VISIBLE)
    d = np.sqrt(((pred[..., :2] - gt[..., :2]) ** 2).sum(-1))
    out = {}
    for t in tolerances:
        correct = int((both & (d <= t)).sum())
        out['pck@%g' % t] = _div(correct, both.sum()) if valid.any() else -1
        out['correct@%g' % t] = correct
    out['avg_dist'] = _div(d[both].sum(), both.sum()) if valid.any() else 10000
    out['ratio_detected'] = _div(valid.sum(), valid.size)
    out.update(number=int(valid.size), valid=int(valid.sum()), valid_visible=int(both.sum()))
    return out


def same(a, b, tol=0.0):
    """Two metric values agree: both NaN, or within tol (relative where the reference value b is not 0)."""
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return abs(a - b) <= tol * (abs(b) if b != 0 else 1.0)
