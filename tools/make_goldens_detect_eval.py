#!/usr/bin/env python3
"""Generate tests/golden/detect_eval.npz by running the REFERENCE's own detector-evaluation functions on the CPU.

Runs only where the reference sources are (TTUP_REFERENCE); the tests read the .npz alone.  tensorboard / cv2 are stubbed as in
tools/make_goldens.py.  No model and no dataset: the predictions are recorded heatmaps (a seeded Gaussian blob near the annotated
position plus noise), pushed batch by batch through the statements of the reference's val():

  * positions: ball and table `extract_position_torch_gaussian(pred, WIDTH, HEIGHT)`;
  * loss: `F.interpolate(pred, size=(HEIGHT, WIDTH), mode='bilinear')` against the loaders' `create_heatmap` target (zeros for an
    invisible ball / keypoint) interpolated to the same size, through nn.MSELoss and through both `weighted_mse_loss`, accumulated
    as `loss += loss_fn(...).item() / len(valloader)`; and the same squared errors summed per (sample, channel) in torch fp32;
  * metrics: both `calculate_pck_fixed_tolerance` at 2, 5, 10, 20 px, `average_distance`, `distance_to_streak` (called as
    balldetection/train.py:220 calls it), `ratio_detected`, on the extracted positions and on hand-made cases for the sentinels.

Fixture conditions, asserted from the reference's numbers alone (a seed that misses one is skipped and reported): no target pixel
within 1e-6 of the 0.1 weight threshold; no streak or keypoint distance within 1e-3 px of a tolerance; no segment with L^2 within a
factor 10 of 1e-12 unless it is exactly 0; every metric has a non-empty denominator in a case and each sentinel a case of its own.

    python tools/make_goldens_detect_eval.py
"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TTUP_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from tools.make_goldens import install_stubs  # noqa: E402

HEIGHT, WIDTH = 1080, 1920
TOLERANCES = (2, 5, 10, 20)
# name -> (heatmap size, batches, sigma)
BALL_SETS = {'ball_a': ((22, 40), (4, 4, 3), 6.0), 'ball_b': ((44, 80), (2, 2, 1), 2.5)}
TABLE_SETS = {'table_a': ((22, 40), (2, 1), 6.0)}


class Miss(Exception):
    """A fixture condition this seed does not meet."""


def blobs(rng, centres, hw, spread):
    """One (h, w) float32 heatmap per centre ((M, 2) evaluation pixels): a Gaussian blob `spread` heatmap pixels (per centre) off the
    annotated position, plus noise."""
    h, w = hw
    y, x = np.mgrid[:h, :w].astype(np.float64)
    out = np.zeros((len(centres), h, w), np.float32)
    for k, (cx, cy) in enumerate(centres):
        mx = (cx + 0.5) * w / WIDTH - 0.5 + rng.normal(0, spread[k])
        my = (cy + 0.5) * h / HEIGHT - 0.5 + rng.normal(0, spread[k])
        s = rng.uniform(0.9, 1.6)
        out[k] = rng.uniform(0.5, 1.0) * np.exp(-((x - mx) ** 2 + (y - my) ** 2) / (2 * s * s)) + rng.normal(0, 0.01, (h, w))
    return out


def check_targets(hm):
    m = float((hm - np.float32(0.1)).abs().min())
    if m < 1e-6:
        raise Miss('a target pixel lies %.2e from the weight threshold' % m)
    return m


def run_loss(pred, make_target, batches, losses):
    """val()'s loss statements over the batches -> ({name: accumulated loss}, {name: per-(sample, channel) fp32 sums}, margin)."""
    total = {k: 0.0 for k in losses}
    sums = {k: [] for k in losses}
    at, margin = 0, np.inf
    for b in batches:
        p = F.interpolate(torch.from_numpy(pred[at:at + b].copy()), size=(HEIGHT, WIDTH), mode='bilinear')
        hm = F.interpolate(make_target(at, at + b), size=(HEIGHT, WIDTH), mode='bilinear')
        margin = min(margin, check_targets(hm))
        for k, (fn, weighted) in losses.items():
            total[k] += fn(p, hm).item() / len(batches)
            wgt = torch.where(hm > 0.1, torch.ones_like(hm) * 100, torch.ones_like(hm)) if weighted else torch.ones_like(hm)
            sums[k].append((wgt * (p - hm) ** 2).sum(dim=(2, 3)).numpy().astype(np.float64))
        at += b
    return total, {k: np.concatenate(v) for k, v in sums.items()}, margin


def check_distances(d, what):
    d = np.asarray(d, np.float64)
    for t in TOLERANCES:
        m = np.abs(d - t).min() if d.size else np.inf
        if m < 1e-3:
            raise Miss('%s: a distance lies %.2e px from the tolerance %d' % (what, m, t))


def check_segments(bh, a, b, what):
    seg = np.asarray(b, np.float32) - np.asarray(a, np.float32)
    l2 = np.sum(seg ** 2, axis=1)
    bad = (l2 != 0) & (l2 > 1e-13) & (l2 < 1e-11)
    if bad.any():
        raise Miss('%s: a segment has L^2 = %g' % (what, l2[bad][0]))


def ball_case(bh, pred_pos, gt, lo, hi, vis):
    """The metric block of the ball val() (train.py:207-220) on one case -> dict of the reference's returns."""
    m = np.asarray(vis) == bh.BALL_VISIBLE
    pred_pos, gt, lo, hi = (np.array(a, dtype=np.float32) for a in (pred_pos, gt, lo, hi))
    out = {}
    for t in TOLERANCES:
        out['pck@%d' % t] = bh.calculate_pck_fixed_tolerance(pred_pos[m], gt[m], lo[m], hi[m], tolerance_pixels=t)
    out['avg_dist'] = bh.average_distance(pred_pos[m][:, :2], gt[m])
    out['dist_streak'] = bh.distance_to_streak(pred_pos[m][:, :2], gt[m], lo[m], hi[m])
    if m.any():
        p = pred_pos[m][:, :2]
        check_distances(np.minimum(bh._batched_distance_point_to_segment(p, lo[m], gt[m]), bh._batched_distance_point_to_segment(p, gt[m], hi[m])), 'ball PCK')
        for a, b in ((lo[m], gt[m]), (gt[m], hi[m]), (gt[m], lo[m]), (lo[m], hi[m])):
            check_segments(bh, a, b, 'ball')
    return {k: np.float64(v) for k, v in out.items()}


def table_case(th, pred_pos, gt):
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # the 0 / 0 of a case without a valid & visible keypoint
        for t in TOLERANCES:
            out['pck@%d' % t] = th.calculate_pck_fixed_tolerance(pred_pos, gt, tolerance_pixels=t)
        out['avg_dist'] = th.average_distance(pred_pos, gt)
        out['ratio_detected'] = th.ratio_detected(pred_pos)
    p, g = np.array(pred_pos, dtype=np.float32), np.array(gt, dtype=np.float32)
    both = (p[..., 2] == th.KEYPOINT_VISIBLE) & (g[..., 2] == th.KEYPOINT_VISIBLE)
    check_distances(np.sqrt(np.sum((p[..., :2] - g[..., :2]) ** 2, axis=2))[both], 'table PCK')
    return {k: np.float64(v) for k, v in out.items()}


def streaks(rng, gt):
    """Blur-streak ends around gt (N, 2): random direction and length; every fourth sample has no streak at all (min == gt == max)."""
    n = len(gt)
    ang = rng.uniform(0, 2 * np.pi, n)
    d = np.stack([np.cos(ang), np.sin(ang)], 1)
    lo = gt - d * rng.uniform(2, 25, (n, 1))
    hi = gt + (d + rng.normal(0, 0.2, (n, 2))) * rng.uniform(2, 25, (n, 1))
    lo[::4], hi[::4] = gt[::4], gt[::4]
    return lo, hi


def generate(seed, bh, th, bds, tds):
    rng = np.random.default_rng(seed)
    out = {'seed': np.int64(seed), 'tolerances': np.array(TOLERANCES, np.float64)}
    margins = []
    for name, (hw, batches, sigma) in BALL_SETS.items():
        n = sum(batches)
        gt = np.stack([rng.uniform(60, WIDTH - 60, n), rng.uniform(60, HEIGHT - 60, n)], 1)          # float64, as the loader holds them
        gt[0] = (3.25, 2.5)                                                                              # a ball in the corner
        vis = np.ones(n, np.int64)
        vis[2], vis[n - 1] = bh.BALL_INVISIBLE, bh.BALL_OCCLUDED
        pred = blobs(rng, gt, hw, rng.choice([0.01, 0.03, 0.08, 0.2], n))[:, None]
        lo, hi = streaks(rng, gt)

        def make_target(b0, b1, gt=gt, vis=vis, sigma=sigma):
            hms = [np.zeros((HEIGHT, WIDTH)) if vis[i] == bh.BALL_INVISIBLE else bds.TTHQ.create_heatmap(None, (gt[i, 0], gt[i, 1]), (HEIGHT, WIDTH), sigma=sigma)
                   for i in range(b0, b1)]
            return torch.stack([torch.tensor(hm).unsqueeze(0).float() for hm in hms])
        total, sums, margin = run_loss(pred, make_target, batches, {'mse': (torch.nn.MSELoss(), False), 'weighted': (bh.weighted_mse_loss, True)})
        margins.append(margin)
        pos = bh.extract_position_torch_gaussian(torch.from_numpy(pred.copy()), WIDTH, HEIGHT)
        pos_table = th.extract_position_torch_gaussian(torch.from_numpy(pred.copy()), WIDTH, HEIGHT).reshape(n, 3)          # inference_balldetection.py:94
        out.update({name + '/pred': pred, name + '/gt': gt, name + '/gt_min': lo.astype(np.float32), name + '/gt_max': hi.astype(np.float32), name + '/vis': vis,
                    name + '/sigma': np.float64(sigma), name + '/batches': np.array(batches, np.int64), name + '/pred_pos': pos, name + '/pred_pos_table': pos_table})
        for k in total:
            out['%s/loss_%s' % (name, k)] = np.float64(total[k])
            out['%s/sums_%s' % (name, k)] = sums[k]
        for k, v in ball_case(bh, pos, gt, lo, hi, vis).items():
            out['%s/metric/%s' % (name, k)] = v
        # the inference script's call: every sample, the degenerate streak (gt, gt, gt), the table-variant positions
        for k, v in ball_case(bh, pos_table, gt, gt, gt, np.ones(n, np.int64)).items():
            out['%s/degenerate/%s' % (name, k)] = v

    # hand-made ball cases: one per sentinel, and the clamp of t at both ends
    gt = np.array([[500.0, 400.0], [900.0, 300.0], [1200.0, 800.0], [300.0, 900.0]])
    lo, hi = gt + np.array([-20.0, 0.0]), gt + np.array([0.0, 30.0])
    near = np.concatenate([gt + np.array([[-31.5, 0.7], [0.4, 37.25], [-8.0, 3.3], [1.6, 11.0]]), np.ones((4, 1))], 1)          # before lo, past hi, inside
    cases = {
        'ball_clamp': (near, gt, lo, hi, np.ones(4, np.int64)),
        'ball_none_visible': (near, gt, lo, hi, np.array([0, -1, 0, 0], np.int64)),                  # PCK -1, both distances 10000
        'ball_none_flagged': (near * np.array([1, 1, 0]), gt, lo, hi, np.ones(4, np.int64)),           # PCK -1 alone
        'ball_none_detected': (np.concatenate([np.full((4, 2), -1000.0), np.ones((4, 1))], 1), gt, lo, hi, np.ones(4, np.int64)),          # 10000 twice
        'ball_single': (near[2:3], gt[2:3], lo[2:3], hi[2:3], np.ones(1, np.int64)),
    }
    for name, (p, g, a, b, v) in cases.items():
        out.update({name + '/pred_pos': p, name + '/gt': g, name + '/gt_min': a.astype(np.float32), name + '/gt_max': b.astype(np.float32), name + '/vis': v})
        for k, val in ball_case(bh, p, g, a, b, v).items():
            out['%s/metric/%s' % (name, k)] = val

    for name, (hw, batches, sigma) in TABLE_SETS.items():
        n = sum(batches)
        coords = np.zeros((n, 13, 3))
        coords[..., 0] = rng.integers(40, WIDTH - 40, (n, 13))          # the loader's int() pixel positions
        coords[..., 1] = rng.integers(40, HEIGHT - 40, (n, 13))
        coords[..., 2] = th.KEYPOINT_VISIBLE
        coords[0, 3, 2] = coords[1, 7, 2] = coords[n - 1, 12, 2] = 0
        coords[0, 0, :2] = (0, 0)
        pred = blobs(rng, coords[..., :2].reshape(-1, 2), hw, rng.choice([0.01, 0.03, 0.08, 0.2], n * 13)).reshape(n, 13, *hw)

        def make_target(b0, b1, coords=coords, sigma=sigma):
            hms = np.zeros((b1 - b0, 13, HEIGHT, WIDTH), dtype=np.float32)
            for i in range(b0, b1):
                for j, (x, y, v) in enumerate(coords[i]):
                    if v == th.KEYPOINT_VISIBLE:
                        hms[i - b0, j] = tds.TTHQ.create_heatmap(None, (x, y), (HEIGHT, WIDTH), sigma=sigma)
            return torch.tensor(hms).float()
        wl = lambda p, hm: th.weighted_mse_loss(p, hm, None)          # noqa: E731  (the visibilities argument is unused there)
        total, sums, margin = run_loss(pred, make_target, batches, {'mse': (torch.nn.MSELoss(), False), 'weighted': (wl, True)})
        margins.append(margin)
        pos = th.extract_position_torch_gaussian(torch.from_numpy(pred.copy()), WIDTH, HEIGHT)
        out.update({name + '/pred': pred, name + '/gt': coords, name + '/sigma': np.float64(sigma), name + '/batches': np.array(batches, np.int64), name + '/pred_pos': pos})
        for k in total:
            out['%s/loss_%s' % (name, k)] = np.float64(total[k])
            out['%s/sums_%s' % (name, k)] = sums[k]
        for k, v in table_case(th, pos, coords).items():
            out['%s/metric/%s' % (name, k)] = v
        none_valid = pos * np.array([1, 1, 0])
        only_invisible = pos.copy()          # valid exactly where the annotation is not visible: 0 / 0
        only_invisible[..., 2] = (coords[..., 2] != th.KEYPOINT_VISIBLE)
        for case, p in (('table_none_valid', none_valid), ('table_only_invisible', only_invisible), ('table_single', pos[:1])):
            g = coords[:1] if case == 'table_single' else coords
            out.update({case + '/pred_pos': p, case + '/gt': g})
            for k, v in table_case(th, p, g).items():
                out['%s/metric/%s' % (case, k)] = v

    # every metric has a non-empty denominator somewhere, every sentinel a case of its own
    m = lambda k: float(out[k])          # noqa: E731
    if not (0 < m('ball_a/metric/pck@5') <= 1 and 0 < m('ball_a/metric/avg_dist') < 10000 and 0 < m('ball_a/metric/dist_streak') < 10000 and
            0 < m('table_a/metric/pck@5') <= 1 and 0 < m('table_a/metric/avg_dist') < 10000 and 0 < m('table_a/metric/ratio_detected') <= 1):
        raise Miss('a main case has an empty metric')
    if not (m('ball_a/metric/pck@2') < m('ball_a/metric/pck@20') and m('table_a/metric/pck@2') < m('table_a/metric/pck@20')):
        raise Miss('the tolerances do not separate the detections')
    assert m('ball_none_visible/metric/pck@5') == -1 and m('ball_none_visible/metric/avg_dist') == 10000 and m('ball_none_visible/metric/dist_streak') == 10000
    assert m('ball_none_flagged/metric/pck@5') == -1 and m('ball_none_flagged/metric/avg_dist') < 10000
    assert m('ball_none_detected/metric/avg_dist') == 10000 and m('ball_none_detected/metric/dist_streak') == 10000 and m('ball_none_detected/metric/pck@5') >= 0
    assert m('table_none_valid/metric/pck@5') == -1 and m('table_none_valid/metric/avg_dist') == 10000 and m('table_none_valid/metric/ratio_detected') == 0
    assert np.isnan(m('table_only_invisible/metric/pck@5')) and np.isnan(m('table_only_invisible/metric/avg_dist'))
    out['target_margin'] = np.float64(min(margins))
    return out


def main():
    install_stubs()
    import balldetection.dataset as bds
    import balldetection.helper_balldetection as bh
    import tabledetection.dataset as tds
    import tabledetection.helper_tabledetection as th
    assert (bh.HEIGHT, bh.WIDTH, th.HEIGHT, th.WIDTH) == (HEIGHT, WIDTH, HEIGHT, WIDTH) and bh.BALL_VISIBLE == th.KEYPOINT_VISIBLE == 1
    for seed in range(20260, 20280):
        try:
            out = generate(seed, bh, th, bds, tds)
            break
        except Miss as e:
            print('seed %d skipped: %s' % (seed, e))
    else:
        raise SystemExit('no seed meets the fixture conditions')
    path = os.path.join(ROOT, 'tests', 'golden', 'detect_eval.npz')
    np.savez_compressed(path, **out)
    print('seed %d, target margin %.3e' % (seed, float(out['target_margin'])))
    print(path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
