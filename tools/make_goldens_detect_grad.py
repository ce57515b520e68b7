#!/usr/bin/env python3
"""Generate tests/golden/detect_grad.npz by running the REFERENCE's own detector training-loss statements with autograd, on the CPU.

Runs only where the reference sources are (TTUP_REFERENCE); the tests read the .npz alone.  No model and no dataset: the network's
output is a recorded heatmap (the generator of tools/make_goldens_detect_eval.py: a seeded Gaussian blob near the annotated position
plus noise, at (22, 40) and (44, 80)), made a leaf that requires a gradient and pushed through the statements of train()
(balldetection/train.py:112-119, tabledetection/train.py:106-108):

    pred = F.interpolate(pred_seg, size=(heat_H, heat_W), mode='bilinear');  loss = loss_fn(pred, heatmap);  loss.backward()

with loss_fn both `weighted_mse_loss` (the training loss of either detector) and nn.MSELoss, and the target the loaders'
`create_heatmap` (zeros for an invisible ball / keypoint).  Recorded per case: the inputs, loss.item() and pred_seg.grad.

Cases: ball and table, weighted and not, at 1080 x 1920 and at a small odd size; a ball without target, a ball whose centre lies
outside the image, a keypoint without target.  Fixture condition, asserted from the reference's numbers alone (a seed that misses
it is skipped and reported): no target pixel within 1e-6 of the 0.1 weight threshold.

    python tools/make_goldens_detect_grad.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TTUP_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from tools.make_goldens import install_stubs  # noqa: E402
from tools.make_goldens_detect_eval import Miss, blobs, check_targets  # noqa: E402

HEIGHT, WIDTH = 1080, 1920
SMALL = (135, 241)          # the small odd output size: ratios 6.1 / 6.0 from (22, 40), 3.07 / 3.01 from (44, 80)
LIMIT = 267408              # bytes of tests/golden/detect_eval.npz: this fixture is no larger


def blobs_at(rng, centres, hw, size, spread):
    """tools/make_goldens_detect_eval.py's generator for annotations in pixels of `size`: it places its blobs from 1080 x 1920
    positions, so the centres go in stretched to that frame."""
    full = np.asarray(centres, np.float64) * np.array([WIDTH / size[1], HEIGHT / size[0]])
    return blobs(rng, full, hw, spread)


def backward(pred, heatmap, loss_fn):
    """train()'s statements on the recorded network output -> (loss.item(), pred_seg.grad)."""
    pred_seg = torch.from_numpy(pred.copy()).requires_grad_(True)
    up = F.interpolate(pred_seg, size=tuple(heatmap.shape[2:]), mode='bilinear')
    loss = loss_fn(up, heatmap)
    loss.backward()
    return np.float64(loss.item()), pred_seg.grad.numpy().copy()


def generate(seed, bh, th, bds, tds):
    rng = np.random.default_rng(seed)
    out = {'seed': np.int64(seed)}
    margins = []
    ball_losses = {'weighted': bh.weighted_mse_loss, 'mse': torch.nn.MSELoss()}
    table_losses = {'weighted': lambda p, hm: th.weighted_mse_loss(p, hm, None), 'mse': torch.nn.MSELoss()}          # (the visibilities argument is unused there)

    # name -> (heatmap size, samples, sigma, output size, losses recorded)
    for name, (hw, n, sigma, size, keys) in {'ball_a': ((22, 40), 3, 6.0, (HEIGHT, WIDTH), ('weighted', 'mse')),
                                             'ball_b': ((44, 80), 1, 2.5, SMALL, ('weighted', 'mse'))}.items():
        gt = np.stack([rng.uniform(0.05 * size[1], 0.95 * size[1], n), rng.uniform(0.05 * size[0], 0.95 * size[0], n)], 1)          # float64, as the loader holds them
        vis = np.ones(n, np.int64)
        if n > 1:
            vis[1] = bh.BALL_INVISIBLE                       # no target: zeros
            gt[2] = (size[1] + 5.5, -3.25)                   # outside the image: the Gaussian's flank alone reaches into it
        pred = blobs_at(rng, gt, hw, size, rng.choice([0.01, 0.03, 0.08, 0.2], n))[:, None]
        hms = [np.zeros(size) if vis[i] == bh.BALL_INVISIBLE else bds.TTHQ.create_heatmap(None, (gt[i, 0], gt[i, 1]), size, sigma=sigma) for i in range(n)]
        heatmap = torch.stack([torch.tensor(hm).unsqueeze(0).float() for hm in hms])          # dataset.py: torch.tensor(heatmap).unsqueeze(0).float()
        margins.append(check_targets(heatmap))
        out.update({name + '/pred': pred, name + '/gt': gt, name + '/vis': vis, name + '/sigma': np.float64(sigma), name + '/size': np.array(size, np.int64)})
        for k in keys:
            out['%s/loss_%s' % (name, k)], out['%s/grad_%s' % (name, k)] = backward(pred, heatmap, ball_losses[k])

    # table_b evaluates table_a's recorded heatmaps at the small size (its annotations are table_a's in pixels of that size): one
    # (1, 13, 22, 40) tensor serves both, which keeps the fixture within LIMIT
    for name, (hw, sigma, size, keys) in {'table_a': ((22, 40), 6.0, (HEIGHT, WIDTH), ('weighted', 'mse')),
                                          'table_b': ((22, 40), 2.5, SMALL, ('weighted',))}.items():
        if name == 'table_a':
            coords = np.zeros((1, 13, 3))
            coords[..., 0] = rng.integers(40, WIDTH - 40, (1, 13))          # the loader's int() pixel positions
            coords[..., 1] = rng.integers(40, HEIGHT - 40, (1, 13))
            coords[..., 2] = th.KEYPOINT_VISIBLE
            coords[0, 3, 2] = coords[0, 12, 2] = 0
            coords[0, 0, :2] = (0, 0)
            pred = blobs(rng, coords[0, :, :2], hw, rng.choice([0.01, 0.03, 0.08, 0.2], 13))[None]
            out[name + '/pred'] = pred
        else:
            coords = out['table_a/gt'].copy()
            coords[..., 0] = np.floor(coords[..., 0] * size[1] / WIDTH)
            coords[..., 1] = np.floor(coords[..., 1] * size[0] / HEIGHT)
            pred = out['table_a/pred']
        hms = np.zeros((1, 13) + tuple(size), dtype=np.float32)
        for j, (x, y, v) in enumerate(coords[0]):
            if v == th.KEYPOINT_VISIBLE:
                hms[0, j] = tds.TTHQ.create_heatmap(None, (x, y), size, sigma=sigma)
        heatmap = torch.tensor(hms).float()
        margins.append(check_targets(heatmap))
        out.update({name + '/gt': coords, name + '/sigma': np.float64(sigma), name + '/size': np.array(size, np.int64)})
        for k in keys:
            out['%s/loss_%s' % (name, k)], out['%s/grad_%s' % (name, k)] = backward(pred, heatmap, table_losses[k])

    for k, v in out.items():
        if '/grad_' in k:
            assert v.dtype == np.float32 and v.shape[2:] in ((22, 40), (44, 80)) and np.isfinite(v).all() and np.abs(v).max() > 0
    out['target_margin'] = np.float64(min(margins))
    return out


def main():
    install_stubs()
    import balldetection.dataset as bds
    import balldetection.helper_balldetection as bh
    import tabledetection.dataset as tds
    import tabledetection.helper_tabledetection as th
    assert (bh.HEIGHT, bh.WIDTH, th.HEIGHT, th.WIDTH) == (HEIGHT, WIDTH, HEIGHT, WIDTH) and bh.BALL_INVISIBLE == 0 and th.KEYPOINT_VISIBLE == 1
    for seed in range(20280, 20300):
        try:
            out = generate(seed, bh, th, bds, tds)
            break
        except Miss as e:
            print('seed %d skipped: %s' % (seed, e))
    else:
        raise SystemExit('no seed meets the fixture conditions')
    path = os.path.join(ROOT, 'tests', 'golden', 'detect_grad.npz')
    np.savez_compressed(path, **out)
    print('seed %d, target margin %.3e' % (seed, float(out['target_margin'])))
    print(path, os.path.getsize(path), 'bytes,', len(out), 'arrays')
    assert os.path.getsize(path) <= LIMIT


if __name__ == '__main__':
    main()
