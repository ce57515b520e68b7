#!/usr/bin/env python3
"""Time of evaluating an uplift model on the device (MultiStageModel.val, csrc/uplift_eval.hip), one JSON line:
forward + metrics over N samples of T steps through `model.val`, the metrics launch alone (ttup_uplift_val_metrics and
ttup_uplift_val_real_metrics on preallocated buffers, device events around `--inner` back-to-back calls), and the bandwidth the
val launch achieves against its 2 * N * T * 12 bytes (pred_position and r_world; the mask and the per-sample vectors add 6 %).

Every timed call is preceded by a warm-up call of the same shape; best and mean of --repeat.  At the default size both tensors
(12 MB) stay in the last-level cache between the back-to-back calls, so the rate is not an HBM rate.

    python tools/bench_uplift_eval.py [--samples 10000] [--len 50] [--size large] [--repeat 5] [--inner 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from upliftingtabletennis_amd import _lib, uplift, weights  # noqa: E402


def host_timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), sum(ts) / len(ts)


def event_timed(launch, repeat, inner):
    """seconds per launch: device events around `inner` back-to-back launches"""
    launch()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            launch()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / inner)
    return min(ts), sum(ts) / len(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=10000)
    ap.add_argument('--len', type=int, default=50)
    ap.add_argument('--size', default='large')
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--inner', type=int, default=50)
    a = ap.parse_args()
    n, t = a.samples, a.len
    _lib.require_gpu()
    lib = _lib.load()
    rng = np.random.default_rng(0)
    f = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()          # noqa: E731
    r_img = f(rng.uniform(0.1, 0.9, (n, t, 2)))
    table = f(np.concatenate([rng.uniform(0.1, 0.9, (n, 13, 2)), np.ones((n, 13, 1))], -1))
    mask = np.ones((n, t), np.float32)
    mask[np.arange(t)[None, :] >= rng.integers(t // 2, t, (n, 1))] = 0
    times = f(np.tile(np.arange(t) * 0.02, (n, 1)) * mask)
    mask = f(mask)
    r_world, rotation = f(rng.normal(0, 1, (n, t, 3))), f(rng.normal(0, 30, (n, 3)))
    model = uplift.MultiStageModel(weights.random_uplift_state_dict(0, a.size), size=a.size, max_batch=n, max_len=t)
    res = {'samples': n, 'len': t, 'size': a.size, 'build_id': _lib.build_id()}
    best, mean = host_timed(lambda: model.val(r_img, table, mask, times, r_world, rotation, check_mask=False), a.repeat)
    res['val_forward_and_metrics_ms_best'], res['val_forward_and_metrics_ms_mean'] = best * 1e3, mean * 1e3
    best, mean = host_timed(lambda: model.forward(r_img, table, mask, times, check_mask=False), a.repeat)
    res['forward_ms_best'], res['forward_ms_mean'] = best * 1e3, mean * 1e3

    rot, pos = model.forward(r_img, table, mask, times, check_mask=False)
    nbytes = int(lib.ttup_uplift_eval_workspace_bytes(n))
    ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device='cuda')
    sums, counts = torch.empty((8,), dtype=torch.float64, device='cuda'), torch.empty((13,), dtype=torch.int64, device='cuda')
    p, st = _lib.ptr, _lib.stream_ptr()

    def launch_val():
        _lib.check(lib.ttup_uplift_val_metrics(p(rot), p(pos), p(r_world), p(rotation), p(mask), n, t, 1, p(ws), nbytes, p(sums), p(counts), st))
    best, mean = event_timed(launch_val, a.repeat, a.inner)
    traffic = 2 * n * t * 12
    res.update({'val_metrics_us_best': best * 1e6, 'val_metrics_us_mean': mean * 1e6, 'val_metrics_traffic_bytes': traffic,
                'val_metrics_gb_per_s_best': traffic / best * 1e-9, 'val_metrics_gb_per_s_mean': traffic / mean * 1e-9})

    mint = f(np.tile(np.array([[2500.0, 0, 1280], [0, 2500, 720], [0, 0, 1]]), (n, 1, 1)))
    mext = f(np.tile(np.array([[1.0, 0, 0, 0], [0, 0, -1, 1], [0, 1, 0, 8], [0, 0, 0, 1]]), (n, 1, 1)))
    cls = torch.from_numpy((np.arange(n) % 3).astype(np.int32)).cuda()
    scores, labels = torch.empty((n,), dtype=torch.float64, device='cuda'), torch.empty((n,), dtype=torch.int32, device='cuda')

    def launch_real():
        _lib.check(lib.ttup_uplift_val_real_metrics(p(rot), p(pos), p(r_img), p(mask), p(mint), p(mext), p(cls), n, t, 1, p(ws), nbytes, p(sums), p(counts),
                                                    p(scores), p(labels), st))
    best, mean = event_timed(launch_real, a.repeat, a.inner)
    res.update({'val_real_metrics_us_best': best * 1e6, 'val_real_metrics_us_mean': mean * 1e6})
    print(json.dumps(res))


if __name__ == '__main__':
    main()
