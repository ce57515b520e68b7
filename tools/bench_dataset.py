#!/usr/bin/env python3
"""Throughput of building uplift training samples on the device (upliftingtabletennis_amd/dataset.py), one JSON line:
samples/s for N train-mode samples (full transform pipeline) and N 'test'-mode samples from a device-resident TrajectoryBatch,
and the chain generator -> samples -> uplift forward at T = 50 with the time of each stage.

Every timed call is preceded by a warm-up call of the same shape and ends in a device synchronise; best and mean of --repeat.

    python tools/bench_dataset.py [--samples 100000] [--trajectories 20000] [--chain 10000] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from upliftingtabletennis_amd import _lib, dataset, trajgen, uplift, weights  # noqa: E402

CONFIG = types.SimpleNamespace(blur_strength=0.4, randomize_std=8, stop_prob=0.5, randdet_prob=0.05, randmiss_prob=0.05, tablemiss_prob=0.05)


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), sum(ts) / len(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=100000)
    ap.add_argument('--trajectories', type=int, default=20000)
    ap.add_argument('--chain', type=int, default=10000)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--mode', default='final_lose')
    a = ap.parse_args()
    gen = lambda n: trajgen.get_valid_trajectories(n, 128, a.mode, 'left_to_right', batches_per_launch=128, as_numpy=False)      # noqa: E731
    tr = gen(a.trajectories)
    idx = np.arange(a.samples) % len(tr)
    seeds = np.arange(a.samples)
    res = {'samples': a.samples, 'trajectories': len(tr), 'build_id': _lib.build_id()}
    for mode in ('train', 'test'):
        ds = dataset.TableTennisDataset(mode, dataset.get_transforms(CONFIG, mode), trajectories=tr)
        best, mean, b = timed(lambda: ds.batch(idx, seeds), a.repeat)
        res[mode + '_samples_per_s_best'], res[mode + '_samples_per_s_mean'] = a.samples / best, a.samples / mean
        if mode == 'train':
            res['train_mean_camera_tries'] = float(b.camera_tries.double().mean())
            res['train_mean_frames'] = float(b.mask.sum(1).mean())
    # chain at T = 50: generator -> samples -> uplift forward, each stage timed alone and the three together
    n = a.chain
    net = uplift.get_model('connectstage', 'large', 'dynamic', 'new', state_dict=weights.random_uplift_state_dict(0, 'large'), max_batch=n, max_len=50)
    tf = dataset.get_transforms(CONFIG, 'train')
    t_gen, _, tr_n = timed(lambda: gen(n), a.repeat)
    ds = dataset.TableTennisDataset('train', tf, trajectories=tr_n)
    t_smp, _, sb = timed(lambda: ds.batch(np.arange(n)), a.repeat)
    t_fwd, _, _ = timed(lambda: net(*sb.model_inputs()), a.repeat)

    def chain():
        d = dataset.TableTennisDataset('train', tf, trajectories=gen(n))
        return net(*d.batch(np.arange(n)).model_inputs())
    t_all, _, _ = timed(chain, a.repeat)
    res.update({'chain_n': n, 'chain_generator_per_s': n / t_gen, 'chain_samples_per_s': n / t_smp, 'chain_forward_per_s': n / t_fwd,
                'chain_end_to_end_per_s': n / t_all, 'chain_slowest_stage': min((n / t_gen, 'generator'), (n / t_smp, 'samples'), (n / t_fwd, 'forward'))[1]})
    print(json.dumps(res))


if __name__ == '__main__':
    main()
