#!/usr/bin/env python3
"""Throughput of the uplift training loss + gradients (uplift.MultiStageModel.loss_and_grad, size `large`) beside the forward-only
rate of the same handle at the same shapes in the same process.

Per batch size (default 64 = the reference's BATCH_SIZE, 1 024, 10 000; T = 50 with 7 padded slots): samples/s of
loss_and_grad -- best and median of --repeat timed calls after a warm-up call of the same shape, host clock around a device
synchronise, the workspace and output allocations inside the timed call as a training step would pay them -- the forward-only
rate measured the same way, their ratio and the workspace bytes.  Prints one JSON line.

    python tools/bench_uplift_grad.py [--batches 64,1024,10000] [--len 50] [--repeat 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from upliftingtabletennis_amd import synth, uplift, weights  # noqa: E402


def inputs(b, length, pad=7):
    n = min(b, 1024)
    base = list(synth.ragged_uplift_batch(n, length - pad, seed=0, pad=pad)) + list(synth.uplift_targets(n, length, 0))
    base = [torch.from_numpy(a).cuda() for a in base]
    rep = (b + n - 1) // n
    return [a.repeat((rep,) + (1,) * (a.dim() - 1))[:b].contiguous() for a in base]


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='64,1024,10000')
    ap.add_argument('--len', type=int, default=50)
    ap.add_argument('--repeat', type=int, default=5)
    a = ap.parse_args()
    sd = weights.random_uplift_state_dict(0, 'large')
    rows = []
    for b in [int(v) for v in a.batches.split(',')]:
        data = inputs(b, a.len)
        net = uplift.MultiStageModel(sd, size='large', max_batch=b, max_len=a.len)
        ws = int(net._lib.ttup_uplift_grad_workspace_bytes(net._handle, b, a.len))
        tg = timed(lambda: net.loss_and_grad(*data, check_mask=False), a.repeat)
        tf = timed(lambda: net.forward(*data[:4], check_mask=False), a.repeat)
        rows.append({'batch': b, 'len': a.len, 'workspace_bytes': ws,
                     'grad_samples_per_s_best': b / min(tg), 'grad_samples_per_s_median': b / statistics.median(tg),
                     'forward_samples_per_s_best': b / min(tf), 'forward_samples_per_s_median': b / statistics.median(tf),
                     'grad_over_forward_time': statistics.median(tg) / statistics.median(tf)})
        del net
        torch.cuda.empty_cache()
    print(json.dumps({'tool': 'bench_uplift_grad', 'size': 'large', 'device': torch.cuda.get_device_name(0), 'repeat': a.repeat, 'rows': rows}))


if __name__ == '__main__':
    main()
