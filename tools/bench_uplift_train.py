#!/usr/bin/env python3
"""Throughput of the uplift training step (uplift.UpliftTrainer.step, size `large`, check_mask=False: no host synchronisation inside)
beside loss_and_grad alone on the same trainer's handle, same shapes, same process; the optimizer's share is the difference.

Per batch size (default 64 = the reference's BATCH_SIZE, and 1 024; T = 50 with 7 padded slots): steps/s and samples/s -- median and
best of --repeat windows of --steps calls each after a warm-up window, host clock around a device synchronise, the two variants
alternating --, and the optimizer step on its own (ttup_uplift_opt_step on a fixed gradient buffer: norm partials, norm, fused
pass -- three launches): --repeat windows of --opt-calls calls, each between two device events, median and spread of the time per
call, and the bytes per second it reaches, counting what the
algorithm must move -- 4 bytes per gradient entry for the norm, 36 per parameter for the fused pass (reads g, p, m, v, ema; writes p,
m, v, ema).  That rate is of the three launches together, launch gaps included, so it is a lower bound of the fused pass's own; the
9 buffers of `large` (74 MB) fit the Infinity Cache.  Prints one JSON line.

    python tools/bench_uplift_train.py [--batches 64,1024] [--len 50] [--steps 20] [--repeat 5] [--size large] [--opt-calls 10000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_uplift_grad import inputs  # noqa: E402
from upliftingtabletennis_amd import _lib, arch, uplift, weights  # noqa: E402


def window(fn, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='64,1024')
    ap.add_argument('--len', type=int, default=50)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--size', default='large')
    ap.add_argument('--opt-calls', type=int, default=10000)
    a = ap.parse_args()
    sd = weights.random_uplift_state_dict(0, a.size)
    n_layout = arch.uplift_grad_layout(a.size)[1]
    n_param = n_layout - arch.uplift_grad_hole(a.size)[1]
    step_bytes = 4 * n_layout + 36 * n_param
    rows = []
    for b in [int(v) for v in a.batches.split(',')]:
        data = inputs(b, a.len)
        tr = uplift.UpliftTrainer(sd, size=a.size, max_batch=b, max_len=a.len)
        step = lambda: tr.step(*data, check_mask=False)                              # noqa: E731
        grad = lambda: tr._model.loss_and_grad(*data, check_mask=False)              # noqa: E731
        window(step, 2), window(grad, 2)
        ts, tg = [], []
        for _ in range(a.repeat):
            ts.append(window(step, a.steps))
            tg.append(window(grad, a.steps))
        # the optimizer step alone, on the last gradient buffer, between device events
        flat = grad()[2].flat
        norm = torch.empty(1, device='cuda')
        opt = lambda: _lib.check(tr._lib.ttup_uplift_opt_step(tr._opt, _lib.ptr(flat), _lib.ptr(norm), _lib.stream_ptr()))      # noqa: E731
        for _ in range(50):
            opt()
        t_opts = []
        for _ in range(a.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.opt_calls):
                opt()
            e1.record()
            torch.cuda.synchronize()
            t_opts.append(e0.elapsed_time(e1) * 1e-3 / a.opt_calls)
        t_opt = statistics.median(t_opts)
        ms, mg = statistics.median(ts), statistics.median(tg)
        rows.append({'batch': b, 'len': a.len, 'steps_per_s_median': 1 / ms, 'steps_per_s_best': 1 / min(ts), 'samples_per_s_median': b / ms,
                     'loss_and_grad_per_s_median': 1 / mg, 'loss_and_grad_samples_per_s_median': b / mg,
                     'optimizer_share_of_step': (ms - mg) / ms, 'step_ms': ms * 1e3, 'loss_and_grad_ms': mg * 1e3,
                     'opt_step_alone_us': t_opt * 1e6, 'opt_step_alone_us_min_max': [min(t_opts) * 1e6, max(t_opts) * 1e6], 'opt_step_alone_bytes': step_bytes, 'opt_step_alone_TB_per_s': step_bytes / t_opt / 1e12})
        del tr
        torch.cuda.empty_cache()
    print(json.dumps({'tool': 'bench_uplift_train', 'size': a.size, 'parameters': n_param, 'device': torch.cuda.get_device_name(0), 'steps': a.steps,
                      'repeat': a.repeat, 'rows': rows}))


if __name__ == '__main__':
    main()
