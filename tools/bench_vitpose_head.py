#!/usr/bin/env python3
"""The ViTPose head's training pass at batch 8, 640x1152 (a 40x72 token grid) on one GPU -> one JSON line.

ms per call (device events around `--steps` calls after `--warmup`, best of two rounds, forward and backward alternating) of the
training-mode forward (pack, two deconvolutions, batch-statistics BN, 1x1 conv), of the backward, and of the eval-mode forward; the
inference head on the same batch for comparison (`ViTPoseNet.run_stage(13)`: last_norm, the BN-folded deconvolutions + ReLU, the 1x1
conv); achieved TFLOP/s of the matrix products against the fp32-operand MFMA peak; the handle's workspace.  Seeded weights and inputs.

    python tools/bench_vitpose_head.py [--batch 8] [--steps 20] [--warmup 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 640, 1152
HP, WP = H // 16, W // 16
FP32_MFMA_PEAK = 157.3      # TFLOP/s, v_mfma_f32_16x16x4_f32 (tools/bench_vitpose.py)


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch
    from upliftingtabletennis_amd import vitpose, vitpose_head, weights
    b, tokens = a.batch, a.batch * HP * WP
    sd = weights.random_vitpose_state_dict(0)
    net = vitpose.ViTPoseNet(sd, max_batch=b, micro_batch=b)
    head = vitpose_head.ViTPoseHead(sd, 1, max_rows=tokens)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal((tokens, 384)).astype(np.float32)).cuda()          # a residual stream; last_norm makes the features of it
    net.run_stage(13, x)
    feat = net.read_tap('ln')
    dheat = torch.from_numpy((rng.standard_normal((b, 1, 4 * HP, 4 * WP)) / (16 * tokens)).astype(np.float32)).cuda()
    best = {}
    for _ in range(2):
        for name, fn in (('forward_train', lambda: head.forward(feat, (HP, WP), train=True)), ('backward', lambda: head.backward(dheat)),
                         ('forward_eval', lambda: head.forward(feat, (HP, WP), train=False)), ('inference_head', lambda: net.run_stage(13, x))):
            best[name] = min(best.get(name, float('inf')), timed(fn, a.steps, a.warmup))
        head.forward(feat, (HP, WP), train=True)          # the backward of the next round goes through batch statistics again
    gflop_fwd = b * (2 * 4 * HP * WP * 256 * 4 * 384 + 2 * 16 * HP * WP * 256 * 4 * 256) / 1e9          # the two deconvolutions; the backward has two products of that size each
    res = {'metric': 'vitpose_head_train_640x1152', 'batch': b, 'tokens': tokens, 'steps': a.steps,
           'ms': {k: round(v, 3) for k, v in best.items()},
           'gflop': {'forward': round(gflop_fwd, 1), 'backward': round(2 * gflop_fwd, 1)},
           'tflops': {'forward_train': round(gflop_fwd / best['forward_train'], 1), 'backward': round(2 * gflop_fwd / best['backward'], 1),
                      'inference_head': round(gflop_fwd / best['inference_head'], 1)},
           'pct_of_fp32_mfma_peak': {'forward_train': round(100 * gflop_fwd / best['forward_train'] / FP32_MFMA_PEAK, 1),
                                     'backward': round(100 * 2 * gflop_fwd / best['backward'] / FP32_MFMA_PEAK, 1)},
           'workspace_mb': round(head.workspace_bytes() / 2 ** 20, 1)}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
