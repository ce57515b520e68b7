#!/usr/bin/env python3
"""ViTPose-small detector throughput at 640x1152 on one GPU -> one JSON line.

frames/s of the whole forward (argmax windows, no heatmap and no host copies) at batch 8 and 32 (micro-batch 8), achieved TFLOP/s
against the measured bf16 MFMA peak (ttup_peak_mfma_bf16) and the fp32-operand MFMA peak the kernels run on (157.3 TFLOP/s, 1/16
of the bf16 rate; every product counted once: there are no split-bf16 terms), and ms per kernel family from a rocprofv3 kernel trace
of a child process (--no-prof skips it).  --dtype f32 (the default) | bf16 picks the path and keeps the line's layout (`batch8`, `batch32`,
`ms_per_frame_by_family` at the top level, plus `dtype`); --dtype both measures the two alternating in one process (f32, bf16, f32, bf16
at each batch size; the best of the two rounds each), puts each dtype's figures under its name, reports `bf16_over_f32` and traces one
child run per dtype.

    python tools/bench_vitpose.py [--dtype f32|bf16|both] [--steps 20] [--warmup 3] [--no-prof]
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, N = 640, 1152, (640 // 16) * (1152 // 16)
# per frame: linears 2*N*(384*1152 + 384*384 + 2*384*1536)*12; attention 2 * 2*N*N*384 * 12; deconvs; patch embed; final 1x1
GFLOP = {'linear': 2 * N * (384 * 1152 + 384 * 384 + 2 * 384 * 1536) * 12 / 1e9,
         'attention': 4 * N * N * 384 * 12 / 1e9,
         'deconv': (2 * 4 * N * 256 * 4 * 384 + 2 * 16 * N * 256 * 4 * 256) / 1e9,
         'patch_embed': 2 * N * 384 * 9 * 256 / 1e9,
         'conv1x1': 2 * 16 * N * 256 / 1e9}
FP32_MFMA_PEAK = 157.3      # TFLOP/s, v_mfma_f32_16x16x4_f32 (1/16 of the bf16 MFMA rate); 155 measured with register-resident loops
FAMILIES = [('attention', 'attention_'), ('patch_embed', 'gemm_kernel<2,'), ('patch_embed', 'gemm_bf16_kernel<2>'),
            ('deconv', 'gemm_kernel<3,'), ('deconv', 'gemm_bf16_kernel<3>'), ('linear', 'gemm_kernel<'), ('linear', 'gemm_bf16_kernel<'),
            ('layernorm', 'ln_'), ('conv1x1', 'conv1x1_'), ('argmax', 'argmax_')]


def run(batch, steps, warmup, dtype='f32'):
    import torch
    from upliftingtabletennis_amd import synth, vitpose, weights
    sd = weights.random_vitpose_state_dict(0)
    net = vitpose.ViTPoseNet(sd, max_batch=batch, dtype=dtype)
    x = torch.from_numpy(synth.vitpose_inputs(0, batch, 9, H, W)[0]).cuda()
    for _ in range(warmup):
        net.forward(x, want_heatmap=False, want_peaks=True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        net.forward(x, want_heatmap=False, want_peaks=True)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def families(stats_csv):
    out = {}
    with open(stats_csv) as f:
        for r in csv.DictReader(f):
            name, ms = r['Name'], float(r['TotalDurationNs']) / 1e6
            fam = next((k for k, pat in FAMILIES if pat in name), 'other')
            out[fam] = out.get(fam, 0.0) + ms
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dtype', choices=('f32', 'bf16', 'both'), default='f32')
    ap.add_argument('--no-prof', action='store_true')
    ap.add_argument('--child', type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        run(a.child, a.steps, a.warmup, 'f32' if a.dtype == 'both' else a.dtype)
        return
    import torch  # noqa: F401
    from upliftingtabletennis_amd import _lib
    lib = _lib.load()
    res = {'metric': 'vitpose_small_640x1152', 'gflop_per_frame': round(sum(GFLOP.values()), 1),
           'gflop_per_frame_by_family': {k: round(v, 1) for k, v in GFLOP.items()}}
    peak = (ctypes.c_double * 4)()
    _lib.check(lib.ttup_peak_mfma_bf16(2000, 2, peak, _lib.stream_ptr()))
    res['peak_bf16_tflops'] = round(peak[0], 1)
    res['peak_fp32_mfma_tflops_spec'] = FP32_MFMA_PEAK
    dtypes = ('f32', 'bf16') if a.dtype == 'both' else (a.dtype,)
    for d in dtypes:
        res[d] = {}
    for b in (8, 32):
        best = {}
        for _ in range(2 if len(dtypes) > 1 else 1):          # alternating: both dtypes see the same clocks and neighbours
            for d in dtypes:
                best[d] = min(best.get(d, float('inf')), run(b, a.steps, a.warmup, d))
        for d in dtypes:
            fps = b / best[d] * 1e3
            tf = fps * res['gflop_per_frame'] / 1e3
            res[d]['batch%d' % b] = {'ms_per_batch': round(best[d], 3), 'frames_per_s': round(fps, 1), 'tflops': round(tf, 1),
                                     'pct_of_bf16_peak': round(100 * tf / peak[0], 2), 'pct_of_fp32_mfma_peak': round(100 * tf / FP32_MFMA_PEAK, 1)}
        if len(dtypes) > 1:
            res.setdefault('bf16_over_f32', {})['batch%d' % b] = round(best['f32'] / best['bf16'], 2)
    res['flop_count_note'] = 'every product is counted once on either path (no split-bf16 terms exist to count)'
    if not a.no_prof:
        for d in dtypes:
            with tempfile.TemporaryDirectory() as td:
                cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', td, '-o', 'vp', '--output-format', 'csv', '--',
                       sys.executable, os.path.abspath(__file__), '--child', '8', '--steps', '5', '--warmup', '0', '--dtype', d]
                subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
                stats = glob.glob(os.path.join(td, '**', '*kernel_stats.csv'), recursive=True)
                if stats:
                    fam = families(stats[0])
                    tot = sum(fam.values())
                    res[d]['ms_per_frame_by_family'] = {k: round(v / 40, 4) for k, v in sorted(fam.items(), key=lambda kv: -kv[1])}
                    res[d]['attention_share'] = round(fam.get('attention', 0.0) / tot, 3)
    if len(dtypes) == 1:          # one dtype: the line as it always was
        res.update(res.pop(dtypes[0]))
        res['dtype'] = dtypes[0]
    print(json.dumps(res))


if __name__ == '__main__':
    main()
