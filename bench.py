#!/usr/bin/env python3
"""Headline benchmark: frames/s end-to-end (detect + refine + uplift) on synthetic 1280x720 video.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full [--ops-json FILE]]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A step = one pass of the hot path over one stream batch that is already resident in HBM:
  258 uint8 frames (1280x720x3)  -> 256 triples -> fused pre-processing (cv2-style resize to 1280x704 +
  normalise) -> WASB/HRNet CNN (bf16 MFMA) -> heatmap argmax + 3x3 window -> L-BFGS-B Gaussian refine
  (table variant, as on the hub surface) -> two-detector filter + uplift transform on the host (as in the
  reference) -> uplift transformer on the clip cut into 120-step trajectories (120 + 120 + 16 detections, padded to
  121 tokens: north_star's "120-step trajectories") -> spin frame change.
`--gpus N` without a torch.distributed environment starts the N ranks itself (a `torch.distributed.run` child process,
before this process touches the GPU) and relays rank 0's line; under `torch.distributed.run` it is one of the ranks.
Every rank processes its own stream (independent units); the only collective is the final gather of
the per-frame (x,y,v) records and the per-trajectory (spin, positions) records.

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run does what the headline needs and nothing else:
set-up, W warm-up steps, the K timed steps, the --dump-outputs records and the line.  `--full` adds the rest to the same line:
`cpu_baseline` (the CPU oracle timed on a bounded sample, run before this process touches the GPU), `roofline` (the CNN graph,
HIP-event timed inside this process in graph order, with the heatmap rooflines and the device's measured peaks), at N=1 the
other legs (`e2e_from_host_fps`, the weight / content / parity regimes and the driver-timed extras for BASELINE configs 1, 2, 3
and 5: `cnn_only_fps`, `uplift_only_traj_s`, `trajgen_traj_s`, ...) and at N>1 every rank's stream -> hardware-queue grouping
(`stream_queue_groups`).  --no-cpu-baseline / --no-roofline / --no-extras leave a part of --full out.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

H_SRC, W_SRC = 720, 1280
W_NET, H_NET = 1280, 704
TRIPLES = int(os.environ.get('TTUP_BENCH_TRIPLES', '256'))
TRAJ_LEN = 120                 # detections per trajectory (north_star: 120-step trajectories)
SEQ_LEN = TRAJ_LEN + 1          # tokens: the uplift net needs at least one padded slot (uplifting/model.py:541-546)
PEAK_BF16_TFLOPS = 2500.0      # dense bf16 MFMA, MI355X_MICROARCH.md (vendor); the measured peak of the device is reported beside it
PEAK_HBM_GBS = 8000.0
DELTA_REF = 4e-6                # 2 x the measured |HIP fp32 heatmap - reference heatmap| on the near-tie fixture (bench weights: 1.1e-6 with the fp32-MFMA kernels,
                                # re-measured for the split-bf16 kernels by test_certified_argmax_matches_the_reference_on_near_ties), rounded up
GFLOP_PER_FRAME_EXECUTED = 331.3   # 344.07 minus the elided stage-4 fuse outputs 1..3


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=20)          # (the driver's own flags: --steps 20 --warmup 5)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--full', action='store_true', help='also run the CPU baseline, the roofline, the other legs (N=1) and the queue probes (N>1)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline')
    ap.add_argument('--no-roofline', action='store_true', help='with --full: skip the roofline')
    ap.add_argument('--no-certify', action='store_true', help='plain bf16 argmax (no fp32 re-evaluation of near-ties)')
    ap.add_argument('--no-extras', action='store_true', help='with --full: skip the other legs (from-host, regimes, configs 1/2/3/5)')
    ap.add_argument('--dump-outputs', metavar='DIR', help='write the records of the last timed step (all ranks, rank order) as DIR/<key>.npy')
    ap.add_argument('--ops-json', metavar='FILE', help='with --full: write the per-op timings behind `roofline` to FILE (nothing is written into the source tree)')
    a = ap.parse_args()
    if a.steps < 1:
        ap.error('--steps must be at least 1')
    if a.ops_json and not a.full:
        ap.error('--ops-json writes the roofline\'s per-op timings: it needs --full')
    if not a.full:          # a plain run: set-up, warm-up, timed steps, --dump-outputs and the line, nothing else
        a.no_cpu_baseline = a.no_roofline = a.no_extras = True
    return a


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(gathered, out_dir):
    """The records the timed path handed to its caller in its last step ({key: [tensor of rank 0, rank 1, ...]}), one DIR/<key>.npy
    per key with the ranks' rows concatenated: float32 stays float32, everything else (xyv float64, n_valid int64) becomes float64.
    The inputs are seeded (weights seed 0, clip seed = rank), so two builds run with the same flags can be compared file for file."""
    arrays = {}
    for k, per_rank in gathered.items():
        a = np.concatenate([t.detach().cpu().numpy() for t in per_rank])
        arrays[k] = a.astype(np.float32 if a.dtype == np.float32 else np.float64)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit('bench.py: --dump-outputs would write %d bytes (limit %d)' % (total, DUMP_LIMIT_BYTES))
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + '.npy'), a)


class Pipeline:
    """Per-rank worker (upliftingtabletennis_amd.pipeline.StreamWorker) plus its resident synthetic clip."""

    def __init__(self, device, seed, certify=True, planted=True, exact_windows=False):
        from upliftingtabletennis_amd import pipeline, synth, weights
        self.worker = pipeline.StreamWorker(device, weights.random_wasb_state_dict(0, planted=planted), weights.random_uplift_state_dict(0, 'large'),
                                            net_wh=(W_NET, H_NET), max_triples=TRIPLES, traj_len=TRAJ_LEN, seq_len=SEQ_LEN, certify=certify,
                                            audit_every=int(os.environ.get('TTUP_AUDIT_EVERY', '256')), exact_windows=exact_windows)
        self.net = self.worker.net
        # synthetic clip: 34 distinct frames tiled to TRIPLES+2 (keeps generation time low; content still varies per frame)
        base, track = synth.synth_frames(34, H_SRC, W_SRC, seed=seed)
        reps = (TRIPLES + 2 + len(base) - 1) // len(base)
        clip = np.concatenate([base] * reps)[:TRIPLES + 2]
        self.frames = torch.from_numpy(clip).to(device)
        _, table, _, _ = synth.synth_trajectories(1, 4, seed=seed)
        self.table_px = np.array(table[0], dtype=np.float64)
        self.table_px[:, 0] *= 1920
        self.table_px[:, 1] *= 1080
        self.fps = 60.0

    def step(self):
        return self.worker.process_clip(self.frames, self.table_px, self.fps)

    def submit(self):
        return self.worker.submit(self.frames)

    def collect(self, ticket):
        return self.worker.collect(ticket, self.table_px, self.fps)


TRAFFIC_FILE = 'r6_traffic.json'      # profiles/: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this round (tools/pmc_traffic.py)


def _family(kernel):
    """Kernel family of an op's device kernel ("c16_chain_kernel<24, 32, 7>+sum+head" -> "c16_chain_kernel"): the epilogue variants of
    the 16-channel chain are one kernel compiled three ways; every other kernel is its own family (template arguments kept)."""
    exact = kernel.split('+')[0]
    base = exact.split('<')[0]
    return base if base in ('c16_chain_kernel', 'bb_chain2_kernel') else exact


_TRAFFIC_CACHE = None


def _traffic(kernel_exact):
    """HBM bytes per launch of ONE device kernel (template arguments included, as rocprofv3 prints them) from the committed PMC passes
    (FETCH_SIZE x2 on gfx950 + WRITE_SIZE, separate runs; MI355X_MICROARCH.md, HBM).  None when the profile does not hold that kernel --
    round 5 matched by substring and silently dropped every launch whose op label differed from the kernel's name."""
    global _TRAFFIC_CACHE
    if _TRAFFIC_CACHE is None:
        try:
            _TRAFFIC_CACHE = json.load(open(os.path.join(ROOT, 'profiles', TRAFFIC_FILE)))
        except Exception:
            _TRAFFIC_CACHE = []
    want = kernel_exact.split('+')[0].replace(' ', '')
    hits = []
    for e in _TRAFFIC_CACHE:
        name = e['kernel'].replace('void ', '').replace('ttup::', '').replace('(anonymous namespace)::', '')
        name = name.split('(')[0].replace(' ', '')
        if name == want:
            hits.append(e)
    if hits:
        return int(sum(e['hbm_bytes'] * e['launches'] for e in hits) / sum(e['launches'] for e in hits))
    return None


def roofline(pipe):
    """HIP-event timing of the CNN graph inside the library, in launch order (one micro-batch, the stream the kernels
    run on).  Ops are grouped by the kernel they launch.  `achieved` / `frac` = the algorithmic FLOP of ALL launches of a
    micro-batch / their summed durations; `longest_kernel` (largest total time) and `lowest_kernel` (least efficient among
    the kernels holding >= 5 % of the time) carry their own algorithmic FLOP per launch / average launch duration."""
    from upliftingtabletennis_amd import wasb
    ops = wasb.time_ops(pipe.net, reps=5, in_graph=True)
    groups = {}
    missing = []          # ops whose device kernel the traffic profile does not hold
    for o in ops:
        # group by kernel family; HBM traffic is looked up per op by the exact device kernel it launched
        name = _family(o['kernel'])
        g = groups.setdefault(name, {'kernel': name, 'launches': 0, 'ms': 0.0, 'flops': 0.0, 'shape': (o['h'], o['w']), 'traffic': 0, 'traffic_ok': True})
        g['launches'] += 1; g['ms'] += o['ms']; g['flops'] += o['flops']
        t = _traffic(o['kernel'])
        if t is None:
            g['traffic_ok'] = False
            missing.append(o['kernel'].split('+')[0])
        else:
            g['traffic'] += t
    table = sorted(groups.values(), key=lambda g: -g['ms'])
    tot_ms = sum(o['ms'] for o in ops)
    tot_fl = sum(o['flops'] for o in ops)
    mb = ops[0]['batch']

    def entry(g):
        tf = g['flops'] / (g['ms'] * 1e-3) / 1e12
        return {'kernel': '%s @%dx%d' % (g['kernel'], g['shape'][0], g['shape'][1]), 'launches': g['launches'], 'ms': round(g['ms'], 4),
                'launch_ms': round(g['ms'] / g['launches'], 4), 'algorithmic_gflop_per_launch': round(g['flops'] / g['launches'] / 1e9, 2),
                'achieved': round(tf, 2), 'frac': round(tf / PEAK_BF16_TFLOPS, 4),
                'traffic': int(g['traffic'] / g['launches']) if g['traffic_ok'] else None}
    mfma = [g for g in table if g['flops'] > 0]          # the element-wise sums are HBM-bound: no FLOP figure
    longest = mfma[0]                                   # largest TOTAL time per micro-batch
    # lowest fraction among the kernels that matter (>= 5 % of the micro-batch): the small stride-2 / 1x1 convs are HBM- or latency-bound
    heavy = [g for g in mfma if g['ms'] >= 0.05 * tot_ms]
    lowest = min(heavy, key=lambda g: g['flops'] / g['ms'])
    # whole graph: passes launched back to back between ONE pair of events (an event record between two kernels is a queue packet of
    # its own: the per-op intervals above each carry one, and their sum overstates what a lane spends on a micro-batch)
    replay_ms = wasb.time_replay(pipe.net, reps=10)
    all_tf = tot_fl / (replay_ms * 1e-3) / 1e12
    ev_tf = tot_fl / (tot_ms * 1e-3) / 1e12
    # HBM bytes of the whole micro-batch from the committed PMC passes (every kernel's bytes per launch x its launches in the graph)
    # (None -- not a partial sum -- when the profile lacks any kernel the graph launches: `traffic_missing` lists them)
    traffic_all = int(sum(g['traffic'] for g in table)) if not missing else None
    # Headline fraction = ALL CNN kernels of one micro-batch (two kernels tie for "dominant" within 1 %, so a
    # dominant-kernel headline flips between 0.21 and 0.31 from box to box; the whole graph's fraction does not).  The dominant
    # kernel by total time and the least efficient heavy kernel are listed beside it, each with its own launch duration.
    r = {'bound': 'mfma', 'achieved': round(all_tf, 2), 'peak': PEAK_BF16_TFLOPS, 'unit': 'TFLOP/s',
         'frac': round(all_tf / PEAK_BF16_TFLOPS, 4), 'traffic': traffic_all,
         'kernel': 'all %d kernel launches of the CNN graph for one micro-batch of %d frames (%.3f ms): %.1f GFLOP executed per frame'
                   % (len(ops), mb, replay_ms, tot_fl / mb / 1e9),
         'scope': 'cnn_all_ops', 'ms_per_microbatch': round(replay_ms, 3), 'ms_per_microbatch_op_events': round(tot_ms, 3), 'micro_batch': mb,
         'algorithmic_gflop_per_microbatch': round(tot_fl / 1e9, 2),
         'longest_kernel': entry(longest), 'lowest_kernel': entry(lowest),
         'timing': 'whole graph (achieved, frac, ms_per_microbatch): 10 passes launched back to back on one stream between ONE pair of HIP events '
                   '(ttup_wasb_time_replay); per kernel (longest_kernel, lowest_kernel, per_kernel) and ms_per_microbatch_op_events: hipEvent between '
                   'consecutive ops in launch order (ttup_wasb_time_graph), 5 passes -- every interval carries one event record',
         'per_kernel': [{'kernel': g['kernel'], 'launches': g['launches'], 'ms': round(g['ms'], 4),
                         'tflops': round(g['flops'] / (g['ms'] * 1e-3) / 1e12, 1) if g['flops'] else None} for g in table],
         'cnn_all_ops': {'ms_per_microbatch': round(replay_ms, 3), 'tflops': round(all_tf, 2), 'frac': round(all_tf / PEAK_BF16_TFLOPS, 4),
                         'op_events': {'ms_per_microbatch': round(tot_ms, 3), 'tflops': round(ev_tf, 2), 'frac': round(ev_tf / PEAK_BF16_TFLOPS, 4)}}}
    if missing:
        r['traffic_missing'] = sorted(set(missing))
    if r['traffic'] is not None:
        r['traffic_note'] = 'bytes per micro-batch / per launch from profiles/%s (rocprofv3 FETCH_SIZE*2 + WRITE_SIZE, separate passes)' % TRAFFIC_FILE
    return r, ops


def heatmap_roofline(device, eps_abs):
    """HBM roofline of the kernels that stream fp32 heatmaps, on 256 heatmaps resident in HBM (923 MB: well past the 256 MiB
    Infinity Cache), HIP events on the launch stream.
      production : cert_scan_kernel (csrc/certify.hip) -- the pass over the heatmap on the timed path: candidates within 2*eps of
                   the maximum that the stage-4 epilogue found (in the pipeline it runs right behind that epilogue, per micro-batch);
      seam       : argmax_partial_kernel + argmax_finish_kernel -- the standalone extract_position_* seam (ttup_refine)."""
    from upliftingtabletennis_amd import refine, _lib
    n = 256
    heat = torch.randn((n, H_NET, W_NET), device=device)
    refine.refine_device(heat, 1920, 1080, _lib.REFINE_BALL)
    torch.cuda.synchronize()
    lib = _lib.load()
    ws_bytes = lib.ttup_refine_workspace_bytes(n, H_NET, W_NET)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
    idx = torch.empty((n,), dtype=torch.int64, device=device)
    win = torch.empty((n, 9), dtype=torch.float32, device=device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 20
    nbytes = n * H_NET * W_NET * 4

    def timed(fn):
        fn()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps
    ms = timed(lambda: _lib.check(lib.ttup_refine(_lib.ptr(heat), n, H_NET, W_NET, 1920, 1080, 0, None, _lib.ptr(idx), _lib.ptr(win), _lib.ptr(ws), ws_bytes, _lib.stream_ptr())))
    gbs = nbytes / (ms * 1e-3) / 1e9
    seam = {'bound': 'hbm', 'achieved': round(gbs, 1), 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'frac': round(gbs / PEAK_HBM_GBS, 4),
            'traffic': _traffic('argmax_partial_kernel<true>'), 'kernel': 'argmax_partial_kernel + argmax_finish_kernel (the extract_position_* seam; not on the timed path)',
            'launch_ms': round(ms, 4), 'heatmaps': n, 'algorithmic_bytes_per_launch': nbytes}
    K = 32
    cidx = torch.empty((n, K), dtype=torch.int32, device=device)
    cbf = torch.empty((n, K), dtype=torch.float32, device=device)
    ccnt = torch.zeros((n,), dtype=torch.int32, device=device)

    def scan():          # counters zeroed in stream order before every launch, as cert_begin does on the production path (a launch that
        ccnt.zero_()     # starts from accumulated counts skips the candidate stores: round-3 advisor)
        _lib.check(lib.ttup_certify_scan(_lib.ptr(heat), _lib.ptr(idx), n, H_NET, W_NET, float(eps_abs), K, _lib.ptr(cidx), _lib.ptr(ccnt), _lib.ptr(cbf), _lib.stream_ptr()))
    ms_zero = timed(lambda: ccnt.zero_())
    ms = timed(scan) - ms_zero
    gbs = nbytes / (ms * 1e-3) / 1e9
    prod = {'bound': 'hbm', 'achieved': round(gbs, 1), 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'frac': round(gbs / PEAK_HBM_GBS, 4),
            'traffic': _traffic('cert_scan_kernel'), 'kernel': 'cert_scan_kernel (certified argmax, step 1): the heatmap pass of the timed path, here on 256 HBM-resident heatmaps',
            'launch_ms': round(ms, 4), 'heatmaps': n, 'algorithmic_bytes_per_launch': nbytes, 'eps_abs': round(float(eps_abs), 6)}
    return prod, seam


def _cpu_child(style, n, threads):
    """One CPU-oracle timing in a FRESH process (`python bench.py --cpu-child style n threads`): no GPU is touched, the OpenMP pool is this
    process's own (OMP_NUM_THREADS / OMP_PROC_BIND / OMP_PLACES come from the caller's environment).  One FULL-SIZE warm-up triple first
    (oneDNN creates its convolution primitives per shape: a 64-row strip warms nothing that the full frame uses), then n timed triples.
    Prints one JSON line {seconds, triples, threads, per_triple, parts, torch, mkldnn, omp}."""
    torch.set_num_threads(threads)
    from oracle import glue_ref, refine_ref, uplift_ref, wasb_ref
    from upliftingtabletennis_amd import synth, weights
    frames, _ = synth.synth_frames(n + 3, H_SRC, W_SRC, seed=0)
    sd = weights.random_wasb_state_dict(0, planted=True)
    parts = {'resize_normalise': 0.0, 'cnn': 0.0, 'refine': 0.0, 'uplift': 0.0}
    per = []
    if style == 'b1':          # batch 1 per triple + table-variant fit, like interface.py:102-119, + one trajectory through the uplift net
        usd = weights.random_uplift_state_dict(0, 'large')
        t_w = time.time()
        xw = glue_ref.triple_to_tensor(frames[n], frames[n + 1], frames[n + 2], (W_NET, H_NET))[None]
        refine_ref.extract_position_table(wasb_ref.wasb_forward(xw, sd).numpy(), 1920, 1080)
        warm = time.time() - t_w
        t0 = time.time()
        for i in range(n):
            ta = time.time()
            x = glue_ref.triple_to_tensor(frames[i], frames[i + 1], frames[i + 2], (W_NET, H_NET))[None]
            tb = time.time()
            heat = wasb_ref.wasb_forward(x, sd).numpy()
            tc = time.time()
            refine_ref.extract_position_table(heat, 1920, 1080)
            td = time.time()
            parts['resize_normalise'] += tb - ta; parts['cnn'] += tc - tb; parts['refine'] += td - tc
            per.append(round(td - ta, 3))
        tu = time.time()
        ball, table, mask, times = synth.synth_trajectories(1, TRAJ_LEN, seed=0, pad=1)
        rot, p3 = uplift_ref.uplift_forward(ball, table, mask, times, usd)
        uplift_ref.transform_rotationaxes(rot, p3)
        parts['uplift'] = time.time() - tu
        dt = time.time() - t0
    else:                      # micro-batches of 4 + ball-variant fit, like inference/utils.py:51-59
        x = np.stack([glue_ref.triple_to_tensor(frames[i], frames[i + 1], frames[i + 2], (W_NET, H_NET)) for i in range(n)])
        t_w = time.time()
        refine_ref.extract_position_ball(wasb_ref.wasb_forward(x[:4], sd).numpy(), 1920, 1080)
        warm = time.time() - t_w
        t0 = time.time()
        for b0 in range(0, n, 4):
            ta = time.time()
            heat = wasb_ref.wasb_forward(x[b0:b0 + 4], sd).numpy()
            tb = time.time()
            refine_ref.extract_position_ball(heat, 1920, 1080)
            tc = time.time()
            parts['cnn'] += tb - ta; parts['refine'] += tc - tb
            per.append(round(tc - ta, 3))
        dt = time.time() - t0
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:
        aff = os.cpu_count()
    import resource
    ru = resource.getrusage(resource.RUSAGE_SELF)
    try:
        thp = open('/sys/kernel/mm/transparent_hugepage/enabled').read().strip()
    except OSError:
        thp = 'unknown'
    print(json.dumps({'rusage': {'user_s': round(ru.ru_utime, 1), 'sys_s': round(ru.ru_stime, 1), 'minor_faults': ru.ru_minflt}, 'thp': thp,
                      'glibc_tunables': os.environ.get('GLIBC_TUNABLES'), 'seconds': dt, 'triples': n, 'threads': torch.get_num_threads(), 'warmup_seconds': round(warm, 3), 'per_triple': per,
                      'parts': {k: round(v, 3) for k, v in parts.items()}, 'torch': torch.__version__,
                      'mkldnn': bool(torch.backends.mkldnn.is_available() and torch.backends.mkldnn.enabled), 'affinity': aff,
                      'omp': {k: os.environ.get(k) for k in ('OMP_NUM_THREADS', 'OMP_PROC_BIND', 'OMP_PLACES', 'GOMP_CPU_AFFINITY', 'KMP_AFFINITY') if os.environ.get(k)}}), flush=True)


def _cpu_model():
    try:
        for ln in open('/proc/cpuinfo'):
            if ln.startswith('model name'):
                return ln.split(':', 1)[1].strip()
    except OSError:
        pass
    return 'unknown'


CPU_POLICY = {'OMP_PROC_BIND': 'close', 'OMP_PLACES': 'cores', 'GLIBC_TUNABLES': 'glibc.malloc.hugetlb=1'}


def _run_cpu_child(style, n, threads, env_add, timeout):
    """`bench.py --cpu-child` in a fresh CPU-only process; its JSON line, or None when it did not finish inside `timeout` seconds."""
    env = dict(os.environ, OMP_NUM_THREADS=str(threads), MKL_NUM_THREADS=str(threads), **env_add)
    for k in ('TTUP_LIB', 'HIP_VISIBLE_DEVICES', 'ROCR_VISIBLE_DEVICES'):
        env.pop(k, None)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--cpu-child', style, str(n), str(threads)], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return None
    for ln in reversed(r.stdout.splitlines()):
        if ln.startswith('{'):
            return json.loads(ln)
    return None


def cpu_baseline():
    """The CPU oracle (torch fp32, kind "port": oracle/*_ref.py, pinned to the reference by the goldens) on a bounded sample of the same
    workload, in the reference's two calling styles -- (a) batch 1 per triple with the table-variant fit, like the hub surface
    (interface.py:102-119), + one 120-point trajectory through the uplift net; (b) micro-batches of 4 with the ball-variant fit, like the
    evaluation path (inference/utils.py:51-59).

    Every timing is a FRESH CPU-only child process (`--cpu-child`: its own OpenMP pool, OMP_NUM_THREADS set, one full-size warm-up
    triple, no GPU) and the whole leg runs BEFORE this process touches the GPU.  A sweep over 8 / 16 / 32 / 64 / 128 threads (2 timed
    triples each, cut off at 15 s) picks the thread count; the reported value is 8 triples at that count, `cores` = its threads.
    Environment of the children: OMP_PROC_BIND=close, OMP_PLACES=cores, GLIBC_TUNABLES=glibc.malloc.hugetlb=1.

    Why the tunable, and why rounds 3-4 (1.94 frames/s) and round 5 (0.37) disagreed on unchanged code: the eager fp32 graph allocates
    a fresh 100-900 MB tensor per layer, glibc mmap()s each, and with the host's transparent-hugepage mode at `madvise` (the round-5/6
    boxes) every one is faulted in as 4-KB pages -- 12.6 M page faults for four triples, a third of the CPU time in the kernel, and
    SLOWER with more threads (they queue on the process's memory map).  With malloc asking for huge pages the same run takes 0.21 M
    faults and 1.15 instead of 1.8-2.1 s per triple.  `plain` in the line is the best thread count WITHOUT the tunable.  The
    rounds-3/4 figure (0.52 s per triple) was not reproducible on any thread count or policy on the round-6 boxes; those rounds did not
    record the host's THP mode or CPU model (NOTES.md 15)."""
    model = _cpu_model()
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    sweep, best = [], None
    for t in (8, 16, 32, 64, 128):
        if t > avail:
            continue
        res = _run_cpu_child('b1', 2, t, CPU_POLICY, 15)
        if res is None:
            sweep.append({'threads': t, 'seconds_per_triple': '> %.1f (cut off at 15 s for warm-up + 2 triples)' % (15 / 3.0)})
            continue
        spt = res['seconds'] / res['triples']          # (includes the one uplift trajectory: 0.02 s)
        sweep.append({'threads': t, 'seconds_per_triple': round(spt, 3), 'user_s': res['rusage']['user_s'], 'sys_s': res['rusage']['sys_s'],
                      'minor_faults': res['rusage']['minor_faults']})
        if best is None or spt < best[1]:
            best = (t, spt)
    if best is None:
        return {'value': None, 'unit': 'frames/s', 'cores': 0, 'kind': 'port', 'sample': 'no CPU child finished', 'thread_sweep': sweep}, None
    t = best[0]
    n = int(os.environ.get('TTUP_CPU_BASELINE_TRIPLES', '8'))
    res = _run_cpu_child('b1', n, t, CPU_POLICY, 90) or {}
    plain = _run_cpu_child('b1', 2, t, {'OMP_PROC_BIND': 'close', 'OMP_PLACES': 'cores'}, 30)
    res4 = _run_cpu_child('b4', n, t, CPU_POLICY, 90)
    dt = res.get('seconds')
    base = {'value': round(n / dt, 4) if dt else None, 'unit': 'frames/s', 'cores': t, 'kind': 'port', 'cpu_model': model, 'host_threads': avail,
            'sample': '%d triples 1280x720, batch 1 (resize+normalise, CNN fp32, table-variant refine) + 1 trajectory of %d points, after one full-size '
                      'warm-up triple, in a fresh CPU-only process on %d OpenMP threads: %s s' % (n, TRAJ_LEN, t, ('%.1f' % dt) if dt else 'n/a'),
            'per_triple_s': res.get('per_triple'), 'parts_s': res.get('parts'), 'rusage': res.get('rusage'),
            'env': dict(CPU_POLICY, OMP_NUM_THREADS=str(t)), 'torch': res.get('torch'), 'mkldnn': res.get('mkldnn'), 'thp': res.get('thp'),
            'thread_sweep': sweep,
            'thread_sweep_note': 'fresh CPU-only process per thread count: one full-size warm-up triple, then 2 timed triples; run before this process touched the GPU',
            'plain': None if not plain else {'frames_per_s': round(plain['triples'] / plain['seconds'], 4), 'minor_faults': plain['rusage']['minor_faults'],
                                            'note': 'same thread count and binding without GLIBC_TUNABLES=glibc.malloc.hugetlb=1 (2 triples)'}}
    b4 = None
    if res4:
        b4 = {'value': round(res4['triples'] / res4['seconds'], 4), 'unit': 'frames/s', 'cores': t, 'kind': 'port', 'cpu_model': model, 'host_threads': avail,
              'sample': '%d triples 1280x720 in micro-batches of 4 (CNN fp32, ball-variant refine; resize+normalise outside the timing), inference/utils.py:51-59, '
                        'after one warm-up micro-batch, fresh CPU-only process on %d OpenMP threads: %.1f s' % (res4['triples'], t, res4['seconds'])}
    return base, b4


def from_host_leg(pipe, steps):
    """The headline step with the clip coming from the HOST every step (VERDICT r3 missing #7; the reference moves every frame host ->
    device, interface.py:110-112): the 258-frame uint8 clip sits in pinned memory, the upload of step k+1 runs on a copy stream
    (into one of three device buffers) while step k computes, and submit() waits for its clip's upload event.  Same worker, same
    streams as the headline; wall clock over `steps` steps after one warm-up step."""
    dev = pipe.frames.device
    host = torch.empty(pipe.frames.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(pipe.frames)
    bufs = [torch.empty_like(pipe.frames) for _ in range(3)]
    copy = torch.cuda.Stream(dev)

    def upload(i):
        with torch.cuda.stream(copy):
            bufs[i % 3].copy_(host, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        return ev
    e_up0, e_up1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(copy):
        e_up0.record(); bufs[0].copy_(host, non_blocking=True); e_up1.record()
    torch.cuda.synchronize()
    upload_ms = e_up0.elapsed_time(e_up1)

    def run(k):
        ticket, ev = None, upload(0)
        for i in range(k):
            torch.cuda.current_stream(dev).wait_event(ev)
            nxt = pipe.worker.submit(bufs[i % 3])
            if i + 1 < k:
                ev = upload(i + 1)          # overlaps with step i on the GPU
            if ticket is not None:
                pipe.collect(ticket)
            ticket = nxt
        pipe.collect(ticket)
        torch.cuda.synchronize()
    run(2)
    t0 = time.perf_counter()
    run(steps)
    dt = (time.perf_counter() - t0) / steps
    return {'value': round(TRIPLES / dt, 1), 'unit': 'frames/s', 'ms_per_step': round(dt * 1e3, 3), 'upload_ms_alone': round(upload_ms, 3),
            'upload_gbs_alone': round(host.numel() / upload_ms / 1e6, 1), 'bytes_per_step': int(host.numel()),
            'config': 'the headline step with its %d-frame uint8 clip uploaded from pinned host memory EVERY step on a copy stream, overlapped '
                      'with the previous step (three device buffers); the first upload of the run is inside the timed region' % host.shape[0]}


def _settle(worker, run_step, least=2, most=16):
    """Warm-up of a regime leg: steps until the worker's strip audit has dropped to its steady rate (one triple per `audit_every`
    after `audit_settle_clips` clips without a widening; before that one per `audit_every_fast`) -- the rate a long-running stream sees --
    at least `least`, at most `most`.  Returns the number of steps run."""
    n = 0
    while n < least or (n < most and worker.audit_rate() not in (0, worker.audit_every)):
        run_step()
        n += 1
    return n


def _audit_note(worker, au0, k, warm):
    """Audit activity of a leg's timed region (differences against `au0`, the counters at its start)."""
    au = worker.audit
    return {'warmup_steps': warm, 'audit_every_in_timed_region': au['audit_every_now'],
            'strip_audits_per_step': round((au['audited_frames'] - au0['audited_frames']) / max(1, k), 2),
            'audit_crops_per_step': round((au['audit_crop_frames'] - au0['audit_crop_frames']) / max(1, k), 2)}


def extras(device):
    """Driver-timed legs for the other BASELINE configs (N=1 only): CNN only (config 2), uplift only (config 3),
    trajectory generator (config 5), and the RK4 + Gauss-Newton fit named by north_star (extension)."""
    from upliftingtabletennis_amd import synth, uplift, wasb, weights
    out = {}
    # config 2: ball-detection CNN only, bf16, batch 256 (pre-processing, CNN, fused argmax + window; no refine / uplift)
    base, _ = synth.synth_frames(34, H_SRC, W_SRC, seed=1)
    clip = torch.from_numpy(np.concatenate([base] * 8)[:258]).to(device)
    net = wasb.WASBNet(weights.random_wasb_state_dict(0, planted=True), resolution=(W_NET, H_NET), max_batch=256, dtype='bf16', device=device)
    net.forward_frames(clip)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(4):
        net.forward_frames(clip)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 4
    out['cnn_only_fps'] = {'value': round(256 / dt, 1), 'unit': 'frames/s', 'config': 'BASELINE config 2: CNN only, bf16, batch 256 x 1280x720',
                           'ms_per_batch': round(dt * 1e3, 3), 'tflops': round(256 / dt * GFLOP_PER_FRAME_EXECUTED / 1e3, 1)}
    del net, clip
    # the full pipeline again on NOISE weights (no planted peak: near-ties on every heatmap, several crops per frame) -- the
    # certification load, and with it the throughput, depend on the weight set; the headline is the planted-peak regime
    try:
        pn = Pipeline(device, seed=0, certify=True, planted=False)
        warm = _settle(pn.worker, pn.step)
        torch.cuda.synchronize()
        au0 = pn.worker.audit
        # counters of the timed region only: the first warm-up clip runs on the default crop budget (one crop per heatmap) before
        # the worker has seen what this content asks for, and sends what does not fit to the full-frame fp32 path
        cs_warm, reruns_warm = pn.net.certify_stats(reset=True), pn.worker.fp32_reruns
        k = 4
        t0 = time.perf_counter()
        tk = None
        for _ in range(k):
            nx = pn.submit()
            if tk is not None:
                pn.collect(tk)
            tk = nx
        pn.collect(tk)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / k
        cs, au = pn.net.certify_stats(), pn.worker.audit
        out['noise_weights_fps'] = {'value': round(TRIPLES / dt, 1), 'unit': 'frames/s', 'ms_per_step': round(dt * 1e3, 2),
                                    'config': 'the headline workload on seeded NOISE weights (weights.random_wasb_state_dict(0, planted=False)), certified argmax on',
                                    'eps_abs': round(au['eps'], 6), 'crops_per_heatmap': round(cs['crops'] / max(1, cs['heatmaps']), 3), 'small_core_crop_share': round(cs['small_crops'] / max(1, cs['crops']), 3),
                                    'single_candidate_share': round(cs['single'] / max(1, cs['heatmaps']), 3), 'not_certified_share': round(cs['not_certified'] / max(1, cs['heatmaps']), 4),
                                    'fp32_full_frame_reruns': pn.worker.fp32_reruns - reruns_warm, 'max_err_over_eps': round(au['max_err_over_eps'], 4),
                                    'not_certified_causes': {'candidate_list': cs['over_candidates'], 'crops_per_heatmap': cs['over_crops_per_map'], 'crop_list': cs['over_crop_list']},
                                    'counters': 'timed region only (%d heatmaps)' % cs['heatmaps'], 'audit': _audit_note(pn.worker, au0, k, warm),
                                    'warmup': {'heatmaps': cs_warm['heatmaps'], 'not_certified': cs_warm['not_certified'], 'fp32_full_frame_reruns': reruns_warm,
                                               'note': 'the warm-up steps (until the strip audit is at its steady rate); the first one runs on the default crop budget of one crop per heatmap'}}
        del pn
        torch.cuda.empty_cache()
    except Exception as e:          # the regime leg must not take the headline line down
        out['noise_weights_fps'] = {'error': repr(e)[:300]}
    # parity mode: the headline workload with EXACT WINDOWS -- every heatmap gets an fp32 crop, so every 3x3 window that
    # the sub-pixel fit sees holds fp32 values and the refined (x, y) agrees with the reference to 1e-5 network px instead of 1e-2
    # (tests/test_e2e_gpu.py); the production mode keeps the bf16 window of single-candidate heatmaps
    try:
        pe = Pipeline(device, seed=0, certify=True, planted=True, exact_windows=True)
        warm = _settle(pe.worker, pe.step)
        torch.cuda.synchronize()
        pe.net.certify_stats(reset=True)
        au0, reruns0 = pe.worker.audit, pe.worker.fp32_reruns
        k = 4
        t0 = time.perf_counter()
        tk = None
        for _ in range(k):
            nx = pe.submit()
            if tk is not None:
                pe.collect(tk)
            tk = nx
        pe.collect(tk)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / k
        cs = pe.net.certify_stats()
        out['exact_windows_fps'] = {'value': round(TRIPLES / dt, 1), 'unit': 'frames/s', 'ms_per_step': round(dt * 1e3, 2),
                                    'config': 'the headline workload in parity mode (StreamWorker(exact_windows=True) / TTUP_EXACT_WINDOWS=1): an fp32 crop for EVERY heatmap, '
                                              'all 3x3 windows in fp32',
                                    'crops_per_heatmap': round(cs['crops'] / max(1, cs['heatmaps']), 3), 'small_core_crop_share': round(cs['small_crops'] / max(1, cs['crops']), 3), 'not_certified_share': round(cs['not_certified'] / max(1, cs['heatmaps']), 4),
                                    'fp32_full_frame_reruns': pe.worker.fp32_reruns - reruns0, 'audit': _audit_note(pe.worker, au0, k, warm)}
        del pe
        torch.cuda.empty_cache()
    except Exception as e:
        out['exact_windows_fps'] = {'error': repr(e)[:300]}
    # config 3: uplift only, 10 000 trajectories x 120 steps (+1 padded token)
    B, T = 10000, 120
    arrs = [torch.from_numpy(a).to(device) for a in synth.synth_trajectories(2000, T, seed=0, pad=1)]
    ball, table, mask, times = [a.repeat((5,) + (1,) * (a.dim() - 1)).contiguous() for a in arrs]
    up = uplift.get_model('connectstage', 'large', 'dynamic', 'new', state_dict=weights.random_uplift_state_dict(0, 'large'), max_batch=B, max_len=T + 1, device=device)
    up(ball[:64], table[:64], mask[:64], times[:64])
    up(ball, table, mask, times)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    up(ball, table, mask, times)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out['uplift_only_traj_s'] = {'value': round(B / dt, 1), 'unit': 'trajectories/s', 'config': 'BASELINE config 3: uplift transformer (the reference\'s uplift), B=10000, T=120',
                                 'seconds': round(dt, 4), 'tflops_fp32': round(B * 2.0 / dt / 1e3, 1)}
    del up
    # config 1 on the GPU: the torch.hub entry point on one 48-frame host clip (numpy frames in, spin + 3-D positions out)
    os.environ.setdefault('TTUP_SYNTHETIC_WEIGHTS', '1')
    import warnings
    import hubconf
    frames48, _ = synth.synth_frames(48, H_SRC, W_SRC, seed=0)
    images = [f for f in frames48]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        hub = hubconf.full_pipeline()
    hub.predict(images, 60.0)             # warm-up: staging buffers, streams, the detector's one-off fp32 calibration
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        hub.predict(images, 60.0)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    out['hub_clip_fps'] = {'value': round(len(images) / dt, 1), 'unit': 'frames/s', 'ms_per_clip': round(dt * 1e3, 2),
                           'config': 'BASELINE config 1 on the GPU: hubconf.full_pipeline().predict on a 48-frame 1280x720 host clip (upload, table HRNet on every '
                                     'frame + DBSCAN filter, ball detector, refine, uplift); wall clock'}
    # steady state of the same surface: a 256-frame clip.  The reference's own predict() cannot finish on it -- more than 49 valid
    # detections give a mask without a zero and uplifting/model.py:541-546 raises (kept: tests/test_fullsize_configs.py) -- so this
    # leg times the parts of predict() up to that point on all 256 frames (staging, upload, both detectors on every frame, keypoint
    # filter, filter_trajectory_ball) and runs the uplift on the first 49 detections, as a caller cutting rallies would
    try:
        from upliftingtabletennis_amd import glue
        frames256 = np.concatenate([frames48] * 6)[:256]
        images256 = [f for f in frames256]

        def long_clip():
            pos, kp = hub._clip_detections(images256, want_table=True, table_consumer=lambda k: hub.table_detector_aux.filter_trajectory(k, k))
            filt, _, tb = hub.ball_detector.filter_trajectory(pos, pos, 60.0)
            bc, tc, tm, mk = glue._uplifting_transform(filt[:49], np.asarray(kp, dtype=np.float64), tb[:49])
            return hub.uplifting_model.predict_without_normalization(bc, tc, mk, tm)
        long_clip()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            long_clip()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 2
        out['hub_clip_fps_256'] = {'value': round(256 / dt, 1), 'unit': 'frames/s', 'ms_per_clip': round(dt * 1e3, 2),
                                   'config': 'the hub pipeline\'s overlapped clip path on a 256-frame 1280x720 host clip: staging, upload, table HRNet (13 certified keypoints) on every '
                                             'frame + DBSCAN filter, ball detector (certified), refine, filter_trajectory_ball; uplift on the first 49 detections (the '
                                             'reference\'s predict() raises ValueError on a clip with more: uplifting/model.py:541-546); wall clock'}
    except Exception as e:
        out['hub_clip_fps_256'] = {'error': repr(e)[:300]}
    del hub
    try:
        from upliftingtabletennis_amd import odefit
        out['odefit_traj_s'] = odefit.bench(device, B, T)
    except ImportError:
        pass
    # config 5: 125 000 accepted drag+Magnus trajectories in the reference's output format
    from upliftingtabletennis_amd import trajgen
    trajgen.simulate_seeds(np.arange(262144), 'final_lose', 'left_to_right')       # warm-up at full size: the 9.7 GB sample buffer comes from the caching allocator afterwards
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = trajgen.simulate_seeds(np.arange(262144), 'final_lose', 'left_to_right')
    torch.cuda.synchronize()
    dt_dev = time.perf_counter() - t0
    acc = int((res['n_keep'] > 0).sum().item())
    del res
    t0 = time.perf_counter()
    tr = trajgen.get_valid_trajectories(125000, 128, 'final_lose', 'left_to_right', batches_per_launch=128)
    dt_cold = time.perf_counter() - t0          # first call: the pinned host blocks of the results are allocated (and page-locked) here
    n_rows = int(sum(len(c['rows']) for c in tr.chunks))
    del tr
    t0 = time.perf_counter()
    tr = trajgen.get_valid_trajectories(125000, 128, 'final_lose', 'left_to_right', batches_per_launch=128)
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    probe = [tr[i]['positions'].shape[0] for i in range(0, len(tr), 25)]          # the dict API is a thin adaptor: 5000 of them
    dt_views = time.perf_counter() - t0
    out['trajgen_traj_s'] = {'value': round(len(tr) / dt, 1), 'unit': 'trajectories/s', 'seconds': round(dt, 3),
                             'config': 'BASELINE config 5: 125000 accepted final_lose trajectories, device RK4 + selection, kept samples packed on the device and copied to '
                                       'pinned host memory; reference-format dictionaries are views made on access (trajgen.TrajectoryBatch)',
                             'first_call_seconds': round(dt_cold, 3), 'host_bytes': n_rows * 72, 'dict_views_per_s': round(len(probe) / dt_views, 1),
                             'device_seeds_s': round(262144 / dt_dev, 1), 'device_accepted_traj_s': round(acc / dt_dev, 1)}
    del tr
    # (last of the legs: every pipeline built here shifts the stream -> hardware-queue mapping of what follows)
    # the full pipeline on the headline weights but CHANGING content: four clips with their own background, noise, trajectory, blob
    # size (sigma 1.3 / 2 / 3 / 4 px: the wide ones have flat, saturated tops, i.e. near-ties on every heatmap) and brightness gain,
    # fed in turn -- the certification load of the headline clip (one blob size, one gain) is at the easy end
    try:
        from upliftingtabletennis_amd import synth
        pv = Pipeline(device, seed=0, certify=True, planted=True)
        clips = []
        for c, (sigma, gain) in enumerate(((1.3, 0.7), (2.0, 1.0), (3.0, 1.3), (4.0, 1.6))):
            base, _ = synth.synth_frames(34, H_SRC, W_SRC, seed=100 + c, sigma=sigma)
            base = np.clip(np.rint(base.astype(np.float32) * gain), 0, 255).astype(np.uint8)
            reps = (TRIPLES + 2 + len(base) - 1) // len(base)
            clips.append(torch.from_numpy(np.concatenate([base] * reps)[:TRIPLES + 2]).to(device))
        turn = [0]

        def one():                           # warm-up: the clips in turn until the audits have settled eps and their rate for this content
            pv.worker.collect(pv.worker.submit(clips[turn[0] % len(clips)]), pv.table_px, pv.fps)
            turn[0] += 1
        warm = _settle(pv.worker, one, least=len(clips), most=24)
        pv.net.certify_stats(reset=True)
        au0 = pv.worker.audit                # counters at the start of the timed region: the line reports the timed region's own
        pv.worker.margin_log = []            # fp32 top-2 margins of the timed region's heatmaps (ambiguous_share)
        torch.cuda.synchronize()
        k = 8
        t0 = time.perf_counter()
        tk = None
        for i in range(k):
            nx = pv.worker.submit(clips[i % len(clips)])
            if tk is not None:
                pv.worker.collect(tk, pv.table_px, pv.fps)
            tk = nx
        pv.worker.collect(tk, pv.table_px, pv.fps)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / k
        cs, au = pv.net.certify_stats(), pv.worker.audit
        mg = np.concatenate(pv.worker.margin_log) if pv.worker.margin_log else np.zeros(0, np.float32)
        pv.worker.margin_log = None
        out['varied_content_fps'] = {'value': round(TRIPLES / dt, 1), 'unit': 'frames/s', 'ms_per_step': round(dt * 1e3, 2),
                                     'config': 'the headline pipeline and weights on four alternating clips: blob sigma 1.3 / 2 / 3 / 4 px, brightness gain 0.7 / 1.0 / 1.3 / 1.6, own background and noise each',
                                     'eps_abs': round(au['eps'], 6), 'crops_per_heatmap': round(cs['crops'] / max(1, cs['heatmaps']), 3), 'small_core_crop_share': round(cs['small_crops'] / max(1, cs['crops']), 3),
                                     'single_candidate_share': round(cs['single'] / max(1, cs['heatmaps']), 3), 'not_certified_share': round(cs['not_certified'] / max(1, cs['heatmaps']), 4),
                                     'eps_widened': au['widened'] - au0['widened'], 'recertified_clips': au['recertified_clips'] - au0['recertified_clips'],
                                     'recertified_heatmaps': au['recertified_heatmaps'] - au0['recertified_heatmaps'],
                                     'counters': 'timed region only (eps_widened / recertified_* are differences against the end of the warm-up)',
                                     'eps_widened_in_warmup': au0['widened'], 'audit': _audit_note(pv.worker, au0, k, warm)}
        if mg.size:
            # "reference-ambiguous" heatmaps: the fp32 winner leads the best other candidate by less than DELTA_REF, the measured bound
            # on |HIP fp32 heatmap - reference heatmap| x 2 (tests/test_fullsize_configs.py::test_certified_argmax_matches_the_reference_on_near_ties)
            out['varied_content_fps']['certified_argmax'] = {
                'ambiguous_share': round(float((mg < DELTA_REF).mean()), 4), 'delta_ref': DELTA_REF, 'heatmaps': int(mg.size),
                'margin_below': {('%g' % d): round(float((mg < d).mean()), 4) for d in (1e-5, 1e-4, 1e-3, 1e-2)},
                'note': 'share of the timed region\'s heatmaps whose fp32 top-2 margin among the candidates is below delta_ref: there the reference\'s own fp32 argmax '
                        '(torch CPU summation order) and any other fp32 evaluation may pick different pixels of the tied set'}
        del pv, clips
        torch.cuda.empty_cache()
    except Exception as e:
        out['varied_content_fps'] = {'error': repr(e)[:300]}
    return out


def spawn_ranks(a):
    """`python bench.py --gpus N` outside torch.distributed: start the N ranks as a child `torch.distributed.run`
    (this process has not touched the GPU: no torch.cuda.is_available(), no HIP call) and relay rank 0's JSON line."""
    n_dev = torch.cuda.device_count()          # does not initialise the GPU on this image
    if n_dev < a.gpus and os.environ.get('TTUP_BENCH_SHARE_GPU') != '1':
        print('bench.py: --gpus %d but only %d device(s) visible (TTUP_BENCH_SHARE_GPU=1 TTUP_DIST_BACKEND=gloo runs a dry run '
              'of the multi-rank flow on fewer devices)' % (a.gpus, n_dev), file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(a.gpus), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__), '--gpus', str(a.gpus), '--steps', str(a.steps), '--warmup', str(a.warmup)]
    cmd += ['--full'] * a.full + ['--no-cpu-baseline'] * a.no_cpu_baseline + ['--no-roofline'] * a.no_roofline + ['--no-extras'] * a.no_extras + ['--no-certify'] * a.no_certify
    if a.dump_outputs:
        cmd += ['--dump-outputs', os.path.abspath(a.dump_outputs)]
    if a.ops_json:
        cmd += ['--ops-json', os.path.abspath(a.ops_json)]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', str(max(1, min(8, (os.cpu_count() or 8) // max(1, a.gpus)))))
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in r.stdout.splitlines():
        if ln.startswith('{') and '"metric"' in ln:
            line = ln
        else:
            print(ln, file=sys.stderr)
    if r.returncode != 0 or line is None:
        print('bench.py: the %d-rank run failed (exit code %d)' % (a.gpus, r.returncode), file=sys.stderr)
        return r.returncode or 1
    print(line, flush=True)
    return 0


def pin_rank_to_cores(local, n_local):
    """Per-rank CPU affinity, set before anything touches the GPU (the runtime's helper threads inherit it): the cores this process
    may use are cut into `n_local` contiguous blocks and rank `local` keeps block `local` -- the ranks of one node then never
    migrate onto each other's cores (the host glue of a step is a few hundred microseconds of numpy between two launches, and a
    descheduled rank is what the max-over-ranks timing sees).  Returns the cores kept (all of them at n_local = 1)."""
    try:
        cores = sorted(os.sched_getaffinity(0))
    except AttributeError:
        return None
    if n_local <= 1 or len(cores) < n_local or os.environ.get('TTUP_NO_AFFINITY') == '1':
        return cores
    q, r = divmod(len(cores), n_local)
    lo = local * q + min(local, r)
    mine = cores[lo:lo + q + (1 if local < r else 0)]
    os.sched_setaffinity(0, mine)
    return mine


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == '--cpu-child':          # a CPU-oracle timing of cpu_baseline(): never touches the GPU
        return _cpu_child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    a = parse()
    share = os.environ.get('TTUP_BENCH_SHARE_GPU') == '1'
    if a.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(spawn_ranks(a))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world != a.gpus:
        raise SystemExit('bench.py: --gpus %d does not match WORLD_SIZE %d' % (a.gpus, world))
    cores = pin_rank_to_cores(local, int(os.environ.get('LOCAL_WORLD_SIZE', world)))          # before the first GPU call
    # the CPU baseline FIRST: fresh CPU-only children, nothing of this process on the GPU or the host cores yet
    cpu_lines = cpu_baseline() if (not a.no_cpu_baseline and world == 1) else None
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a HIP device (there is no CPU fallback); the CPU oracle is only the baseline leg')
    # TTUP_BENCH_SHARE_GPU=1 + TTUP_DIST_BACKEND=gloo: dry run of the multi-rank flow on a box with fewer GPUs than ranks
    # (ranks share devices, the gather goes through the host); the measured configuration is one rank per GPU over RCCL
    backend = os.environ.get('TTUP_DIST_BACKEND', 'nccl')
    if share:
        local = local % torch.cuda.device_count()
    elif local >= torch.cuda.device_count():
        raise SystemExit('bench.py: rank %d has no GPU (%d visible)' % (local, torch.cuda.device_count()))
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    # host threads per rank: the host glue (filter / pad of a few hundred detections, pinned copies) is small; N ranks with the
    # default thread pool each would oversubscribe the box's cores.  torch.distributed.run exports OMP_NUM_THREADS=1 when it is
    # unset; the direct path and the self-spawned path end up with the same explicit setting here.
    host_threads = int(os.environ.get('TTUP_THREADS_PER_RANK', max(1, min(8, len(cores) if cores else (os.cpu_count() or 8) // max(1, world)))))
    torch.set_num_threads(host_threads)
    # The worker and ALL its streams first, the process group after them: HIP maps streams onto four hardware queues in the order in
    # which they are created, the pipeline's throughput depends on that mapping by up to 6 % (tools/queue_probe.py),
    # and RCCL takes streams of its own -- every rank of an N-GPU run thus gets the mapping the single-GPU run has.
    pipe = Pipeline(device, seed=rank, certify=not a.no_certify)
    for _ in range(a.warmup):
        pipe.step()
    pipe.worker.submit_streams()
    if os.environ.get('TTUP_BENCH_FAIL_RANK') == str(rank):          # test hook: a rank that dies must take the whole run down with a non-zero exit code
        raise SystemExit('bench.py: rank %d failing on request (TTUP_BENCH_FAIL_RANK)' % rank)
    dist = None
    collective = None
    pre_init_q = None
    probe_queues = (a.full and world > 1) or os.environ.get('TTUP_BENCH_QUEUE_PROBE') == '1'
    if world > 1:
        # the worker's stream -> hardware-queue grouping BEFORE the process group exists (RCCL creates streams of its own): compared
        # with the grouping after the timed region, `queue_mapping_changed` in the line says whether the collective's streams moved it
        if probe_queues:
            try:
                pre_init_q = pipe.worker.queue_groups()
            except Exception as e:
                pre_init_q = 'probe failed: %r' % (e,)
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        if backend == 'nccl':
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        # prove the collective backend sees every rank: a sum of ones over device tensors (RCCL) must equal the world size
        ones = torch.ones(1, device=device if backend == 'nccl' else 'cpu')
        dist.all_reduce(ones)
        collective = {'backend': dist.get_backend(), 'ranks': int(ones.item()), 'world_size': dist.get_world_size()}
        if collective['ranks'] != world:
            raise SystemExit('bench.py: all_reduce saw %d of %d ranks' % (collective['ranks'], world))

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
    barrier()
    t0 = time.perf_counter()
    from upliftingtabletennis_amd import pipeline
    # K steps, software-pipelined one deep: the detector of step k+1 is enqueued before the host filters / pads the
    # detections of step k and enqueues their uplift, so the GPU does not idle during the host glue.  Every step's
    # detect + refine + uplift + gather completes inside the timed region (the last collect is before the barrier).
    ticket = None
    spec = pipe.worker.record_spec()
    keys = pipe.worker.RECORD_KEYS
    gather_s = []

    def gather(rec):
        # final gather of the small per-frame / per-trajectory records: the only collective on the path, ONE all_gather per step
        g0 = time.perf_counter()
        out = pipeline.gather_records({k: rec[k] for k in keys}, dist, spec=spec)
        gather_s.append(time.perf_counter() - g0)          # host wall clock of the call (pack, all_gather, unpack on rank 0)
        return out
    for _ in range(a.steps):
        nxt = pipe.submit()
        if ticket is not None:
            gathered = gather(pipe.collect(ticket))
        ticket = nxt
    gathered = gather(pipe.collect(ticket))
    torch.cuda.synchronize()
    dt_own = time.perf_counter() - t0          # this rank's own K steps, before it waits for the others
    if dist is not None and rank == 0:
        n_rows = sum(int(t.shape[0]) for t in gathered['xyv'])
        if n_rows != TRIPLES * world:
            raise SystemExit('bench.py: the gather returned %d detections, expected %d' % (n_rows, TRIPLES * world))
    barrier()
    dt = time.perf_counter() - t0
    per_rank = None
    if dist is not None:
        # after the timed region: every rank's wall clock (value = work of all ranks / the MAX), its own un-barriered step time and
        # its gather times, so that an N-GPU line explains its own spread
        mine = torch.tensor([dt, dt_own, float(np.mean(gather_s)), float(np.max(gather_s))], device=device if backend == 'nccl' else 'cpu', dtype=torch.float64)
        allr = torch.empty((world * 4,), device=mine.device, dtype=torch.float64)
        dist.all_gather_into_tensor(allr, mine)
        allr = allr.cpu().reshape(world, 4)
        dt = float(allr[:, 0].max())
        own = allr[:, 1] / a.steps * 1e3
        per_rank = {'ms_per_step_min': round(float(own.min()), 3), 'ms_per_step_max': round(float(own.max()), 3),
                    'ms_per_step': [round(float(v), 3) for v in own], 'gather_ms_mean': [round(float(v) * 1e3, 3) for v in allr[:, 2]],
                    'gather_ms_max': [round(float(v) * 1e3, 3) for v in allr[:, 3]],
                    'note': 'ms_per_step = each rank\'s own K steps up to its last synchronize (before the closing barrier); gather = host wall clock of '
                            'gather_records (pack + all_gather_into_tensor + unpack on rank 0), which also absorbs the wait for the slowest rank of the step'}
    if a.dump_outputs and rank == 0:          # after the timed region, before any later leg reuses the worker
        dump_outputs(gathered, a.dump_outputs)
    # stream -> hardware-queue grouping of every rank's worker (after the timed region, one rank at a time: ranks that share a
    # GPU in a dry run would disturb each other's probes): the single-GPU mapping is the best one seen and every
    # rank should have it -- an N-GPU line then says so itself
    queue_groups = None
    if probe_queues:
        mine_q = None
        for r in range(world):
            if r == rank:
                try:
                    mine_q = pipe.worker.queue_groups()
                except Exception as e:
                    mine_q = 'probe failed: %r' % (e,)
            if dist is not None:
                dist.barrier()
        if dist is not None:
            allq = [None] * world
            dist.all_gather_object(allq, mine_q)
            allpre = [None] * world
            dist.all_gather_object(allpre, pre_init_q)
        else:
            allq, allpre = [mine_q], [pre_init_q]
        queue_groups = {'per_rank': allq, 'all_equal': len(set(allq)) == 1}
        if dist is not None:
            queue_groups['pre_init_per_rank'] = allpre
            queue_groups['queue_mapping_changed'] = any(a_ != b_ for a_, b_ in zip(allpre, allq))
            queue_groups['note'] = ('pre_init = probed after the warm-up, before init_process_group; per_rank = after the timed region; with ranks sharing '
                                    'a GPU (dry run) the spin-kernel probe is disturbed by the other ranks and the flag is not meaningful') if share else \
                                   'pre_init = probed after the warm-up, before init_process_group; per_rank = after the timed region'
    frames = TRIPLES * a.steps * world
    line = {'metric': 'frames/sec end-to-end (detect+uplift), 1280x720', 'value': round(frames / dt, 2), 'unit': 'frames/s',
            'n_gpus': world, 'steps': a.steps, 'warmup': a.warmup, 'ms_per_step': round(dt / a.steps * 1e3, 3),
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'bf16', 'data': 'synthetic',
            'config': {'workload': 'full detect->uplift pipeline: %d triples of 1280x720 uint8 frames per step per GPU (WASB/HRNet @1280x704, '
                                   'table-variant refine), cut into %d trajectories of up to %d detections (%d tokens) through the uplift transformer; '
                                   'random-init weights' % (TRIPLES, (TRIPLES + TRAJ_LEN - 1) // TRAJ_LEN, TRAJ_LEN, SEQ_LEN),
                       'frames_per_step_per_gpu': TRIPLES, 'parallelism': 'stream-per-gpu x%d, final gather' % world}}
    if pipe.worker.certify:
        cs = pipe.net.certify_stats()
        au = pipe.worker.audit
        line['certified_argmax'] = {'eps_abs': round(pipe.worker.certify_eps, 6), 'heatmaps': cs['heatmaps'], 'single_candidate': cs['single'],
                                    'resolved_on_fp32_crops': cs['resolved'], 'not_certified': cs['not_certified'], 'crops': cs['crops'],
                                    'fp32_full_frame_reruns': pipe.worker.fp32_reruns,
                                    'audited_frames': au['audited_frames'], 'audit_every_frames': pipe.worker.audit_every,
                                    'audit_every_frames_fast': pipe.worker.audit_every_fast, 'audit_settle_clips': pipe.worker.audit_settle_clips,
                                    'audit_every_now': au['audit_every_now'], 'frames_seen': au['frames_seen'],
                                    'audited_share': round(au['audited_share'], 5) if au['audited_share'] else None,
                                    'strip_audited_share': round(au['strip_audited_share'], 5) if au.get('strip_audited_share') else None,
                                    'audit_crops_every': pipe.worker.audit_crops_every, 'audit_crop_frames': au.get('audit_crop_frames'), 'widen_sources': au['widen_sources'],
                                    'max_err_seen': round(au['max_err_seen'], 6), 'max_candidate_err': round(cs['max_candidate_err'], 6),
                                    'max_err_over_eps': round(au['max_err_over_eps'], 4), 'eps_widened': au['widened'], 'recertified_clips': au['recertified_clips'], 'recertified_heatmaps': au['recertified_heatmaps'],
                                    'note': 'an index is the fp32 argmax whenever |bf16 - fp32| <= eps on its frame (csrc/certify.hip); eps is audited inside the timed '
                                            'steps: one random frame per audit_every frames on the fp32 twin (side stream; per audit_every_frames_fast until eps has stood for audit_settle_clips clips in a row: strip_audited_share = those / processed frames) + audit crops (one single-candidate heatmap per audit_crops_every triples gets an fp32 crop that measures |bf16 - fp32| at its winner; audited_share counts both) + the error at every candidate of every crop; '
                                            'eps = 1.5 x the largest error seen; a new maximum widens it and the heatmaps whose guard band (2 eps .. 2.5 eps below the maximum) is not empty are run again, the whole clip when eps grows by more than a quarter at once.  Counts cover warm-up + timed steps'}
    line['host_threads_per_rank'] = host_threads
    line['cpu_affinity'] = {'cores_of_rank0': ('%d-%d (%d cores)' % (cores[0], cores[-1], len(cores))) if cores and cores == list(range(cores[0], cores[-1] + 1)) else cores, 'policy': 'contiguous block per local rank (os.sched_setaffinity before the first GPU call)'}
    line['gather_ms_per_step'] = round(float(np.mean(gather_s)) * 1e3, 3)
    if per_rank is not None:
        line['per_rank'] = per_rank
    if queue_groups is not None:
        line['stream_queue_groups'] = queue_groups
        if 'queue_mapping_changed' in queue_groups:
            line['queue_mapping_changed'] = queue_groups['queue_mapping_changed']
    from upliftingtabletennis_amd import _lib as _l
    line['build_id'] = _l.build_id()          # hash of csrc/* + include/ttup.h compiled into libttup.so, checked against the tree at load
    if collective is not None:
        line['collectives_per_step'] = 1
        line['rccl_ranks'] = collective['ranks'] if collective['backend'] == 'nccl' else 0
        line['collective'] = collective
    if rank == 0 and world == 1 and not a.no_extras:
        line['e2e_from_host_fps'] = from_host_leg(pipe, a.steps)
    if rank == 0:
        if not a.no_roofline:
            r, ops = roofline(pipe)
            line['roofline'] = r
            prod, seam = heatmap_roofline(device, pipe.worker.certify_eps or 0.05)
            line['roofline_heatmap'] = prod
            line['roofline_heatmap_seam'] = seam
            try:          # measured peaks of THIS device beside the vendor figures (csrc/peaks.hip)
                from upliftingtabletennis_amd import peaks
                pk = peaks.measure(device)
                r['peak_measured'] = round(pk['peak_bf16_tflops'], 1)
                r['frac_measured'] = round(r['achieved'] / pk['peak_bf16_tflops'], 4)
                for k in ('longest_kernel', 'lowest_kernel'):
                    r[k]['frac_measured'] = round(r[k]['achieved'] / pk['peak_bf16_tflops'], 4)
                for h in (prod, seam):
                    h['peak_measured'] = round(pk['peak_hbm_gbs'], 1)
                    h['frac_measured'] = round(h['achieved'] / pk['peak_hbm_gbs'], 4)
                line['peaks_measured'] = pk
            except Exception as e:
                line['peaks_measured'] = {'error': repr(e)[:300]}
            line['cnn_gflop_per_frame'] = GFLOP_PER_FRAME_EXECUTED
            line['cnn_tflops_end_to_end'] = round(frames / dt * GFLOP_PER_FRAME_EXECUTED / 1e3, 2)
            if a.ops_json:
                with open(a.ops_json, 'w') as f:
                    json.dump(ops, f, indent=1)
        if not a.no_extras and world == 1:
            del pipe
            torch.cuda.empty_cache()
            line.update(extras(device))
        if cpu_lines is not None:
            line['cpu_baseline'], line['cpu_baseline_b4'] = cpu_lines
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
