#!/usr/bin/env python3
"""Generate tests/golden/dataset.npz by running the REFERENCE's own uplifting/data.py::TableTennisDataset and the transforms of
uplifting/transformations.py on seeded (trajectory, sample seed) pairs.

Runs only where the reference sources are (TTUP_REFERENCE); the tests read the .npz alone.  cv2 / tensorboard are stubbed as in
tools/make_goldens.py, `paths.data_path` points at a temporary folder in the `save_dataset` layout.

Input trajectories: 24 (every mode x direction x 2) from oracle/trajgen_ref.py on the CPU -- input data, stored in the fixture
(positions, first rotation, bounces; `--cache DIR` keeps them between runs: the CPU integrator needs minutes per mode).
A sample with seed s is `random.seed(s); np.random.seed(s); dataset[i]`.  The reference returns float32 tensors; the float64
arrays behind them are recorded at its own `torch.tensor(..., dtype=torch.float32)` calls, and the integer record (fps, frames,
camera tries, blur samples, dropped frames) is read off its own calls: `random.randint`'s result, the argument of
`sample_camera`, the eight `random.uniform` calls per try, the rows MotionBlur wrote, the times RandomMissing kept.

Cases: the full train pipeline on >= 96 pairs (at least 8 with >= 2 camera tries), each transform alone on 24, 'test' mode on 24,
the order of `data_paths` for a small folder tree, and raw words of both MT19937 streams.  A candidate pair is left out when a
decision sits on a knife edge for a device whose sin / cos differ from glibc's in the last bits (tests/helpers/dataset_ref.py
computes the margins): in-image / extent test within 1e-6 px, |u[2]| < 1e-9, polar r2 within 1e-12 of 1.  The share left out is
printed and must stay below 2 %.  Also printed: the reference's own time per sample (single core), for DESIGN.md 16.

    python tools/make_goldens_dataset.py [--cache DIR]
"""
import concurrent.futures
import os
import pickle
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TTUP_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from oracle import trajgen_ref  # noqa: E402
from tests.helpers import dataset_ref as R  # noqa: E402
from tools.make_goldens import install_stubs  # noqa: E402

CONFIG = {'blur_strength': 0.4, 'randomize_std': 8, 'stop_prob': 0.5, 'randdet_prob': 0.05, 'randmiss_prob': 0.05, 'tablemiss_prob': 0.05}
# each transform alone: strong enough that every branch is taken within 24 samples
SINGLE = {'blur_strength': 0.25, 'randomize_std': 5, 'stop_prob': 0.9, 'randdet_prob': 0.3, 'randmiss_prob': 0.3, 'tablemiss_prob': 0.3}
N_FULL, MIN_MULTI_TRY = 96, 8
STREAM_SEEDS = [0, 1, 12345, 2 ** 32 - 1]
STREAM_WORDS = 1500


def _trajectories_of(args):
    mode, direction = args
    times = trajgen_ref.save_times()
    found, cur, batch = [], 0, 384
    while len(found) < 2:
        seeds = list(range(cur, cur + batch))
        pos, vel, rot, ns = trajgen_ref.simulate(seeds, mode, direction)
        for i, s in enumerate(seeds):
            res = trajgen_ref.select(pos[i, :ns[i]], times, mode, direction)
            if res is not None:
                n, b = res
                found.append({'positions': pos[i, :n].copy(), 'velocities': vel[i, :n].copy(), 'rotations': rot[i, :n].copy(),
                              'times': times[:n].copy(), 'bounces': np.asarray(b, np.float64), 'seed': s})
        cur += batch
    return found[:2]


def make_trajectories(cache):
    combos = [(m, d) for m in trajgen_ref.MODES for d in trajgen_ref.DIRECTIONS]
    out = {}
    todo = []
    for c in combos:
        p = cache and os.path.join(cache, 'traj_%s_%s.pkl' % c)
        if p and os.path.exists(p):
            out[c] = pickle.load(open(p, 'rb'))
        else:
            todo.append(c)
    with concurrent.futures.ProcessPoolExecutor(max_workers=12) as ex:
        for c, res in zip(todo, ex.map(_trajectories_of, todo)):
            out[c] = res
            if cache:
                pickle.dump(res, open(os.path.join(cache, 'traj_%s_%s.pkl' % c), 'wb'))
    ex_m, mint = trajgen_ref.camera_matrices()
    trajs = []
    for c in combos:
        for t in out[c]:
            n = len(t['times'])
            t = dict(t, Mext=np.repeat(ex_m[None], n, 0), Mint=np.repeat(mint[None], n, 0), mode=c[0], direction=c[1])
            trajs.append(t)
    return trajs


class Recorder:
    """Stands in for the modules `random` / `torch` inside uplifting.data: passes every call on and keeps what went through."""
    def __init__(self):
        self.reset()

    def reset(self):
        self.fps, self.uniforms, self.f64, self.n_frames = None, 0, [], None

    # random
    def randint(self, a, b):
        self.fps = random.randint(a, b)
        return self.fps

    def uniform(self, a, b):
        self.uniforms += 1
        return random.uniform(a, b)

    def Random(self, *a):
        return random.Random(*a)

    # torch
    float32 = torch.float32
    utils = torch.utils

    def tensor(self, x, dtype=None):
        self.f64.append(np.array(x, copy=True))
        return torch.tensor(x, dtype=dtype)


def reference_dataset(root, trajs, mode, transforms, rec):
    import uplifting.data as D
    ds = D.TableTennisDataset.__new__(D.TableTennisDataset)
    # the constructor lists folders and cuts the 70/10/20 split; here every one of the 24 trajectories is addressed directly
    D.TableTennisDataset.__init__(ds, mode, transforms)
    ds.data_paths = [t['path'] for t in trajs]
    ds.length = len(ds.data_paths)
    orig = ds.sample_camera

    def counted(r_world):
        rec.n_frames = len(r_world)
        return orig(r_world)
    ds.sample_camera = counted
    return ds


def compose(names, cfg):
    import uplifting.transformations as TR
    mk = {'MotionBlur': lambda: TR.MotionBlur(cfg['blur_strength']), 'RandomizeDetections': lambda: TR.RandomizeDetections(cfg['randomize_std']),
          'RandomStop': lambda: TR.RandomStop(cfg['stop_prob']), 'RandomDetection': lambda: TR.RandomDetection(cfg['randdet_prob']),
          'RandomMissing': lambda: TR.RandomMissing(cfg['randmiss_prob']), 'TableMissing': lambda: TR.TableMissing(cfg['tablemiss_prob'])}
    rec = {}
    ts = []
    for n in R.TRANSFORM_NAMES:
        t = mk[n]() if n in names else TR.Identity()
        if n == 'MotionBlur' and n in names:
            inner = t

            def blur(data, inner=inner):
                data = inner(data)
                L = int(np.sum(data['mask']))
                bp = data['blur_positions']
                rec['blur_idx'] = [int(np.nonzero((bp == data['r_world'][i]).all(1))[0][0]) for i in range(L)]
                return data
            t = blur
        if n == 'RandomMissing' and n in names:
            inner2 = t

            def miss(data, inner2=inner2):
                before, L = data['times'].copy(), int(np.sum(data['mask']))
                data = inner2(data)
                kept = set(data['times'][:int(np.sum(data['mask']))].tolist())
                rec['dropped'] = [before[i] not in kept for i in range(L)]
                return data
            t = miss
        ts.append(t)
    ts.append(TR.NormalizeImgCoords())
    return TR.Compose(ts), rec


def run_case(ds, rec, trec, i, seed):
    rec.reset()
    trec.clear()
    random.seed(seed)
    np.random.seed(seed)
    out = ds[i]
    f64 = rec.f64
    assert len(f64) == 9
    for a, b in zip(out[:6] + out[7:], f64[:6] + f64[7:]):
        assert np.array_equal(a.numpy(), np.asarray(b).astype(np.float32))
    f64[6] = np.asarray(f64[6], np.float64)[0:1]
    assert np.array_equal(out[6].numpy(), f64[6].astype(np.float32))
    train = ds.mode == 'train'
    tries = rec.uniforms // 8
    ints = {'fps': rec.fps if train else 50, 'n_frames': rec.n_frames if train else -1, 'camera_tries': tries,
            'camera_success': int(train and tries < 100)}
    blur = np.full(50, -1, np.int64)
    blur[:len(trec.get('blur_idx', []))] = trec.get('blur_idx', [])
    dropped = np.zeros(50, bool)
    dropped[:len(trec.get('dropped', []))] = trec.get('dropped', [])
    return [np.asarray(a, np.float64) for a in f64], ints, blur, dropped


def check_restatement(traj, seed, mode, cfg, enabled, f64, ints, blur, dropped):
    """The numpy restatement must agree before its margins mean anything."""
    s = R.build_sample(traj, seed, mode, cfg, enabled)
    for name, ref in zip(R.OUTPUTS, f64):
        np.testing.assert_allclose(s[name], ref.reshape(s[name].shape), rtol=1e-12, atol=1e-12, err_msg=name)
    assert np.array_equal(s.mask, f64[2])
    if mode == 'train':
        assert (s.fps, s.n_frames, s.camera_tries, s.camera_success) == (ints['fps'], ints['n_frames'], ints['camera_tries'], ints['camera_success']), (ints, s.fps, s.n_frames, s.camera_tries)
    assert np.array_equal(s.blur_idx, blur) and np.array_equal(s.dropped, dropped)
    return s


def knife_edge(s):
    m = s.margins
    return m['min_border'] < 1e-6 or m['min_extent'] < 1e-6 or m['min_u2'] < 1e-9 or s.r2_margin < 1e-12


def main():
    cache = sys.argv[sys.argv.index('--cache') + 1] if '--cache' in sys.argv else None
    trajs = make_trajectories(cache)
    install_stubs()
    tmp = tempfile.mkdtemp()
    root = os.path.join(tmp, 'syntheticdata')
    import paths
    paths.data_path = tmp
    import uplifting.helper
    uplifting.helper.DATA_PATH = tmp
    import uplifting.data as D
    D.DATA_PATH = tmp
    count = {}
    for t in trajs:
        k = count.get((t['mode'], t['direction']), 0)
        count[(t['mode'], t['direction'])] = k + 1
        t['path'] = os.path.join(root, t['mode'], t['direction'], 'trajectory_%04d' % k)
        os.makedirs(t['path'])
        for key in ('positions', 'velocities', 'rotations', 'times', 'Mext', 'Mint', 'bounces'):
            np.save(os.path.join(t['path'], key + '.npy'), t[key])
    rec = Recorder()
    D.random, D.torch = rec, rec

    out = {}
    nk = np.array([len(t['times']) for t in trajs], np.int64)
    out['traj/positions'] = np.concatenate([t['positions'] for t in trajs])
    out['traj/offsets'] = np.concatenate([[0], np.cumsum(nk)]).astype(np.int64)
    out['traj/rotation0'] = np.stack([t['rotations'][0] for t in trajs])
    out['traj/bounces'] = np.stack([np.pad(t['bounces'], (0, 4 - len(t['bounces']))) for t in trajs])
    out['traj/n_bounces'] = np.array([len(t['bounces']) for t in trajs], np.int32)
    out['traj/times'] = trajgen_ref.save_times()
    out['traj/Mext'], out['traj/Mint'] = trajs[0]['Mext'][0], trajs[0]['Mint'][0]

    def store(prefix, rows):
        for j, name in enumerate(R.OUTPUTS):
            out['%s/%s' % (prefix, name)] = np.stack([r[0][j] for r in rows])
        for key in ('fps', 'n_frames', 'camera_tries', 'camera_success'):
            out['%s/%s' % (prefix, key)] = np.array([r[1][key] for r in rows], np.int32)
        out[prefix + '/blur_idx'] = np.stack([r[2] for r in rows]).astype(np.int16)
        out[prefix + '/dropped'] = np.stack([r[3] for r in rows])
        out[prefix + '/traj'] = np.array([r[4] for r in rows], np.int64)
        out[prefix + '/seed'] = np.array([r[5] for r in rows], np.int64)

    candidates = left_out = 0
    # ---- full train pipeline
    tf, trec = compose(R.TRANSFORM_NAMES, CONFIG)
    ds = reference_dataset(root, trajs, 'train', tf, rec)
    rows, multi, seed = [], 0, 1000
    t_ref, n_ref = 0.0, 0
    while len(rows) < N_FULL or multi < MIN_MULTI_TRY:
        i = seed % len(trajs)
        t0 = time.perf_counter()
        f64, ints, blur, dropped = run_case(ds, rec, trec, i, seed)
        t_ref += time.perf_counter() - t0
        n_ref += 1
        s = check_restatement(trajs[i], seed, 'train', CONFIG, R.ALL_ON, f64, ints, blur, dropped)
        candidates += 1
        if knife_edge(s):
            left_out += 1
        elif len(rows) < N_FULL or ints['camera_tries'] >= 2:
            rows.append((f64, ints, blur, dropped, i, seed))
            multi += ints['camera_tries'] >= 2
        seed += 1
    store('full', rows)
    print('full pipeline: %d cases, %d with >= 2 camera tries, numpy stream %d ... %d words per sample' %
          ((len(rows), multi) + (lambda c: (min(c), max(c)))([R.build_sample(trajs[r[4]], r[5], 'train', CONFIG).np_stream.count for r in rows])))
    # ---- each transform alone
    for k, name in enumerate(R.TRANSFORM_NAMES):
        tf, trec = compose([name], SINGLE)
        ds = reference_dataset(root, trajs, 'train', tf, rec)
        rows, seed = [], 5000 + 100 * k
        while len(rows) < len(trajs):
            i = len(rows)
            f64, ints, blur, dropped = run_case(ds, rec, trec, i, seed)
            s = check_restatement(trajs[i], seed, 'train', SINGLE, 1 << k, f64, ints, blur, dropped)
            candidates += 1
            if knife_edge(s):
                left_out += 1
            else:
                rows.append((f64, ints, blur, dropped, i, seed))
            seed += 1
        store('single/' + name, rows)
    # ---- test mode
    tf, trec = compose([], CONFIG)
    import uplifting.transformations as TR
    ds = reference_dataset(root, trajs, 'test', TR.Compose([TR.NormalizeImgCoords()]), rec)
    rows = []
    for i in range(len(trajs)):
        f64, ints, blur, dropped = run_case(ds, rec, trec, i, 77 + i)
        s = check_restatement(trajs[i], 77 + i, 'test', CONFIG, 0, f64, ints, blur, dropped)
        assert min(s.n_frames, 50) == int(f64[2].sum())
        ints['n_frames'] = s.n_frames          # 'test' mode never hands the uncropped track to a call that could be watched
        rows.append((f64, ints, blur, dropped, i, 77 + i))
    store('test', rows)
    # ---- data_paths order of a small folder tree (empty trajectory folders are enough for the constructor)
    tree = os.path.join(tmp, 'tree', 'syntheticdata')
    counts = []
    k = 0
    for tm in ['intermediate', 'final_win', 'final_lose', 'first_good', 'first_short', 'first_long']:
        for direction in ['left_to_right', 'right_to_left']:
            n = 3 + (5 * k) % 8
            k += 1
            counts.append(n)
            for j in range(n):
                os.makedirs(os.path.join(tree, tm, direction, 'trajectory_%04d' % j))
    paths.data_path = uplifting.helper.DATA_PATH = os.path.join(tmp, 'tree')
    out['paths/counts'] = np.array(counts, np.int32)
    for mode in ('train', 'test'):
        dps = D.TableTennisDataset(mode).data_paths
        out['paths/' + mode] = np.array([os.path.relpath(p, tree) for p in dps])
    # ---- raw MT19937 words of both streams
    out['stream/seeds'] = np.array(STREAM_SEEDS, np.int64)
    py_w, np_w = [], []
    for s in STREAM_SEEDS:
        random.seed(s)
        py_w.append([random.getrandbits(32) for _ in range(STREAM_WORDS)])
        np_w.append(np.random.RandomState(s)._bit_generator.random_raw(STREAM_WORDS))
    out['stream/py'], out['stream/np'] = np.array(py_w, np.uint32), np.array(np_w, np.uint32)
    for key in CONFIG:
        out['config/full/' + key] = np.float64(CONFIG[key])
        out['config/single/' + key] = np.float64(SINGLE[key])

    share = left_out / candidates
    print('candidates %d, left out on a knife edge %d (%.2f %%)' % (candidates, left_out, 100 * share))
    assert share <= 0.02
    print('reference CPU path: %.2f ms per sample (single core, full train pipeline, %d samples)' % (1e3 * t_ref / n_ref, n_ref))
    path = os.path.join(ROOT, 'tests', 'golden', 'dataset.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 1301004


if __name__ == '__main__':
    main()
