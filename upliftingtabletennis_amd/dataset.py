"""Uplift training samples from generated trajectories on the MI355X: mirror of uplifting/data.py::TableTennisDataset and of
uplifting/transformations.py::get_transforms -- the names, the argument meaning and the 9-tuple
(r_img, table_img, mask, r_world, rotation, times, bounces, Mint, Mext) are the reference's.  A sample is built by one device lane
through the C-ABI (`ttup_dataset_seed`, `ttup_dataset_build`): frame rate, resampling, `sample_camera`, mask / padding, the train
transforms, the float32 cast.  No CPU fallback.

Seed convention (the reference has none: its two random streams are process-global).  A sample with seed `s` is what the
reference returns for `random.seed(s); np.random.seed(s); dataset[i]`; `ds[i]` uses `s = seed + epoch * len(ds) + i`
(`ds.set_epoch(e)`), `ds.batch(indices, seeds)` takes explicit seeds.  `0 <= s < 2**32` (np.random.seed's range).

Deviations: tensors stay on the device; a MotionBlur window that holds no stored sample leaves its frame as it is (the
reference's `np.random.choice` raises there; with blur_strength >= 0.1 and the generator's 2 ms samples this needs fps 65 and
strength < 0.13 on the last frame).
"""
import ctypes
import os
import random

import numpy as np
import torch

from . import _lib, trajgen

HEIGHT, WIDTH = 1440, 2560
SEQUENCE_LEN = 50
TRAJECTORY_MODES = ['intermediate', 'final_win', 'final_lose', 'first_good', 'first_short', 'first_long']      # data.py:29
DIRECTIONS = ['left_to_right', 'right_to_left']
OUTPUTS = [('r_img', (SEQUENCE_LEN, 2)), ('table_img', (13, 3)), ('mask', (SEQUENCE_LEN,)), ('r_world', (SEQUENCE_LEN, 3)), ('rotation', (3,)),
           ('times', (SEQUENCE_LEN,)), ('bounces', (1,)), ('Mint', (3, 3)), ('Mext', (4, 4))]
MAX_LAUNCH = 65536          # samples per launch: 5 KB of generator state each


# ---------------------------------------------------------------------------------------------------- transforms
class _Transform:
    def __call__(self, data):
        raise NotImplementedError('the transforms run inside the sample kernel; hand them to TableTennisDataset')


class MotionBlur(_Transform):
    def __init__(self, blur_strength=0.5):
        self.blur_strength = blur_strength
        assert 0.1 <= blur_strength < 0.5 or blur_strength == 0, 'blur_strength should be in the range [0.1, 0.5) or 0.'


class RandomizeDetections(_Transform):
    def __init__(self, std=5):
        self.std = std


class RandomStop(_Transform):
    def __init__(self, stop_prob=0.5):
        self.stop_prob = stop_prob


class RandomDetection(_Transform):
    def __init__(self, randdet_prob):
        self.randdet_prob = randdet_prob


class RandomMissing(_Transform):
    def __init__(self, randmiss_prob):
        self.randmiss_prob = randmiss_prob


class TableMissing(_Transform):
    def __init__(self, tablemiss_prob):
        self.tablemiss_prob = tablemiss_prob


class Identity(_Transform):
    pass


class NormalizeImgCoords(_Transform):
    pass


class Compose(_Transform):
    def __init__(self, transforms):
        self.transforms = transforms


_ORDER = [(MotionBlur, 'blur_strength'), (RandomizeDetections, 'std'), (RandomStop, 'stop_prob'), (RandomDetection, 'randdet_prob'),
          (RandomMissing, 'randmiss_prob'), (TableMissing, 'tablemiss_prob'), (NormalizeImgCoords, None)]


def get_transforms(config, mode='train'):
    """`get_transforms` (transformations.py:286-300).  `config` carries blur_strength, randomize_std, stop_prob, randdet_prob,
    randmiss_prob, tablemiss_prob.  Raises the reference's AssertionError for a blur_strength outside [0.1, 0.5) or 0 -- which
    the reference's own TrainConfig default of 0.5 trips, there as here."""
    transforms = []
    if mode == 'train':
        transforms.append(MotionBlur(config.blur_strength))
        transforms.append(RandomizeDetections(config.randomize_std))
        transforms.append(RandomStop(config.stop_prob))
        transforms.append(RandomDetection(config.randdet_prob))
        transforms.append(RandomMissing(config.randmiss_prob))
        transforms.append(TableMissing(config.tablemiss_prob))
    transforms.append(NormalizeImgCoords())
    return Compose(transforms)


def transform_plan(transforms):
    """-> (mask, strengths[6]) for the kernel.  The kernel runs the transforms in the order of `get_transforms`; any of them may be
    missing or an `Identity`, another order raises NotImplementedError."""
    if transforms is None:
        return 0, [0.0] * 6
    items = transforms.transforms if isinstance(transforms, Compose) else list(transforms)
    mask, strengths, at = 0, [0.0] * 6, 0
    for t in items:
        if isinstance(t, Identity):
            continue
        k = next((k for k in range(at, len(_ORDER)) if type(t) is _ORDER[k][0]), None)
        if k is None:
            raise NotImplementedError('transforms must keep the order of get_transforms (MotionBlur, RandomizeDetections, RandomStop, '
                                      'RandomDetection, RandomMissing, TableMissing, NormalizeImgCoords); got %s' % type(t).__name__)
        mask |= 1 << k
        if k < 6:
            strengths[k] = float(getattr(t, _ORDER[k][1]))
        at = k + 1
    return mask, strengths


# ---------------------------------------------------------------------------------------------------- data_paths
def list_data_paths(path, mode):
    """`data_paths` of the reference's constructor (data.py:28-50) for a folder tree <path>/<trajectory mode>/<direction>/
    trajectory_%04d: 70 % / 10 % / 20 % of every (mode, direction) block for train / val / test, and the reference's shuffle of the
    list accumulated so far with a fresh random.Random(0) before every block.  'val' raises what the reference raises."""
    data_paths = []
    holder = type('_Partial', (), {})()          # stands for the half-built dataset object of the reference's constructor
    for tm in TRAJECTORY_MODES:
        for direction in DIRECTIONS:
            folder = os.path.join(path, tm, direction)
            dps = sorted(os.path.join(folder, 'trajectory_%04d' % i) for i, _ in enumerate(os.listdir(folder)))
            random.Random(0).shuffle(data_paths)
            if mode == 'train':
                dps = dps[:int(0.7 * len(dps))]
            elif mode == 'val':
                dps = dps[int(0.7 * len(dps)):int(0.8 * len(dps))]
                holder.data_paths.pop(0)          # data.py:42: AttributeError, the attribute is assigned after the loop
            elif mode == 'test':
                dps = dps[int(0.8 * len(dps)):]
            else:
                raise ValueError('Unknown mode %s' % mode)
            data_paths.extend(dps)
    return data_paths


class SampleBatch:
    """Stacked device tensors of `n` samples: the nine outputs (float32) and the diagnostics fps, n_frames (before the crop to
    50), camera_tries, camera_success (int32).  `batch[i]` is the reference's 9-tuple of sample i."""

    def __init__(self, tensors, diag, float64=None, record=None):
        for (name, _), t in zip(OUTPUTS, tensors):
            setattr(self, name, t)
        self.fps, self.n_frames, self.camera_tries, self.camera_success = diag.unbind(1)
        self.float64, self.record = float64, record

    def __len__(self):
        return int(self.mask.shape[0])

    def __getitem__(self, i):
        return tuple(getattr(self, name)[i] for name, _ in OUTPUTS)

    def model_inputs(self):
        """(r_img, table_img, mask, times) for the uplift forward.  The mask goes on unchanged: a track of >= 50 frames has the
        reference's all-ones mask."""
        return self.r_img, self.table_img, self.mask, self.times


class TableTennisDataset:
    """`TableTennisDataset(mode, transforms)` (data.py:24-166).  Input: `trajectories` = a `trajgen.TrajectoryBatch` or a list of
    reference-format dictionaries (all of them are used, in their order), or `path` = a folder tree in the `save_dataset` layout
    (<path>/<trajectory mode>/<direction>/trajectory_%04d), cut and ordered as the reference does (`list_data_paths`)."""

    def __init__(self, mode='train', transforms=None, *, trajectories=None, path=None, seed=0, device=None):
        _lib.require_gpu()
        if mode == 'val' and path is None:
            raise AttributeError("'TableTennisDataset' object has no attribute 'data_paths'")          # data.py:42
        if mode not in ('train', 'val', 'test'):
            raise ValueError('Unknown mode %s' % mode)
        if (trajectories is None) == (path is None):
            raise ValueError('give either trajectories or path')
        self.mode, self.transforms, self.seed, self.epoch = mode, transforms, int(seed), 0
        self.device = torch.device(device if device is not None else 'cuda')
        self._mask, self._strengths = transform_plan(transforms)
        self.data_paths = None
        if path is not None:
            self.data_paths = list_data_paths(path, mode)
            trajectories = [{k: np.load(os.path.join(p, k + '.npy')) for k in ('positions', 'times', 'bounces', 'rotations', 'Mint', 'Mext')}
                            for p in self.data_paths]
        dev = self.device
        if isinstance(trajectories, trajgen.TrajectoryBatch):
            st = trajectories.stacked()
            rows, offsets, bounces, n_bounces = st['rows'], st['offsets'], st['bounces'], st['n_bounces']
            times, mext, mint = trajectories.times, trajectories.Mext[None], trajectories.Mint[None]
        else:
            trajectories = list(trajectories)
            if not trajectories:
                raise ValueError('no trajectories')
            nk = [len(t['times']) for t in trajectories]
            rows = np.zeros((sum(nk), 9))
            offsets = np.concatenate([[0], np.cumsum(nk)]).astype(np.int64)
            bounces, n_bounces = np.zeros((len(nk), 4)), np.zeros(len(nk), np.int32)
            times = np.asarray(trajectories[int(np.argmax(nk))]['times'], np.float64)
            for j, t in enumerate(trajectories):
                o = int(offsets[j])
                rows[o:o + nk[j], 0:3] = np.asarray(t['positions'])
                rows[o, 6:9] = np.asarray(t['rotations'])[0]
                b = np.asarray(t['bounces'], np.float64).reshape(-1)[:4]
                bounces[j, :len(b)], n_bounces[j] = b, len(b)
                if not np.array_equal(np.asarray(t['times']), times[:nk[j]]):
                    raise ValueError('trajectory %d does not carry the shared time labels of the generator' % j)
            mext = np.stack([np.asarray(t['Mext'], np.float64).reshape(-1, 4, 4)[0] for t in trajectories])
            mint = np.stack([np.asarray(t['Mint'], np.float64).reshape(-1, 3, 3)[0] for t in trajectories])
        def f64(a):          # (read-only numpy views, e.g. the batch's shared time labels, are copied before torch sees them)
            return torch.as_tensor(a if torch.is_tensor(a) else np.array(a, dtype=np.float64), dtype=torch.float64).to(dev).contiguous()
        self._rows, self._bounces, self._times = f64(rows), f64(bounces), f64(np.asarray(times))
        self._offsets = torch.as_tensor(np.asarray(offsets), dtype=torch.int64).to(dev)
        self._n_bounces = torch.as_tensor(np.asarray(n_bounces), dtype=torch.int32).to(dev)
        self._mext, self._mint = f64(np.asarray(mext)), f64(np.asarray(mint))
        self._cam_per_traj = int(self._mext.shape[0] > 1)
        self.length = int(self._offsets.numel()) - 1

    def __len__(self):
        return self.length

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __getitem__(self, idx):
        if not -self.length <= idx < self.length:
            raise IndexError('list index out of range')          # data_paths[idx]
        return self.batch([idx % self.length])[0]

    def batch(self, indices, seeds=None, want_float64=False, want_record=False):
        """All samples of `indices` in one launch (per 65 536).  seeds: one per index (default seed + epoch * len + index).
        want_float64 / want_record (tests): the outputs before the float32 cast as `.float64` (a dict), the per-frame integer
        record (nearest stored sample, blur sample, dropped) as `.record` (n, 3, 50)."""
        lib = _lib.load()
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
        sd = idx + self.seed + self.epoch * self.length if seeds is None else np.ascontiguousarray(np.asarray(seeds, dtype=np.int64).reshape(-1))
        if sd.shape != idx.shape:
            raise ValueError('one seed per index')
        n, dev = int(idx.size), self.device
        out32 = [torch.zeros((n,) + shape, dtype=torch.float32, device=dev) for _, shape in OUTPUTS]
        out64 = [torch.zeros((n,) + shape, dtype=torch.float64, device=dev) for _, shape in OUTPUTS] if want_float64 else None
        diag = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        record = torch.zeros((n, 3, SEQUENCE_LEN), dtype=torch.int32, device=dev) if want_record else None
        strengths = (ctypes.c_double * 6)(*self._strengths)
        vp = ctypes.c_void_p
        with torch.cuda.device(dev):
            ws_bytes = lib.ttup_dataset_workspace_bytes(min(n, MAX_LAUNCH))
            ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
            for a in range(0, n, MAX_LAUNCH):
                m = min(MAX_LAUNCH, n - a)
                p32 = (vp * 9)(*[t[a:].data_ptr() for t in out32])
                p64 = (vp * 9)(*[t[a:].data_ptr() for t in out64]) if want_float64 else None
                _lib.check(lib.ttup_dataset_seed(sd[a:].ctypes.data_as(vp), m, _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))
                _lib.check(lib.ttup_dataset_build(
                    _lib.ptr(self._rows), _lib.ptr(self._offsets), int(self._rows.shape[0]), self.length, _lib.ptr(self._bounces), _lib.ptr(self._n_bounces),
                    _lib.ptr(self._times), int(self._times.numel()), _lib.ptr(self._mext), _lib.ptr(self._mint), self._cam_per_traj,
                    idx[a:].ctypes.data_as(vp), m, 0 if self.mode == 'train' else 1, strengths, self._mask, p32, p64,
                    _lib.ptr(diag[a:]), _lib.ptr(record[a:]) if want_record else None, _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))
        return SampleBatch(out32, diag, dict(zip([k for k, _ in OUTPUTS], out64)) if want_float64 else None, record)
