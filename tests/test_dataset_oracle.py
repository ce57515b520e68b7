"""Uplift training samples from generated trajectories, CPU side: the numpy restatement (tests/helpers/dataset_ref.py) and the
host build of the kernel's per-sample code (csrc/dataset_core.h through tests/helpers/host_dataset.cpp) against the fixture
the reference's own TableTennisDataset / transforms produced (tests/golden/dataset.npz, tools/make_goldens_dataset.py); the
host-side surface of upliftingtabletennis_amd.dataset."""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest

from conftest import has_gpu
from helpers import dataset_ref as R
from upliftingtabletennis_amd import dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ['full'] + ['single/' + n for n in R.TRANSFORM_NAMES] + ['test']
F64_RTOL = 1e-12          # restatement against the reference: same libm, differences only from operation order


def trajectories(g):
    """The fixture's 24 input trajectories as reference-format dictionaries."""
    off, pos, times = g['traj/offsets'], g['traj/positions'], g['traj/times']
    out = []
    for j in range(len(off) - 1):
        n = int(off[j + 1] - off[j])
        rot = np.zeros((n, 3))
        rot[0] = g['traj/rotation0'][j]
        out.append({'positions': pos[off[j]:off[j + 1]], 'times': times[:n], 'bounces': g['traj/bounces'][j, :g['traj/n_bounces'][j]],
                    'rotations': rot, 'Mext': g['traj/Mext'][None], 'Mint': g['traj/Mint'][None]})
    return out


def group_setup(g, group):
    """-> mode, config dict, transform mask of a fixture group."""
    if group == 'test':
        return 'test', None, 0
    kind = 'full' if group == 'full' else 'single'
    cfg = {k: float(g['config/%s/%s' % (kind, k)]) for k in ('blur_strength', 'randomize_std', 'stop_prob', 'randdet_prob', 'randmiss_prob', 'tablemiss_prob')}
    return 'train', cfg, R.ALL_ON if group == 'full' else 1 << R.TRANSFORM_NAMES.index(group.split('/')[1])


def test_the_fixture_holds_the_cases_the_issue_asks_for(golden):
    g = golden('dataset.npz')
    assert len(g['traj/offsets']) - 1 == 24
    assert len(g['full/seed']) >= 96 and int((g['full/camera_tries'] >= 2).sum()) >= 8
    for name in R.TRANSFORM_NAMES:
        assert len(g['single/%s/seed' % name]) == 24
    assert len(g['test/seed']) == 24
    assert g['stream/py'].shape[1] > 2 * 624 and g['stream/np'].shape[1] > 2 * 624          # crosses two regenerations
    assert g['full/dropped'].any() and (g['full/blur_idx'] >= 0).any() and (g['full/table_img'][:, :, 2] == 0).any()
    assert (g['full/mask'].sum(1) < np.minimum(g['full/n_frames'], 50) - g['full/dropped'].sum(1)).any()          # RandomStop cut something


@pytest.mark.parametrize('group', GROUPS)
def test_restatement_reproduces_the_reference(golden, group):
    g = golden('dataset.npz')
    trajs = trajectories(g)
    mode, cfg, enabled = group_setup(g, group)
    for c in range(len(g[group + '/seed'])):
        s = R.build_sample(trajs[int(g[group + '/traj'][c])], int(g[group + '/seed'][c]), mode, cfg, enabled)
        assert (s.fps, s.n_frames) == (g[group + '/fps'][c], g[group + '/n_frames'][c]), (group, c)
        assert (s.camera_tries, s.camera_success) == (g[group + '/camera_tries'][c], g[group + '/camera_success'][c]), (group, c)
        assert np.array_equal(s.mask, g[group + '/mask'][c]) and np.array_equal(s.table_img[:, 2], g[group + '/table_img'][c][:, 2])
        assert np.array_equal(s.blur_idx, g[group + '/blur_idx'][c]) and np.array_equal(s.dropped, g[group + '/dropped'][c])
        for name in R.OUTPUTS:
            ref = g['%s/%s' % (group, name)][c]
            assert np.abs(s[name] - ref).max() <= F64_RTOL * max(1.0, np.abs(ref).max()), (group, c, name)


def test_mt_models_match_the_recorded_streams(golden):
    g = golden('dataset.npz')
    for j, seed in enumerate(g['stream/seeds']):
        py, npr = R.PyRandom(int(seed)), R.NpRandom(int(seed))
        n = g['stream/py'].shape[1]
        assert [py.genrand_uint32() for _ in range(n)] == g['stream/py'][j].tolist()
        assert [npr.genrand_uint32() for _ in range(n)] == g['stream/np'][j].tolist()


@pytest.fixture(scope='module')
def host_dataset(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('hostdataset') / 'host_dataset.so')
    subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-Wno-unknown-pragmas', '-o', so,
                           os.path.join(ROOT, 'tests', 'helpers', 'host_dataset.cpp')])
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_kernel_source_on_the_host_draws_the_recorded_streams(host_dataset, golden):
    g = golden('dataset.npz')
    n = g['stream/py'].shape[1]
    for j, seed in enumerate(g['stream/seeds']):
        for which, key in ((0, 'stream/py'), (1, 'stream/np')):
            out = np.zeros(n, np.uint32)
            host_dataset.ttup_host_dataset_draws(ctypes.c_longlong(int(seed)), which, n, _p(out))
            assert np.array_equal(out, g[key][j]), (seed, key)


# csrc/dataset_core.h on the host: the reference's operations in the reference's order with glibc's sin / cos / log, where the
# fixture went through numpy's own loops and BLAS dot products.  Same bar as for the restatement, for the same reason (one libm
# family, differences from operation order and last-place roundings only); measured when written: 7.2e-16.
HOST_F64_BAR = F64_RTOL


@pytest.mark.parametrize('group', GROUPS)
def test_kernel_source_on_the_host_reproduces_the_reference(host_dataset, golden, group):
    """The per-sample code of the HIP kernel, compiled for the host: every integer / boolean output equals the reference's,
    the float64 outputs agree to HOST_F64_BAR."""
    g = golden('dataset.npz')
    mode, cfg, enabled = group_setup(g, group)
    n = len(g[group + '/seed'])
    rows = np.zeros((len(g['traj/positions']), 9))
    rows[:, :3] = g['traj/positions']
    rows[g['traj/offsets'][:-1], 6:9] = g['traj/rotation0']
    out = [np.zeros((n,) + shape) for _, shape in dataset.OUTPUTS]
    ptrs = (ctypes.c_void_p * 9)(*[a.ctypes.data for a in out])
    diag, record = np.zeros((n, 4), np.int32), np.zeros((n, 3, 50), np.int32)
    strengths = np.array([cfg[k] for k in ('blur_strength', 'randomize_std', 'stop_prob', 'randdet_prob', 'randmiss_prob', 'tablemiss_prob')] if cfg else [0.0] * 6)
    host_dataset.ttup_host_dataset_build(
        _p(rows), _p(np.ascontiguousarray(g['traj/offsets'])), ctypes.c_longlong(len(rows)), 24, _p(np.ascontiguousarray(g['traj/bounces'])),
        _p(np.ascontiguousarray(g['traj/n_bounces'])), _p(np.ascontiguousarray(g['traj/times'])), len(g['traj/times']),
        _p(np.ascontiguousarray(g['traj/Mext'])), _p(np.ascontiguousarray(g['traj/Mint'])), _p(np.ascontiguousarray(g[group + '/traj'])),
        _p(np.ascontiguousarray(g[group + '/seed'])), n, 0 if mode == 'train' else 1, _p(strengths), enabled | 64, ptrs, _p(diag), _p(record))
    worst = check_against_fixture(g, group, dict(zip([k for k, _ in dataset.OUTPUTS], out)), diag, record, HOST_F64_BAR)
    print('\n%s: host build, worst float64 deviation %.3e' % (group, worst))


def check_against_fixture(g, group, f64, diag, record, bar):
    """Integer / boolean outputs exactly, float64 outputs within `bar` relative to max(1, |ref|) per tensor.  Returns the largest
    deviation seen (printed before the assertion)."""
    train = group != 'test'
    assert np.array_equal(diag[:, 0], g[group + '/fps']) and np.array_equal(diag[:, 1], g[group + '/n_frames'])
    if train:
        assert np.array_equal(diag[:, 2], g[group + '/camera_tries']) and np.array_equal(diag[:, 3], g[group + '/camera_success'])
    assert np.array_equal(f64['mask'], g[group + '/mask'])
    assert np.array_equal(f64['table_img'][:, :, 2], g[group + '/table_img'][:, :, 2])
    assert np.array_equal(record[:, 1], g[group + '/blur_idx']) and np.array_equal(record[:, 2] != 0, g[group + '/dropped'])
    worst = 0.0
    for name, _ in dataset.OUTPUTS:
        ref = g['%s/%s' % (group, name)]
        dev = np.abs(f64[name] - ref).reshape(len(ref), -1).max(1) / np.maximum(1.0, np.abs(ref).reshape(len(ref), -1).max(1))
        print('%s %s: max deviation %.3e' % (group, name, dev.max()))
        worst = max(worst, float(dev.max()))
    assert worst <= bar, (group, worst)
    return worst


def test_data_paths_order_equals_the_reference(golden, tmp_path):
    g = golden('dataset.npz')
    k = 0
    for tm in dataset.TRAJECTORY_MODES:
        for direction in dataset.DIRECTIONS:
            for j in range(int(g['paths/counts'][k])):
                os.makedirs(tmp_path / tm / direction / ('trajectory_%04d' % j))
            k += 1
    for mode in ('train', 'test'):
        got = [os.path.relpath(p, tmp_path) for p in dataset.list_data_paths(str(tmp_path), mode)]
        assert got == [str(p) for p in g['paths/' + mode]]
        counts = {(tm, d): int(g['paths/counts'][i * 2 + j]) for i, tm in enumerate(dataset.TRAJECTORY_MODES) for j, d in enumerate(dataset.DIRECTIONS)}
        assert got == [os.path.join(tm, d, 'trajectory_%04d' % i) for tm, d, i in R.data_paths(counts, mode)]
    with pytest.raises(AttributeError):
        dataset.list_data_paths(str(tmp_path), 'val')          # data.py:42
    with pytest.raises(ValueError):
        dataset.list_data_paths(str(tmp_path), 'training')


def test_get_transforms_raises_what_the_reference_raises():
    cfg = types.SimpleNamespace(blur_strength=0.4, randomize_std=8, stop_prob=0.5, randdet_prob=0.05, randmiss_prob=0.05, tablemiss_prob=0.05)
    tf = dataset.get_transforms(cfg, 'train')
    assert [type(t).__name__ for t in tf.transforms] == R.TRANSFORM_NAMES + ['NormalizeImgCoords']
    assert dataset.transform_plan(tf) == (127, [0.4, 8.0, 0.5, 0.05, 0.05, 0.05])
    assert dataset.transform_plan(dataset.get_transforms(cfg, 'test')) == (64, [0.0] * 6)
    assert dataset.transform_plan(None) == (0, [0.0] * 6)
    for bad in (0.5, 0.05, 0.7):          # 0.5 is the reference's own TrainConfig default
        cfg.blur_strength = bad
        with pytest.raises(AssertionError):
            dataset.get_transforms(cfg, 'train')
    cfg.blur_strength = 0
    dataset.get_transforms(cfg, 'train')
    swapped = dataset.Compose([dataset.RandomStop(0.5), dataset.RandomizeDetections(3), dataset.NormalizeImgCoords()])
    with pytest.raises(NotImplementedError):
        dataset.transform_plan(swapped)
    only = dataset.Compose([dataset.Identity(), dataset.RandomizeDetections(3), dataset.Identity(), dataset.NormalizeImgCoords()])
    assert dataset.transform_plan(only) == (2 | 64, [0.0, 3.0, 0.0, 0.0, 0.0, 0.0])


def test_no_cpu_fallback(golden):
    if has_gpu():
        pytest.skip('GPU present')
    with pytest.raises(RuntimeError):
        dataset.TableTennisDataset('train', None, trajectories=trajectories(golden('dataset.npz')))
