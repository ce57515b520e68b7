"""Uplift training samples from generated trajectories on the MI355X, through the C-ABI, against the fixture the reference's own
TableTennisDataset / transforms produced (tests/golden/dataset.npz).  The reference is never read here."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import has_gpu
from test_dataset_oracle import GROUPS, check_against_fixture, group_setup, trajectories

pytestmark = pytest.mark.gpu
if has_gpu():
    from upliftingtabletennis_amd import _lib, dataset, trajgen, uplift, weights

# float64 outputs against the reference's fixture, relative to max(1, |ref|) per tensor.  Largest deviation measured on the first
# MI355X run: MEASURED (the device's sin / cos / log against numpy's); bar = 2 x measured.
MEASURED = 7.22e-16
F64_BAR = 2 * MEASURED
ULPS = 2          # float32 outputs: the fp64 chain deviates far less than one float32 ulp, only the final rounding can flip


def make_dataset(g, group):
    mode, cfg, enabled = group_setup(g, group)
    if mode == 'test':
        tf = dataset.Compose([dataset.NormalizeImgCoords()])
    else:
        mk = [lambda: dataset.MotionBlur(cfg['blur_strength']), lambda: dataset.RandomizeDetections(cfg['randomize_std']),
              lambda: dataset.RandomStop(cfg['stop_prob']), lambda: dataset.RandomDetection(cfg['randdet_prob']),
              lambda: dataset.RandomMissing(cfg['randmiss_prob']), lambda: dataset.TableMissing(cfg['tablemiss_prob'])]
        tf = dataset.Compose([mk[k]() if enabled >> k & 1 else dataset.Identity() for k in range(6)] + [dataset.NormalizeImgCoords()])
    return dataset.TableTennisDataset(mode, tf, trajectories=trajectories(g))


def within_ulps(got, ref32, ulps):
    got, ref32 = np.asarray(got, np.float32), np.asarray(ref32, np.float32)
    return np.abs(got.astype(np.float64) - ref32.astype(np.float64)) <= ulps * np.spacing(np.maximum(np.abs(got), np.abs(ref32))).astype(np.float64)


def test_device_streams_equal_the_recorded_words(golden):
    """Both MT19937 streams word for word over 1500 draws: two passes over the 624-word state and into a third."""
    g = golden('dataset.npz')
    lib = _lib.load()
    seeds = np.ascontiguousarray(g['stream/seeds'])
    n, count = len(seeds), g['stream/py'].shape[1]
    ws_bytes = lib.ttup_dataset_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    for which, key in ((0, 'stream/py'), (1, 'stream/np')):
        out = torch.zeros((n, count), dtype=torch.int32, device='cuda')
        _lib.check(lib.ttup_dataset_seed(seeds.ctypes.data_as(ctypes.c_void_p), n, _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))
        _lib.check(lib.ttup_dataset_draws(_lib.ptr(ws), ws_bytes, n, which, count, _lib.ptr(out), _lib.stream_ptr()))
        assert np.array_equal(out.cpu().numpy().view(np.uint32), g[key]), key


@pytest.mark.parametrize('group', GROUPS)
def test_samples_match_the_reference(golden, group):
    """Full pipeline, each transform alone, 'test' mode: integer / boolean outputs exactly, float32 within 2 ulps, float64
    within 2 x the measured deviation."""
    g = golden('dataset.npz')
    ds = make_dataset(g, group)
    b = ds.batch(g[group + '/traj'], g[group + '/seed'], want_float64=True, want_record=True)
    f64 = {k: v.cpu().numpy() for k, v in b.float64.items()}
    diag = np.stack([t.cpu().numpy() for t in (b.fps, b.n_frames, b.camera_tries, b.camera_success)], 1)
    if group == 'full':
        assert int((diag[:, 2] >= 2).sum()) >= 8
    worst = check_against_fixture(g, group, f64, diag, b.record.cpu().numpy(), F64_BAR)
    print('%s: device, worst float64 deviation %.3e (bar %.3e)' % (group, worst, F64_BAR))
    for name, _ in dataset.OUTPUTS:
        got, ref = getattr(b, name).cpu().numpy(), g['%s/%s' % (group, name)].astype(np.float32)
        ok = within_ulps(got, ref, ULPS)
        print('%s %s: float32 values off by more than 0 ulp: %d, more than %d ulps: %d' % (group, name, int((got != ref).sum()), ULPS, int((~ok).sum())))
        assert ok.all(), (group, name)
        assert got.dtype == np.float32 and np.array_equal(got, f64[name].astype(np.float32))          # the cast is the last step


def test_item_equals_batch_row_and_launch_split_does_not_matter(golden, monkeypatch):
    g = golden('dataset.npz')
    ds = make_dataset(g, 'full')
    idx, seeds = g['full/traj'], g['full/seed']
    whole = ds.batch(idx, seeds)
    monkeypatch.setattr(dataset, 'MAX_LAUNCH', 7)
    split = ds.batch(idx, seeds)
    part = ds.batch(idx[40:50][::-1], seeds[40:50][::-1])
    for name, _ in dataset.OUTPUTS:
        assert torch.equal(getattr(whole, name), getattr(split, name)), name
        assert torch.equal(getattr(whole, name)[40:50].flip(0), getattr(part, name)), name
    assert torch.equal(whole.camera_tries, split.camera_tries)
    monkeypatch.undo()
    ds2 = dataset.TableTennisDataset('train', ds.transforms, trajectories=trajectories(g), seed=1000)
    ds2.set_epoch(2)
    rows = ds2.batch(np.arange(len(ds2)))
    ref = ds2.batch(np.arange(len(ds2)), 1000 + 2 * len(ds2) + np.arange(len(ds2)))
    for i in (0, 5, len(ds2) - 1):
        item = ds2[i]
        assert len(item) == 9 and [tuple(t.shape) for t in item] == [s for _, s in dataset.OUTPUTS]
        for t, (name, _) in zip(item, dataset.OUTPUTS):
            assert torch.equal(t, getattr(rows, name)[i]) and torch.equal(t, getattr(ref, name)[i]), name
    with pytest.raises(IndexError):
        ds2[len(ds2)]


def test_generator_to_samples_to_uplift_on_the_device(golden):
    """trajgen -> ds.batch -> uplift forward on device tensors end to end; and the forward fed with device-built samples of the
    fixture's (trajectory, seed) pairs gives the (rot, pos) of the forward fed with the fixture's samples, within the uplift's
    1e-4 relative bar."""
    g = golden('dataset.npz')
    net = uplift.get_model('connectstage', 'large', 'dynamic', 'new', state_dict=weights.random_uplift_state_dict(7, 'large'), max_batch=128, max_len=64)
    ds = make_dataset(g, 'full')
    b = ds.batch(g['full/traj'], g['full/seed'])
    rot, pos = net(*b.model_inputs())
    fix = [torch.from_numpy(g['full/' + k].astype(np.float32)).cuda() for k in ('r_img', 'table_img', 'mask', 'times')]
    rot_f, pos_f = net(*fix)
    e_rot = float((rot - rot_f).abs().max() / rot_f.abs().max())
    e_pos = float((pos - pos_f).abs().max() / pos_f.abs().max())
    print('forward on device samples against forward on fixture samples: rot %.3e pos %.3e' % (e_rot, e_pos))
    assert e_rot <= 1e-4 and e_pos <= 1e-4
    tr = trajgen.get_valid_trajectories(96, 16, 'intermediate', 'left_to_right', as_numpy=False)
    assert torch.is_tensor(tr.stacked()['rows']) and tr.stacked()['rows'].is_cuda
    chain = dataset.TableTennisDataset('train', ds.transforms, trajectories=tr, seed=3)
    assert len(chain) == 96
    sb = chain.batch(np.arange(96))
    assert all(t.is_cuda for t in sb.model_inputs()) and sb.mask.min() == 0
    assert bool((sb.fps >= 20).all()) and bool((sb.fps <= 65).all()) and bool((sb.camera_tries >= 1).all())
    first = tr[0]
    one = dataset.TableTennisDataset('train', ds.transforms, trajectories=[{k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in first.items()}], seed=3)
    for t, u in zip(one[0], chain[0]):
        assert torch.equal(t, u)          # the stacked device rows and the reference-format dictionary are the same input
    rot, pos = net(*sb.model_inputs())
    assert rot.shape == (96, 3) and pos.shape == (96, 50, 3) and bool(torch.isfinite(rot).all()) and bool(torch.isfinite(pos).all())


def test_bad_arguments_are_refused_before_anything_is_launched(golden):
    g = golden('dataset.npz')
    ds = make_dataset(g, 'full')
    lib = _lib.load()
    vp = ctypes.c_void_p
    n = 4
    out = [torch.zeros((n,) + s, dtype=torch.float32, device='cuda') for _, s in dataset.OUTPUTS]
    diag = torch.full((n, 4), -7, dtype=torch.int32, device='cuda')
    ws_bytes = lib.ttup_dataset_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')

    def build(mode=0, strengths=(0.4, 8, 0.5, 0.05, 0.05, 0.05), index=(0, 1, 2, 3), ws_bytes=ws_bytes, mask=127):
        idx = np.array(index, np.int64)
        return lib.ttup_dataset_build(_lib.ptr(ds._rows), _lib.ptr(ds._offsets), int(ds._rows.shape[0]), len(ds), _lib.ptr(ds._bounces), _lib.ptr(ds._n_bounces),
                                      _lib.ptr(ds._times), int(ds._times.numel()), _lib.ptr(ds._mext), _lib.ptr(ds._mint), 1, idx.ctypes.data_as(vp), n, mode,
                                      (ctypes.c_double * 6)(*strengths), mask, (vp * 9)(*[t.data_ptr() for t in out]), None, _lib.ptr(diag), None,
                                      _lib.ptr(ws), ws_bytes, _lib.stream_ptr())
    seeds = np.arange(n, dtype=np.int64)
    assert lib.ttup_dataset_seed(seeds.ctypes.data_as(vp), n, _lib.ptr(ws), ws_bytes, _lib.stream_ptr()) == _lib.OK
    assert build(mode=2) == _lib.EINVAL and b'mode' in lib.ttup_last_error()
    assert build(strengths=(0.4, 8, 1.5, 0.05, 0.05, 0.05)) == _lib.EINVAL and b'probability' in lib.ttup_last_error()
    assert build(strengths=(0.4, 8, 0.5, -0.1, 0.05, 0.05)) == _lib.EINVAL
    assert build(strengths=(0.5, 8, 0.5, 0.05, 0.05, 0.05)) == _lib.EINVAL and b'blur_strength' in lib.ttup_last_error()
    assert build(index=(0, 1, 2, 24)) == _lib.EINVAL and b'out of range' in lib.ttup_last_error()
    assert build(index=(0, -1, 2, 3)) == _lib.EINVAL
    assert build(ws_bytes=ws_bytes - 1) == _lib.EINVAL and b'workspace' in lib.ttup_last_error()
    assert build(mask=128) == _lib.EINVAL
    assert lib.ttup_dataset_seed(seeds.ctypes.data_as(vp), n, _lib.ptr(ws), ws_bytes - 1, _lib.stream_ptr()) == _lib.EINVAL
    big = np.array([0, 1, 2, 2 ** 32], np.int64)
    assert lib.ttup_dataset_seed(big.ctypes.data_as(vp), n, _lib.ptr(ws), ws_bytes, _lib.stream_ptr()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert bool((diag == -7).all())          # nothing ran
    assert build() == _lib.OK
    torch.cuda.synchronize()
    assert bool((diag[:, 0] >= 20).all())
    with pytest.raises(ValueError):
        ds.batch([0, 99])
