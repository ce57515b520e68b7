"""f4: the device camera calibration (csrc/calib.hip) at the edges of its C-ABI: the DLT start it returns through `start_dev`
against the numpy oracle's, subset counts other than 100 (the C-ABI takes 1..128), cameras in a batch against the same camera
alone, the status codes, and visibility sets on which the DLT is degenerate.  A test-local helper calls `ttup_calib_forward`
itself (the pattern of `calib.calibrate_cameras`) with a chosen subset count and a `start_dev` buffer and returns the status
un-raised.  /root/reference is never read.

Cameras are `synth._random_camera(default_rng(seed))` projecting `synth.TABLE_POINTS`, as test_calib_gpu.py builds its planted one.
Measured on an MI355X: the device's DLT start (12x12 Jacobi on the normal matrix, its own RQ split) differs from the oracle's
(LAPACK SVD, scipy rq) by 1.3e-12 at worst, in units of max(|ref|, 1), over 8 cameras x {0, 1 px} noise x three visibility sets
(bar 1e-9)."""
import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu
from oracle import calib_ref

pytestmark = pytest.mark.gpu
if has_gpu():
    from upliftingtabletennis_amd import _lib, calib, synth

SIX = [0, 3, 5, 9, 10, 11]
SENTINEL = -7.0


def _keypoints(seed, noise=0.0, visible=None):
    """(13,3) keypoints [x, y, visibility] of a seeded random camera, with seeded Gaussian pixel noise."""
    R, c, f = synth._random_camera(np.random.default_rng(seed))
    Mext = np.eye(4); Mext[:3, :3] = R; Mext[:3, 3] = -R @ c
    Mint = np.array([[f, 0, 960.0, 0], [0, f, 540.0, 0], [0, 0, 1, 0]])
    xy = calib.reproject(synth.TABLE_POINTS, Mint, Mext) + noise * np.random.default_rng(1000 + seed).normal(0, 1.0, (13, 2))
    vis = np.zeros(13)
    vis[list(range(13)) if visible is None else visible] = 1.0
    return np.concatenate([xy, vis[:, None]], axis=1)


def _subsets(kp, n):
    """The wrapper's subsets for one camera, (n,4) int32: the reference's first min(n, 100) draws; subsets 100.. repeat subset 0.
    A camera the kernel refuses before it reads its subsets (fewer than 6 visible keypoints) gets zeros (no key)."""
    vis = [k + 1 for k in range(13) if kp[k, 2] == 1]
    if len(vis) < 6:
        return np.zeros((n, 4), np.int32)
    sub = calib.ransac_subsets(vis, min(n, 100))
    return np.concatenate([sub, np.tile(sub[:1], (n - len(sub), 1))]) if n > len(sub) else sub


def _forward(kps, subsets=None, n_subsets=100, max_iter=300, want_start=True):
    """ttup_calib_forward itself -> dict(rc, mint, mext, n_inliers, status, start) of host arrays.  The outputs are pre-filled
    so that whatever the library did not write can be told apart."""
    lib = _lib.load()
    kp = np.ascontiguousarray(np.asarray(kps, np.float64))
    b = len(kp)
    if subsets is None:
        subsets = np.stack([_subsets(kp[i], max(n_subsets, 1)) for i in range(b)])
    dev = torch.device('cuda')
    kpt, sub = torch.from_numpy(kp).to(dev), torch.from_numpy(np.ascontiguousarray(subsets, np.int32)).to(dev)
    mint = torch.full((b, 3, 4), SENTINEL, dtype=torch.float64, device=dev)
    mext = torch.full((b, 4, 4), SENTINEL, dtype=torch.float64, device=dev)
    start = torch.full((b, 8), SENTINEL, dtype=torch.float64, device=dev) if want_start else None
    ninl = torch.full((b,), -7, dtype=torch.int32, device=dev)
    status = torch.full((b,), -7, dtype=torch.int32, device=dev)
    rc = lib.ttup_calib_forward(_lib.ptr(kpt), _lib.ptr(sub), b, int(n_subsets), calib.WIDTH, calib.HEIGHT, int(max_iter),
                                _lib.ptr(mint), _lib.ptr(mext), _lib.ptr(ninl), _lib.ptr(status), _lib.ptr(start), _lib.stream_ptr())
    torch.cuda.synchronize()
    return {'rc': rc, 'mint': mint.cpu().numpy(), 'mext': mext.cpu().numpy(), 'n_inliers': ninl.cpu().numpy(), 'status': status.cpu().numpy(),
            'start': start.cpu().numpy() if want_start else None}


def _same_camera(a, i, b, j, what):
    for k in ('mint', 'mext', 'n_inliers', 'start', 'status'):
        assert np.array_equal(a[k][i], b[k][j]), (what, k, i, j, a[k][i], b[k][j])


def _oracle_start(kp):
    """The reference's start for its refinements: `dlt_calib` on the visible keypoints, turned into (fx, fy, tx, ty, tz, euler xyz
    wrapped to [-pi, pi)) exactly as `calib_ref.regress_cameramatrices` forms x0."""
    from scipy.spatial.transform import Rotation
    vis = kp[:, 2] == 1
    Mint, Mext = calib_ref.dlt_calib(calib_ref.TABLE_POINTS[vis], kp[vis, :2])
    try:
        angles = Rotation.from_matrix(Mext[:3, :3]).as_euler('xyz', degrees=False)
    except ValueError:
        angles = np.array([0, 0, 0])
    x0 = np.array([Mint[0, 0], Mint[1, 1], Mext[0, 3], Mext[1, 3], Mext[2, 3], angles[0], angles[1], angles[2]])
    x0[5:] = np.mod((x0[5:] + np.pi), (2 * np.pi)) - np.pi
    return x0


@functools.lru_cache(maxsize=None)
def _five():
    """Five different noisy cameras (one with an invisible keypoint), each alone and all in one batch: shared, never modified."""
    kps = np.stack([_keypoints(20 + i, noise=1.0, visible=[k for k in range(13) if k != 5] if i == 2 else None) for i in range(5)])
    return kps, _forward(kps), [_forward(kps[i:i + 1]) for i in range(5)]


# ---------------------------------------------------------------------------------------------- B1
def test_dlt_start_matches_the_numpy_oracle():
    """Bar |dev - ref| <= 1e-9 max(|ref|, 1), angles modulo 2 pi.  Basis: the oracle's SVD route and a normal-matrix eigenvector
    route (what the kernel does) differ by at most 3.9e-12 on the CPU over 40 cameras x these sets x both noise levels; 1e-9
    leaves a factor of about 250 for Jacobi against LAPACK and the device's atan2 / asin.
    Measured on an MI355X, worst per visibility set: all 13 1.3e-13, index 5 invisible 1.5e-13, the six points 1.3e-12."""
    sets = {'all 13': None, 'index 5 invisible': [k for k in range(13) if k != 5], 'six points': SIX}
    cases = [(seed, noise, name) for seed in range(8) for noise in (0.0, 1.0) for name in sets]
    kps = np.stack([_keypoints(seed, noise, sets[name]) for seed, noise, name in cases])
    out = _forward(kps)
    assert out['rc'] == _lib.OK
    worst = {name: 0.0 for name in sets}
    for i, (seed, noise, name) in enumerate(cases):
        ref = _oracle_start(kps[i])
        if noise == 0.0:          # on exact pixels the oracle's start IS the planted camera: the comparison is about something
            f = synth._random_camera(np.random.default_rng(seed))[2]
            assert abs(ref[0] - f) < 1e-6 * f and abs(ref[1] - f) < 1e-6 * f, (seed, name, ref, f)
        assert out['status'][i] in (0, -3), (seed, noise, name, out['status'][i])          # the start exists whatever RANSAC made of it
        d = out['start'][i] - ref
        d[5:] = np.mod(d[5:] + np.pi, 2 * np.pi) - np.pi
        err = np.abs(d) / np.maximum(np.abs(ref), 1.0)
        worst[name] = max(worst[name], float(err.max()))
        assert err.max() <= 1e-9, (seed, noise, name, out['start'][i], ref)
    print('\nDLT start, device vs oracle, worst |dev - ref| / max(|ref|, 1): %s' % {k: '%.2e' % v for k, v in worst.items()})


# ---------------------------------------------------------------------------------------------- B2
def test_batch_and_subset_count_do_not_change_a_camera_bit_for_bit():
    kps, batch, solo = _five()
    assert batch['rc'] == _lib.OK and (batch['status'] == 0).all() and all(6 <= n <= v for n, v in zip(batch['n_inliers'], kps[:, :, 2].sum(1)))
    for i in range(5):
        _same_camera(batch, i, solo[i], 0, 'camera in a batch of 5 vs alone')
    # 128 subsets of which 100..127 repeat subset 0: the FIRST subset with the most inliers wins, so nothing changes
    big = _forward(kps, n_subsets=128)
    assert big['rc'] == _lib.OK
    for i in range(5):
        _same_camera(big, i, batch, i, '128 subsets (28 repeats of subset 0) vs 100')
    # one subset s alone = 100 copies of s
    base = np.stack([_subsets(kps[i], 100) for i in range(5)])
    for s in (0, 37, 99):
        one = _forward(kps, subsets=base[:, s:s + 1].copy(), n_subsets=1)
        many = _forward(kps, subsets=np.repeat(base[:, s:s + 1], 100, axis=1), n_subsets=100)
        assert one['rc'] == _lib.OK and many['rc'] == _lib.OK
        for i in range(5):
            _same_camera(one, i, many, i, 'subset %d alone vs 100 copies of it' % s)
    # the start does not depend on the subsets at all; a null start_dev changes nothing else
    assert np.array_equal(one['start'], batch['start'])
    quiet = _forward(kps, want_start=False)
    for k in ('mint', 'mext', 'n_inliers', 'status'):
        assert np.array_equal(quiet[k], batch[k]), k
    # refused before anything is launched
    for kw in ({'n_subsets': 0}, {'n_subsets': 129}, {'max_iter': 0}):
        sub = np.zeros((5, max(kw.get('n_subsets', 100), 1), 4), np.int32)
        bad = _forward(kps, subsets=sub, **kw)
        assert bad['rc'] == _lib.EINVAL and b'ttup_calib_forward' in _lib.load().ttup_last_error(), kw
        assert (bad['status'] == -7).all() and (bad['n_inliers'] == -7).all() and (bad['mint'] == SENTINEL).all() and (bad['start'] == SENTINEL).all(), kw


# ---------------------------------------------------------------------------------------------- B3
def test_too_few_keypoints_is_status_minus_one_and_leaves_the_neighbours_alone():
    kps, _, solo = _five()
    few = _keypoints(30, noise=1.0, visible=[0, 1, 4, 5, 9])
    out = _forward(np.stack([kps[0], few, kps[1]]))
    assert out['rc'] == _lib.OK and out['status'].tolist() == [0, -1, 0] and out['n_inliers'][1] == 0
    _same_camera(out, 0, solo[0], 0, 'left neighbour of a refused camera')
    _same_camera(out, 2, solo[1], 0, 'right neighbour of a refused camera')
    # through the package the same input raises what the reference raises (regress_cameramatrices.py:209), before any launch
    with pytest.raises(AssertionError):
        calib.calibrate_cameras(np.stack([kps[0], few, kps[1]]))


# ---------------------------------------------------------------------------------------------- B4
DEGENERATE = {'index 9 invisible': [k for k in range(13) if k != 9],
              'indices 9 and 10 invisible': [k for k in range(13) if k not in (9, 10)],
              'six points': SIX}


@pytest.mark.parametrize('name', list(DEGENERATE))
def test_defined_behaviour_where_the_dlt_is_degenerate(name):
    """With a net-post top invisible the visible keypoints are a plane plus one point (the reference's DLT start is garbage, focal
    length off by 100 %), with both invisible they are coplanar, and from the six-point set the reference's BFGS diverges: no
    parity or recovery bar.  Required: either ValueError from the package, or finite matrices with an orthonormal rotation and
    status 0 -- never a non-finite matrix passed off as a result.
    Measured on an MI355X (8 noiseless cameras each): all three sets take the second outcome on every camera -- status 0, finite
    matrices, orthonormal rotation -- and the matrices are as meaningless as the reference's: with index 9 invisible 12 inliers but
    fx of either sign (-2615 .. 3128), with 9 and 10 invisible 2 inliers and fx ~ 1e-10 on seven cameras (11 inliers, fx -19.6 on one), on
    the six points 6 inliers and the planted fx on three cameras, 1 or 3 inliers and fx 0.01 .. 67 on five.  Nothing non-finite, so the
    kernel's status codes stay as they are."""
    kps = np.stack([_keypoints(seed, 0.0, DEGENERATE[name]) for seed in range(8)])
    raw = _forward(kps)
    assert raw['rc'] == _lib.OK
    print('\n%s: status %s, inliers %s, fx %s' % (name, raw['status'].tolist(), raw['n_inliers'].tolist(),
                                                   ['%.4g' % raw['mint'][i, 0, 0] if raw['status'][i] == 0 else '-' for i in range(8)]))
    for i in range(8):
        st = int(raw['status'][i])
        assert st in (0, -2, -3), (name, i, st)
        if st == 0:
            assert np.isfinite(raw['mint'][i]).all() and np.isfinite(raw['mext'][i]).all() and np.isfinite(raw['start'][i]).all(), (name, i)
            rot = raw['mext'][i][:3, :3]
            assert np.abs(rot @ rot.T - np.eye(3)).max() <= 1e-12 and np.array_equal(raw['mext'][i][3], [0, 0, 0, 1]), (name, i)
            assert 1 <= raw['n_inliers'][i] <= int(kps[i, :, 2].sum())
        else:
            assert raw['n_inliers'][i] == 0
        # the package's answer for this camera alone: the same matrices, or ValueError
        if st == 0:
            mint, mext, ninl = calib.calibrate_cameras(kps[i:i + 1])
            assert np.array_equal(mint[0], raw['mint'][i]) and np.array_equal(mext[0], raw['mext'][i]) and ninl[0] == raw['n_inliers'][i]
        else:
            with pytest.raises(ValueError):
                calib.calibrate_cameras(kps[i:i + 1])
