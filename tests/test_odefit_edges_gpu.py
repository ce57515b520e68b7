"""g1: the drag + Magnus ODE fit (csrc/odefit.hip) at the edges of its lane mapping and of its inputs: trajectories below, at and
above 7 per wave, per-trajectory cameras that differ, irregular and non-increasing time stamps, per-row masks, an all-masked
row, tracks of 1..3 stamps, iteration caps, null optional outputs and refused arguments.

Pixels come from the numpy oracle (oracle/odefit_ref.py), never from the device integrator; "noisy" adds 0.5 px of seeded
Gaussian noise, so costs are O(0.25-0.5) px^2 and relative comparisons mean something.  Where the lanes of one trajectory
never read another trajectory's values the comparison is bit for bit (`torch.equal`).  /root/reference is never read.

Measured on an MI355X: the reported cost agrees with the oracle's cost at the returned parameters to 5.1e-14 relative at worst
over the irregular-stamp tracks (bar 1e-8), the reported positions to 3.1e-16 relative (bar 1e-12); every bit-for-bit
comparison holds as it stands, none had to become a tolerance."""
import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu
from oracle import odefit_ref as R

pytestmark = pytest.mark.gpu
if has_gpu():
    from upliftingtabletennis_amd import _lib, odefit

H, T = 2e-3, 40
OFFSET = np.array([0.02] * 3 + [0.2] * 3 + [5.0] * 3)          # start: planted + (0.02 m, 0.2 m/s, 5 rad/s)
KEYS = ('params', 'cost', 'iters', 'pos3d')


def _pixels(p, times, cam):
    """Oracle pixels (B,T,2); cam (21,) shared or (B,21) per trajectory."""
    cam = np.asarray(cam)
    return np.stack([R.project(cam if cam.ndim == 1 else cam[i], R.integrate(p[i], times[i], H)) for i in range(len(p))])


def _noisy(px, seed):
    return px + np.random.default_rng(seed).normal(0, 0.5, px.shape)


def _cost(params, times, cam, obs, mask=None):
    """Mean over the valid stamps of the squared re-projection distance, and the oracle's positions."""
    pos = R.integrate(params, times, H)
    m = np.ones(len(times), bool) if mask is None else np.asarray(mask) != 0
    return float(np.mean(np.sum((R.project(cam, pos) - obs)[m] ** 2, axis=1))), pos


def _rel(got, ref):
    return float(np.abs(np.asarray(got) - ref).max() / np.abs(ref).max())


def _same(a, i, b, j, what, keys=KEYS):
    for k in keys:
        assert torch.equal(a[k][i], b[k][j]), (what, k, i, j, a[k][i], b[k][j])


def _np(out, k, i):
    return out[k][i].cpu().numpy()


@functools.lru_cache(maxsize=None)
def _tracks():
    """8 noisy tracks on irregular stamps with a different mask per row (12..30 valid stamps; row 0 without its first stamp,
    row 1 without its last).  Shared by the cost, time-stamp and mask tests: never modified, callers copy."""
    b = 8
    p, _, cam = odefit.synth_arcs(b, T, seed=21)
    rng = np.random.default_rng(22)
    times = np.cumsum(rng.uniform(0.004, 0.03, (b, T)), axis=1)
    mask = np.zeros((b, T))
    for i in range(b):
        pool = np.arange(1, T) if i == 0 else (np.arange(T - 1) if i == 1 else np.arange(T))
        mask[i, rng.choice(pool, int(rng.integers(12, 31)), replace=False)] = 1.0
    obs = _noisy(_pixels(p, times, cam), 23)
    init = p + OFFSET
    return {'p': p, 'times': times, 'cam': cam, 'mask': mask, 'obs': obs, 'init': init}


@functools.lru_cache(maxsize=None)
def _tracks_fit():
    d = _tracks()
    return odefit.fit(d['obs'], d['times'], d['cam'], d['init'], mask=d['mask'])


# ---------------------------------------------------------------------------------------------- A1: the lane mapping
def test_grouping_does_not_matter_bit_for_bit():
    """7 trajectories share a wave (9 lanes each, lane 63 idle); the lanes of a group only ever read their own group's values,
    so a trajectory's result cannot depend on its wave-mates, its slot in the wave, or how many workgroups there are.
    B = 15 is two full waves and a last workgroup with one active group; 6, 7, 8 and 13 straddle the wave size."""
    b = 15
    p, times, cam = odefit.synth_arcs(b, T, seed=11)
    obs = _noisy(_pixels(p, times, cam), 12)
    init = p + OFFSET
    full = odefit.fit(obs, times, cam, init)
    rev = odefit.fit(obs[::-1].copy(), times[::-1].copy(), cam, init[::-1].copy())
    solo = [odefit.fit(obs[i:i + 1], times[i:i + 1], cam, init[i:i + 1]) for i in range(b)]
    iters = full['iters'].cpu().numpy()
    print('\naccepted steps per trajectory:', iters.tolist())
    # groups of one wave stop at different rounds: the finished ones idle through their wave-mates' shuffles and barriers
    assert len(set(iters[:7].tolist())) > 1 and (iters > 0).all()
    for i in range(b):
        _same(full, i, solo[i], 0, 'batch of 15 vs alone')
        _same(full, i, rev, b - 1 - i, 'batch of 15 vs reversed batch')
    for n in (6, 7, 8, 13):
        part = odefit.fit(obs[:n], times[:n], cam, init[:n])
        for i in (0, n - 1):
            _same(part, i, solo[i], 0, 'batch of %d vs alone' % n)


# ---------------------------------------------------------------------------------------------- A2: cameras per trajectory
def _nine_cameras(golden):
    g = golden('calib64.npz')
    cams = np.stack([odefit._cam21(g['calib64/%d/Mext_true' % ci], g['calib64/%d/Mint_true' % ci][:, :3]) for ci in range(9)])
    assert all(np.abs(cams[i] - cams[j]).max() > 1e-2 for i in range(9) for j in range(i))
    return cams


def test_per_trajectory_cameras_that_differ(golden):
    """Nine different cameras (true cameras of the 64-camera calibration fixture): a wrong stride in `cam + traj * 21`, in the
    integrator or in the fit, reads a neighbour's camera.  No claim about recovery: some camera / arc pairs end in a local
    minimum (odefit.bench)."""
    cams = _nine_cameras(golden)
    p, times, _ = odefit.synth_arcs(9, T, seed=31)
    pos, px = odefit.integrate(p, times, cams)
    ref_px = np.empty((9, T, 2))
    for i in range(9):
        ref = R.integrate(p[i], times[i], H)
        ref_px[i] = R.project(cams[i], ref)
        assert (ref @ cams[i][8:11] + cams[i][11] > 1.0).all()          # the arc is in front of this camera
        assert _rel(pos[i].cpu().numpy(), ref) <= 1e-12
        assert np.abs(px[i].cpu().numpy() - ref_px[i]).max() <= 1e-9, (i, np.abs(px[i].cpu().numpy() - ref_px[i]).max())
    # the neighbour's camera would be far off: the bar above is meaningful
    assert min(np.abs(ref_px[i] - R.project(cams[(i + 1) % 9], R.integrate(p[i], times[i], H))).max() for i in range(9)) > 1.0
    obs = _noisy(ref_px, 32)
    init = p + OFFSET
    full = odefit.fit(obs, times, cams, init)
    for i in range(9):
        solo = odefit.fit(obs[i:i + 1], times[i:i + 1], cams[i], init[i:i + 1])
        _same(full, i, solo, 0, 'per-trajectory camera vs the same camera shared')


# ---------------------------------------------------------------------------------------------- A3: cost and positions
def test_reported_cost_is_the_oracle_cost_at_the_returned_parameters():
    """Ties the time handling of the fit's Jacobian pass (`normal_equations`) to the integrator's: irregular stamps, a
    different mask per row.  Bar 1e-8 relative on the cost: about twice what the 1e-9-px integrator bar allows on a 0.5-px
    residual.  Measured on an MI355X: worst cost agreement 5.1e-14 relative, worst position agreement 3.1e-16 relative."""
    d, out = _tracks(), _tracks_fit()
    worst_c, worst_p = 0.0, 0.0
    for i in range(8):
        got = _np(out, 'params', i)
        c_ref, pos_ref = _cost(got, d['times'][i], d['cam'], d['obs'][i], d['mask'][i])
        c_init, _ = _cost(d['init'][i], d['times'][i], d['cam'], d['obs'][i], d['mask'][i])
        c_dev = out['cost'][i].item()
        rel_c, rel_p = abs(c_dev - c_ref) / c_ref, _rel(_np(out, 'pos3d', i), pos_ref)
        print('row %d: %2d valid stamps, cost %.6f px^2 (start %.3f), %2d steps, cost vs oracle %.2e, positions vs oracle %.2e'
              % (i, int(d['mask'][i].sum()), c_dev, c_init, out['iters'][i].item(), rel_c, rel_p))
        worst_c, worst_p = max(worst_c, rel_c), max(worst_p, rel_p)
        assert np.isfinite(got).all() and 0.0 < c_ref < 5.0
        assert rel_c <= 1e-8, (i, c_dev, c_ref)
        assert rel_p <= 1e-12, (i, rel_p)
        assert c_dev <= c_init * (1 + 1e-12), (i, c_dev, c_init)
    print('worst cost agreement %.3e relative, worst position agreement %.3e relative' % (worst_c, worst_p))


# ---------------------------------------------------------------------------------------------- A4: non-increasing stamps
def _insert_stamps(d, extra):
    """The shared tracks with extra stamps: `extra[i]` lists row i's (k, time, mask, pixel), each put in before original index k
    (in list order where k repeats).  Returns times, mask, obs and, per row, the new indices of the extra stamps."""
    times, mask, obs, where = [], [], [], []
    for i in range(8):
        t, m, o, w = [], [], [], []
        for k in range(T + 1):
            for kk, tv, mv, ov in extra[i]:
                if kk == k:
                    w.append(len(t)); t.append(tv); m.append(mv); o.append(ov)
            if k < T:
                t.append(d['times'][i][k]); m.append(d['mask'][i][k]); o.append(d['obs'][i][k])
        times.append(t); mask.append(m); obs.append(o); where.append(w)
    return np.array(times), np.array(mask), np.array(obs), where


def test_a_stamp_not_later_than_the_last_used_one_adds_no_step():
    """A masked-out stamp with time 0 INSIDE a track (a missed frame, padded the way the uplift inputs pad): the integrator
    (`odeint_kernel`, the fit's `pos3d` loop, the oracle) keeps its base time and skips it.  `normal_equations` used to move
    its base time to the skipped stamp's 0 and then integrated the next interval over the whole time since 0 -- the fit
    minimised residuals of another model than the one it reports.  Now the padded track gives the results of the track
    with those stamps deleted, bit for bit: they contribute exact zeros and no step."""
    d, clean = _tracks(), _tracks_fit()
    # two padded stamps per row at places that differ from row to row: right after the first stamp (row 0), right before the
    # last (row 1), next to each other (row 7)
    spots = [(1, 17), (9, T - 1), (5, 22), (8, 30), (12, 13), (3, 27), (20, 33), (15, 15)]
    pads = [[(k, 0.0, 0.0, d['obs'][i][k - 1] + 500.0) for k in spots[i]] for i in range(8)]          # time 0, masked, garbage pixel
    times, mask, obs, where = _insert_stamps(d, pads)
    assert times.shape == (8, T + 2) and all((times[i, where[i]] == 0.0).all() and (mask[i, where[i]] == 0.0).all() for i in range(8))
    out = odefit.fit(obs, times, d['cam'], d['init'], mask=mask)
    for i in range(8):
        _same(out, i, clean, i, 'padded vs deleted stamps', keys=('params', 'cost', 'iters'))
        pos, keep = out['pos3d'][i], [k for k in range(T + 2) if k not in where[i]]
        assert torch.equal(pos[keep], clean['pos3d'][i])
        for k in where[i]:
            assert torch.equal(pos[k], pos[k - 1]), (i, k)
    # the device integrator follows the same rule (positions and pixels of the padded stamps repeat the ones before)
    pos, px = odefit.integrate(out['params'], times, d['cam'])
    assert all(torch.equal(pos[i, k], pos[i, k - 1]) and torch.equal(px[i, k], px[i, k - 1]) for i in range(8) for k in where[i])
    assert (pos - out['pos3d']).abs().max().item() <= 1e-12 * out['pos3d'].abs().max().item()
    # a repeated stamp that IS observed (mask 1, its own noisy pixel) adds a residual at the same state and no step
    rng = np.random.default_rng(24)
    dup_at = [int(np.nonzero(d['mask'][i][2:T - 2])[0][i % 3]) + 2 for i in range(8)]          # a valid interior stamp per row
    dups = [[(k + 1, d['times'][i][k], 1.0, d['obs'][i][k] + rng.normal(0, 0.5, 2))] for i, k in enumerate(dup_at)]
    t2, m2, o2, w2 = _insert_stamps(d, dups)
    assert all(t2[i, w2[i][0]] == t2[i, w2[i][0] - 1] and m2[i, w2[i][0] - 1] == 1.0 for i in range(8))
    dup = odefit.fit(o2, t2, d['cam'], d['init'], mask=m2)
    for i in range(8):
        c_ref, pos_ref = _cost(_np(dup, 'params', i), t2[i], d['cam'], o2[i], m2[i])
        assert abs(dup['cost'][i].item() - c_ref) <= 1e-8 * c_ref, (i, dup['cost'][i].item(), c_ref)
        assert _rel(_np(dup, 'pos3d', i), pos_ref) <= 1e-12
        assert torch.equal(dup['pos3d'][i, w2[i][0]], dup['pos3d'][i, w2[i][0] - 1])
        assert not torch.equal(dup['params'][i], clean['params'][i])          # the extra observation counts
    # both kinds in one track: the padded stamps still change nothing
    t3, m3, o3, _ = _insert_stamps(d, [dups[i] + pads[i] for i in range(8)])
    assert t3.shape == (8, T + 3) and (m3.sum(1) == d['mask'].sum(1) + 1).all() and ((t3 == 0.0).sum(1) == 2).all()
    mixed = odefit.fit(o3, t3, d['cam'], d['init'], mask=m3)
    for i in range(8):
        _same(mixed, i, dup, i, 'repeated + padded stamps vs the repeated one alone', keys=('params', 'cost', 'iters'))


# ---------------------------------------------------------------------------------------------- A5: masks
def test_masked_pixels_are_never_read_and_an_all_masked_row_keeps_its_start():
    d, clean = _tracks(), _tracks_fit()
    bad = d['obs'].copy()
    bad[d['mask'] == 0.0] += 500.0
    out = odefit.fit(bad, d['times'], d['cam'], d['init'], mask=d['mask'])
    for i in range(8):
        _same(out, i, clean, i, 'corrupted masked pixels')
    mask = d['mask'].copy()
    mask[3] = 0.0
    out = odefit.fit(d['obs'], d['times'], d['cam'], d['init'], mask=mask)
    init3 = torch.from_numpy(d['init'][3].copy()).to(out['params'].device)
    assert torch.equal(out['params'][3], init3)
    assert out['cost'][3].item() == 0.0 and out['iters'][3].item() == 0
    assert _rel(_np(out, 'pos3d', 3), R.integrate(d['init'][3], d['times'][3], H)) <= 1e-12
    for i in (0, 1, 2, 4, 5, 6, 7):
        _same(out, i, clean, i, 'wave-mate of an all-masked row')


# ---------------------------------------------------------------------------------------------- A6: lengths, caps, grids
@pytest.mark.parametrize('t', [1, 2, 3])
def test_tracks_of_one_two_and_three_stamps(t):
    b = 3
    p, times, cam = odefit.synth_arcs(b, t, seed=41)
    obs = _noisy(_pixels(p, times, cam), 42 + t)
    init = p + OFFSET
    out = odefit.fit(obs, times, cam, init)
    for k in KEYS:
        assert torch.isfinite(out[k].double()).all(), k
    assert out['pos3d'].shape == (b, t, 3)
    for i in range(b):
        c_init, _ = _cost(init[i], times[i], cam, obs[i])
        print('T=%d row %d: cost %.3e px^2 from %.3f, %d steps' % (t, i, out['cost'][i].item(), c_init, out['iters'][i].item()))
        assert out['cost'][i].item() <= c_init * (1 + (1e-12 if t > 1 else 0.0))
    if t == 1:
        # at the first stamp the Jacobian columns of velocity and spin are exactly zero: no step ever moves them
        assert torch.equal(out['params'][:, 3:9], torch.from_numpy(init[:, 3:9].copy()).to(out['params'].device))


def test_iteration_caps():
    p, times, cam = odefit.synth_arcs(8, T, seed=51)
    obs = _noisy(_pixels(p, times, cam), 52)
    init = p + OFFSET
    one = odefit.fit(obs, times, cam, init, max_iter=1)
    three = odefit.fit(obs, times, cam, init, max_iter=3)
    assert (one['iters'] <= 1).all() and (three['iters'] <= 3).all() and (three['iters'] >= one['iters']).all()
    for i in range(8):
        c_init, _ = _cost(init[i], times[i], cam, obs[i])
        assert one['cost'][i].item() <= c_init, (i, one['cost'][i].item(), c_init)
        assert three['cost'][i].item() <= one['cost'][i].item() * (1 + 1e-12)
        c_ref, _ = _cost(_np(one, 'params', i), times[i], cam, obs[i])
        assert abs(one['cost'][i].item() - c_ref) <= 1e-8 * c_ref
    assert (one['iters'] == 1).any()


@pytest.mark.parametrize('fps', [250.0, 500.0])
def test_stamps_on_a_grid_of_whole_steps(fps):
    """dt / h_max is a whole number (2 and 1): `substeps` rounds the quotient the oracle's way on both sides of the integer."""
    p, times, cam = odefit.synth_arcs(3, T, fps=fps, seed=61)
    assert {R.substeps(dt, H) for dt in np.diff(times[0])} == {int(round(500.0 / fps))} and len(set(np.diff(times[0]) / H)) > 1
    pos, px = odefit.integrate(p, times, cam, h_max=H)
    obs = _noisy(_pixels(p, times, cam), 62)
    out = odefit.fit(obs, times, cam, p + OFFSET, h_max=H)
    for i in range(3):
        ref = R.integrate(p[i], times[i], H)
        assert _rel(pos[i].cpu().numpy(), ref) <= 1e-12
        assert np.abs(px[i].cpu().numpy() - R.project(cam, ref)).max() <= 1e-9
        c_ref, pos_ref = _cost(_np(out, 'params', i), times[i], cam, obs[i])
        assert _rel(_np(out, 'pos3d', i), pos_ref) <= 1e-12
        assert abs(out['cost'][i].item() - c_ref) <= 1e-8 * c_ref


# ---------------------------------------------------------------------------------------------- A7: surface
def _forward(obs, times, cam, init, h_max=H, max_iter=80, tol=1e-14, length=None, full=True):
    """ttup_odefit_forward itself: returns (rc, params, pos3d, cost, iters); the optional outputs are null unless `full`.
    The outputs are pre-filled so that a refused call can be seen to have written nothing."""
    lib = _lib.load()
    dev = torch.device('cuda')
    o, t, c, s = (torch.as_tensor(np.asarray(a, np.float64)).to(dev).contiguous() for a in (obs, times, cam, init))
    b, n = t.shape
    params = torch.full((b, 9), -7.0, dtype=torch.float64, device=dev)
    pos = torch.full((b, n, 3), -7.0, dtype=torch.float64, device=dev) if full else None
    cost = torch.full((b,), -7.0, dtype=torch.float64, device=dev) if full else None
    iters = torch.full((b,), -7, dtype=torch.int32, device=dev) if full else None
    rc = lib.ttup_odefit_forward(_lib.ptr(o), _lib.ptr(t), None, _lib.ptr(c), 0, _lib.ptr(s), b, n if length is None else length, float(h_max),
                                 int(max_iter), float(tol), _lib.ptr(params), _lib.ptr(pos), _lib.ptr(cost), _lib.ptr(iters), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, params, pos, cost, iters


def test_null_optional_outputs_empty_batch_and_refused_arguments():
    p, times, cam = odefit.synth_arcs(8, T, seed=71)
    obs = _noisy(_pixels(p, times, cam), 72)
    init = p + OFFSET
    ref = odefit.fit(obs, times, cam, init)
    rc, params, pos, cost, iters = _forward(obs, times, cam, init)
    assert rc == _lib.OK and torch.equal(params, ref['params']) and torch.equal(pos, ref['pos3d']) and torch.equal(cost, ref['cost']) and torch.equal(iters, ref['iters'])
    rc, params, _, _, _ = _forward(obs, times, cam, init, full=False)
    assert rc == _lib.OK and torch.equal(params, ref['params'])
    # an empty batch is not an error
    out = odefit.fit(np.zeros((0, T, 2)), np.zeros((0, T)), cam, np.zeros((0, 9)))
    assert out['params'].shape == (0, 9) and out['pos3d'].shape == (0, T, 3) and out['cost'].shape == (0,) and out['iters'].shape == (0,)
    pos, px = odefit.integrate(np.zeros((0, 9)), np.zeros((0, T)), cam)
    assert pos.shape == (0, T, 3) and px.shape == (0, T, 2)
    # refused with the library's error before anything is launched: the outputs keep what they held
    for kw in ({'max_iter': 0}, {'h_max': 0.0}, {'h_max': -1e-3}, {'tol': -1e-9}, {'length': 0}):
        rc, params, pos, cost, iters = _forward(obs, times, cam, init, **kw)
        assert rc == _lib.EINVAL, kw
        assert b'ttup_odefit_forward' in _lib.load().ttup_last_error()
        assert (params == -7.0).all() and (pos == -7.0).all() and (cost == -7.0).all() and (iters == -7).all(), kw
    for kw in ({'max_iter': 0}, {'h_max': 0.0}, {'tol': -1.0}):
        with pytest.raises(ValueError):
            odefit.fit(obs, times, cam, init, **kw)
    with pytest.raises(ValueError):
        odefit.fit(np.zeros((8, 0, 2)), np.zeros((8, 0)), cam, init)
