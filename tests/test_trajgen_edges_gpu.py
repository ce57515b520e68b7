"""The trajectory generator's two decision kernels (csrc/trajgen.hip) at their edges, on the MI355X.

Selection: every named crafted track of tests/helpers/trajgen_edge_cases.py and its random sweep, per mode x direction in one
launch, against oracle/trajgen_ref.select -- kept length, bounce count and bounce times exactly (float64 bits, no tolerance).
Stop rules: 65 seeds per mode x direction (a ragged second workgroup) against the oracle's recorded sample counts
(tests/golden/trajgen_edges.npz; tests/test_trajgen_edges_host.py recomputes the record and checks that every seed keeps
1e-4 m / 0.05 px from each threshold, so no mismatch here can be rounding).  The reference tree is never read."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from conftest import has_gpu
from oracle import trajgen_ref as T
from helpers import trajgen_edge_cases as C

pytestmark = pytest.mark.gpu
if has_gpu():
    from upliftingtabletennis_amd import _lib, trajgen

TIMES = T.save_times()
COMBOS = [(m, d) for m in T.MODES for d in T.DIRECTIONS]
I_SENT, F_SENT = -77, -123.456


def _pack(tracks, fill=None):
    """(S, 9, N) samples and n_saved of position tracks; rows at and beyond a track's length: zeros, or `fill` (S, 3)."""
    samples = np.zeros((C.S, 9, len(tracks)))
    if fill is not None:
        samples[:, 0:3, :] = fill[:, :, None]
    for i, tr in enumerate(tracks):
        samples[:len(tr), 0:3, i] = tr
    return samples, np.array([len(tr) for tr in tracks], dtype=np.int32)


def _select(samples, n_saved, mode, direction):
    nk, bo, nb = trajgen.select_positions(torch.from_numpy(samples).cuda(), torch.from_numpy(n_saved).cuda(), mode, direction)
    return nk.cpu().numpy(), nb.cpu().numpy(), bo.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _pool(mode, direction):
    """Named cases + sweep of one combination with the oracle's answers: names, tracks, labels, (n_keep, n_bounces, bounces (N, 4))."""
    cases = C.named_cases(mode, direction)
    names = [c['name'] for c in cases]
    tracks = [C.track(c) for c in cases]
    for j, tr in enumerate(C.random_tracks(mode, direction)):
        names.append('%s/%s/random/%d' % (mode, direction, j))
        tracks.append(tr)
    n = len(tracks)
    keep, nb, bo, labels = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 4)), []
    for i, tr in enumerate(tracks):
        why = []
        res = T.select(tr, TIMES, mode, direction, why=why)
        labels.append('/'.join(why))
        if res is not None:
            keep[i], nb[i] = res[0], len(res[1])
            bo[i, :nb[i]] = res[1]
    return names, tracks, labels, (keep, nb, bo)


def _same_bits(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _first_difference(got, want, names, labels):
    for i in range(len(names)):
        if got[0][i] != want[0][i] or got[1][i] != want[1][i] or got[2][i].tobytes() != want[2][i].tobytes():
            return 'lane %d %s [%s]: device n_keep %d n_bounces %d bounces %r, oracle %d %d %r' % (
                i, names[i], labels[i], got[0][i], got[1][i], got[2][i].tolist(), want[0][i], want[1][i], want[2][i].tolist())
    return None


def test_sample_buffer_is_what_the_cases_assume():
    assert _lib.load().ttup_trajgen_max_samples() == C.S == len(TIMES)


@pytest.mark.parametrize('mode,direction', COMBOS)
def test_crafted_selection_is_exact(mode, direction):
    """One launch over all named cases and the sweep; the wrapper's zero-filled `bounces` make the whole (N, 4) array comparable."""
    names, tracks, labels, want = _pool(mode, direction)
    got = _select(*_pack(tracks), mode, direction)
    assert _first_difference(got, want, names, labels) is None, _first_difference(got, want, names, labels)
    assert (want[0] > 0).sum() >= 100 and (want[0] == 0).sum() >= 100


@pytest.mark.parametrize('mode,direction', COMBOS)
def test_rows_beyond_n_saved_are_inert(mode, direction):
    """Rows at and beyond n_saved hold NaN, then the continuation of an accepted 500-sample track: the same output bits."""
    names, tracks, labels, want = _pool(mode, direction)
    cont = tracks[names.index('%s/%s/len/late_%d' % (mode, direction, C.S))]
    assert len(cont) == C.S and want[0][names.index('%s/%s/len/late_%d' % (mode, direction, C.S))] == C.S
    plain = _select(*_pack(tracks), mode, direction)
    for fill in (np.full((C.S, 3), np.nan), cont):
        got = _select(*_pack(tracks, fill), mode, direction)
        assert _same_bits(got, plain), _first_difference(got, plain, names, labels)


@pytest.mark.parametrize('mode,direction', [('first_short', 'left_to_right'), ('final_win', 'right_to_left')])
def test_selection_lanes_are_independent(mode, direction):
    """N = 1, 63, 64, 65, 129 (one lane, a ragged, a full and two / three workgroups): every lane equals the track selected alone and
    the batch in reversed order; the first and last lane of the first workgroup, lane 64 and the last lane hold accepted tracks."""
    names, tracks, labels, want = _pool(mode, direction)
    accepted = [i for i in range(len(tracks)) if want[0][i] > 0]
    order = list(range(129))                       # the first 129 named cases ...
    for slot, i in zip((0, 62, 63, 64, 128), accepted[3:]):          # ... with accepted ones at the workgroup edges
        order[slot] = i
    batch = [tracks[i] for i in order]
    alone = [_select(*_pack([tr]), mode, direction) for tr in batch]
    alone = tuple(np.concatenate([a[j] for a in alone]) for j in range(3))
    assert _first_difference(alone, tuple(w[order] for w in want), [names[i] for i in order], [labels[i] for i in order]) is None
    for n in (1, 63, 64, 65, 129):
        sub = batch[:n]
        assert alone[0][0] > 0 and alone[0][n - 1] > 0
        fwd = _select(*_pack(sub), mode, direction)
        rev = _select(*_pack(sub[::-1]), mode, direction)
        assert _same_bits(fwd, tuple(a[:n] for a in alone)), n
        assert _same_bits(tuple(r[::-1].copy() for r in rev), tuple(a[:n].copy() for a in alone)), n


def _select_abi(samples, n_saved, mode, direction, n=None):
    """`ttup_trajgen_select` itself on sentinel-filled outputs (the kernel does not write `bounces` of rejected lanes or entries at and
    beyond n_bounces: trajgen.select_positions zero-fills them beforehand)."""
    lib = _lib.load()
    n = len(n_saved) if n is None else n
    sm, ns = torch.from_numpy(samples).cuda(), torch.from_numpy(n_saved).cuda()
    nk = torch.full((len(n_saved),), I_SENT, dtype=torch.int32, device='cuda')
    nb = torch.full((len(n_saved),), I_SENT, dtype=torch.int32, device='cuda')
    bo = torch.full((len(n_saved), 4), F_SENT, dtype=torch.float64, device='cuda')
    ws_bytes = lib.ttup_trajgen_workspace_bytes(max(n, 1))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device='cuda')
    rc = lib.ttup_trajgen_select(_lib.ptr(sm), _lib.ptr(ns), n, T.MODES.index(mode), T.DIRECTIONS.index(direction), _lib.ptr(nk), _lib.ptr(bo), _lib.ptr(nb),
                                 _lib.ptr(ws), ws_bytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, nk.cpu().numpy(), nb.cpu().numpy(), bo.cpu().numpy()


@pytest.mark.parametrize('mode,direction', [('first_good', 'left_to_right'), ('intermediate', 'right_to_left')])
def test_select_writes_every_lane_and_only_the_bounces_it_counts(mode, direction):
    """The C ABI on stale buffers: n_keep and n_bounces of EVERY lane are written, rejected lanes included.  `bounces` of rejected lanes
    and the entries at and beyond n_bounces keep the sentinel -- the kernel does not write them, the Python wrapper zero-fills them --
    and n_seeds == 0 returns TTUP_OK without touching anything."""
    names, tracks, labels, want = _pool(mode, direction)
    samples, n_saved = _pack(tracks)
    rc, nk, nb, bo = _select_abi(samples, n_saved, mode, direction)
    assert rc == _lib.OK
    assert np.array_equal(nk, want[0]) and np.array_equal(nb, want[1])
    written = np.arange(4)[None, :] < want[1][:, None]
    assert np.array_equal(bo[written], want[2][written]) and (bo[~written] == F_SENT).all()
    assert (want[0] == 0).sum() >= 100 and (bo[want[0] == 0] == F_SENT).all()
    rc, nk, nb, bo = _select_abi(samples, n_saved, mode, direction, n=0)
    assert rc == _lib.OK and (nk == I_SENT).all() and (nb == I_SENT).all() and (bo == F_SENT).all()


# ---------------------------------------------------------------- stop rules
def _simulate_abi(seeds, mode, direction, camera=None):
    """`ttup_trajgen_simulate` + `ttup_trajgen_select` on NaN / sentinel-filled buffers: samples (S, 9, N), n_saved, n_keep, n_bounces, bounces."""
    lib = _lib.load()
    n = len(seeds)
    sd = torch.as_tensor(np.asarray(seeds, dtype=np.int64), device='cuda')
    samples = torch.full((C.S, 9, n), float('nan'), dtype=torch.float64, device='cuda')
    n_saved = torch.full((n,), I_SENT, dtype=torch.int32, device='cuda')
    nk = torch.full((n,), I_SENT, dtype=torch.int32, device='cuda')
    nb = torch.full((n,), I_SENT, dtype=torch.int32, device='cuda')
    bo = torch.full((n, 4), F_SENT, dtype=torch.float64, device='cuda')
    ws_bytes = lib.ttup_trajgen_workspace_bytes(n)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device='cuda')
    ex, mint = trajgen.camera_matrices() if camera is None else camera
    cam = np.ascontiguousarray(np.concatenate([ex.reshape(-1), mint.reshape(-1)]), dtype=np.float64)
    m, d = T.MODES.index(mode), T.DIRECTIONS.index(direction)
    _lib.check(lib.ttup_trajgen_simulate(_lib.ptr(sd), n, m, d, T.SUBSTEPS, cam.ctypes.data_as(ctypes.c_void_p), _lib.ptr(samples), _lib.ptr(n_saved), None,
                                         _lib.ptr(ws), ws_bytes, _lib.stream_ptr()))
    _lib.check(lib.ttup_trajgen_select(_lib.ptr(samples), _lib.ptr(n_saved), n, m, d, _lib.ptr(nk), _lib.ptr(bo), _lib.ptr(nb), _lib.ptr(ws), ws_bytes,
                                       _lib.stream_ptr()))
    torch.cuda.synchronize()
    return samples.cpu().numpy(), n_saved.cpu().numpy(), nk.cpu().numpy(), nb.cpu().numpy(), bo.cpu().numpy()


def _oracle_first_samples(seeds, mode, direction, count=20):
    """The oracle's first `count` sampled positions (N, count, 3): sample 0 after 1 ms, sample k at 2k ms."""
    st = [T.init_state(s, mode, direction) for s in seeds]
    r, v, w = (np.stack([s[j] for s in st]) for j in range(3))
    out = np.zeros((len(seeds), count, 3))
    for k in range(count):
        r, v, w = T.step_ms(r, v, w, 1 if k < 2 else 2)
        out[:, k] = r
    return out


@pytest.mark.parametrize('mode,direction', COMBOS)
def test_stop_rules_match_the_oracle(mode, direction, golden):
    """n_saved of 65 seeds equals the oracle's for every mode x direction (all five `switch` arms of out_of_bounds, both sides, the
    out-of-image stop, all 500 labels), free flight within 1e-9 m over the first 20 samples; lanes 0, 63 and 64 give the same bits alone
    and with the batch reversed; sample rows at and beyond n_saved keep their NaN prefill."""
    g = golden('trajgen_edges.npz')
    key = 'stop/%s/%s' % (mode, direction)
    seeds = C.stop_seeds(mode, direction)
    assert np.array_equal(g[key + '/seeds'], seeds) and len(seeds) == 65
    want_ns = g[key + '/n_saved']
    reasons = [T.STOP_REASONS[r] for r in g[key + '/reason']]
    assert set(reasons) == set(C.STOP_REASONS[mode])
    assert any(r == 'image' and 0 < n < C.S for r, n in zip(reasons, want_ns))
    res = trajgen.simulate_seeds(seeds, mode, direction)
    ns = res['n_saved'].cpu().numpy()
    bad = [(i, seeds[i], reasons[i], int(ns[i]), int(want_ns[i])) for i in range(65) if ns[i] != want_ns[i]]
    assert not bad, 'lane, seed, oracle stop reason, device n_saved, oracle n_saved: %r' % bad
    got = res['samples'].cpu().numpy()
    ref = _oracle_first_samples(seeds, mode, direction)
    for i in range(65):
        k = min(int(ns[i]), 20)
        assert k == 0 or np.abs(got[:k, 0:3, i] - ref[i, :k]).max() <= 1e-9, (i, seeds[i])
    # the C ABI on prefilled buffers: same results, untouched rows, independent lanes
    full = _simulate_abi(seeds, mode, direction)
    assert np.array_equal(full[1], ns) and np.array_equal(full[2], res['n_keep'].cpu().numpy()) and np.array_equal(full[3], res['n_bounces'].cpu().numpy())
    rev = _simulate_abi(seeds[::-1], mode, direction)
    for i in range(65):
        n = int(ns[i])
        assert np.isnan(full[0][n:, :, i]).all() and not np.isnan(full[0][:n, :, i]).any(), (i, seeds[i])
        assert got[:n, :, i].tobytes() == full[0][:n, :, i].tobytes()
        j = 64 - i
        assert full[0][:n, :, i].tobytes() == rev[0][:n, :, j].tobytes() and np.isnan(rev[0][n:, :, j]).all(), (i, seeds[i])
        assert all(full[q][i].tobytes() == rev[q][j].tobytes() for q in (1, 2, 3, 4)), (i, seeds[i])
    for i in (0, 63, 64):
        one = _simulate_abi([seeds[i]], mode, direction)
        n = int(ns[i])
        assert one[0][:n, :, 0].tobytes() == full[0][:n, :, i].tobytes() and np.isnan(one[0][n:, :, 0]).all(), (i, seeds[i])
        assert all(one[q][0].tobytes() == full[q][i].tobytes() for q in (1, 2, 3, 4)), (i, seeds[i])


def test_out_of_image_stop_follows_the_camera_argument(golden):
    """`ttup_trajgen_simulate` with a camera whose principal point is moved 300 px: other tracks leave the image, at other samples, and
    n_saved equals the oracle's under that camera (same seeds, same margin rule in pixels); nothing in the kernel assumes the fixed camera."""
    g = golden('trajgen_edges.npz')
    mode, direction = C.CAMERA_COMBO
    seeds = C.stop_seeds(mode, direction)
    want, fixed = g['stop_camera/n_saved'], g['stop/%s/%s/n_saved' % (mode, direction)]
    assert (want != fixed).sum() >= 10
    samples, ns, _, _, _ = _simulate_abi(seeds, mode, direction, camera=C.shifted_camera())
    bad = [(i, seeds[i], T.STOP_REASONS[g['stop_camera/reason'][i]], int(ns[i]), int(want[i])) for i in range(65) if ns[i] != want[i]]
    assert not bad, 'lane, seed, oracle stop reason, device n_saved, oracle n_saved: %r' % bad
    plain = _simulate_abi(seeds, mode, direction)
    for i in range(65):                              # up to the earlier stop the two cameras saw the same flight
        n = int(min(ns[i], plain[1][i]))
        assert samples[:n, :, i].tobytes() == plain[0][:n, :, i].tobytes() and np.isnan(samples[int(ns[i]):, :, i]).all()


@pytest.mark.parametrize('mode,direction', [('final_lose', 'left_to_right'), ('intermediate', 'right_to_left')])
def test_get_valid_trajectories_does_not_depend_on_batches_per_launch(mode, direction):
    ref = trajgen.get_valid_trajectories(6, 4, mode, direction, batches_per_launch=1)
    assert len(ref) == 6
    for b in (3, 64):
        got = trajgen.get_valid_trajectories(6, 4, mode, direction, batches_per_launch=b)
        assert [t['seed'] for t in got] == [t['seed'] for t in ref]
        for a, e in zip(got, ref):
            for k in ('positions', 'velocities', 'rotations', 'times', 'Mext', 'Mint', 'bounces'):
                x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(e[k])
                assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), (b, k, a['seed'])
