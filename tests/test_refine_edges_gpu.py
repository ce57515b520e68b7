"""The peak refinement kernels (csrc/refine.hip) at the edges of their launch arithmetic (cases and arithmetic:
tests/helpers/refine_edge_cases.py; tests/test_refine_edges_host.py checks the table itself on the CPU).

Argmax and window against oracle/refine_ref.argmax_window: indices exactly, windows as bits (NaN and -0.0 count), torch.argmax on
the device tensor as a second witness.  The fit against the reference's scipy answers on 24 edge windows per variant, window by
window, by the rule of tests/test_cabi.py: max(1e-6 px, 2 x _fit_radius)."""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from helpers import refine_edge_cases as R
from oracle import refine_ref
from test_cabi import _fit_radius

pytestmark = pytest.mark.gpu
if has_gpu():
    from upliftingtabletennis_amd import refine, _lib


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _check(heat, dev=None, want=None):
    """One launch on `heat` (n, h, w) float32 (or its device tensor `dev`): index and window against the oracle and torch.argmax."""
    n, h, w = heat.shape
    t = torch.from_numpy(heat).cuda() if dev is None else dev
    _, idx, win = refine.refine_device(t, 7 * w, 5 * h, _lib.REFINE_BALL)
    ri, rw = refine_ref.argmax_window(heat)
    got = idx.cpu().numpy()
    bad = np.flatnonzero(got != ri)
    assert bad.size == 0, 'maps %s: got %s, oracle %s' % (bad[:8].tolist(), got[bad[:8]].tolist(), ri[bad[:8]].tolist())
    assert np.array_equal(got, torch.argmax(t.reshape(n, -1), 1).cpu().numpy())
    if want is not None:
        assert np.array_equal(got, np.asarray(want))
    gw = _bits(win.cpu().numpy().reshape(n, 3, 3))
    badw = np.flatnonzero((gw != _bits(rw)).any(axis=(1, 2)))
    assert badw.size == 0, 'windows of maps %s differ, first:\n%s\nagainst\n%s' % (badw[:8].tolist(), win.cpu().numpy().reshape(n, 3, 3)[badw[0]], rw[badw[0]])


@pytest.mark.parametrize('shape', R.SWEEP_SHAPES, ids=lambda s: '%dx%d' % s)
def test_peak_at_every_position(shape):
    """hw maps in one launch, map k with its single peak at flat index k: every corner, border and interior window; one-row and
    one-column maps pad two opposite sides of every window."""
    _check(R.sweep(shape), want=np.arange(shape[0] * shape[1]))


@pytest.mark.parametrize('b', R.BOUNDARY_SHAPES, ids=lambda b: '%dx%d%s' % (b.h, b.w, '_misaligned' if b.misaligned else ''))
def test_peak_at_every_slice_and_loop_boundary(b):
    """One map, three maps and all positions as one batch: peaks at both ends, around every multiple of 1024 and 4096 elements (the
    unrolled loop's trips and its hand-over to the tail loop) and around every slice start, in the vector kernel, the scalar kernel
    with more than one slice, and the scalar kernel on a vector-sized map whose base is offset by one float."""
    for n_maps, pos in R.boundary_batches(b):
        heat = R.peaked(np.random.default_rng(n_maps + b.h), b.h, b.w, pos)
        dev = None
        if b.misaligned:
            buf = torch.zeros(heat.size + 1, dtype=torch.float32, device='cuda')
            buf[1:] = torch.from_numpy(heat.reshape(-1)).cuda()
            dev = buf[1:].view(heat.shape)
            assert dev.data_ptr() % 16 == 4 and dev.is_contiguous()
        else:
            dev = torch.from_numpy(heat).cuda()
            assert dev.data_ptr() % 16 == 0
        _check(heat, dev, want=pos)


@pytest.mark.parametrize('shape', R.SPECIAL_SHAPES, ids=lambda s: '%dx%d' % s)
def test_ties_and_special_values(shape):
    """Equal maxima across slices, waves and lanes resolve to the first index; a constant, an all -inf and an all-NaN map give 0; +inf
    wins over finite values, NaN over +inf wherever it sits, the first NaN over later ones; +0.0 and -0.0 tie."""
    heat, names = R.specials(*shape)
    t = torch.from_numpy(heat).cuda()
    _, idx, _ = refine.refine_device(t, shape[1], shape[0], _lib.REFINE_TABLE)
    got = idx.cpu().numpy()
    wrong = [(s.name, int(g), s.want) for s, g in zip(names, got) if g != s.want]
    assert not wrong, wrong
    _check(heat, t, want=[s.want for s in names])
    # each map alone as well: with one map the launch is the same, but no neighbour's partials sit beside its own
    for k in (0, len(names) - 1):
        _check(heat[k:k + 1], want=[names[k].want])


@pytest.mark.parametrize('n_maps', R.COUNT_TAILS)
def test_map_count_tails(n_maps):
    """8x8 maps, peak of map k at k % 64: the 64-lane block tail of the fit kernel, 2048 / n_maps at 2, 1 and 0.  Every map's
    refined position is finite and inside its map, visibility exactly 1."""
    heat = R.count_maps(n_maps)
    # the restated launch arithmetic is the library's: the workspace the header's function states follows from the slice count
    assert _lib.load().ttup_refine_workspace_bytes(n_maps, 8, 8) == R.workspace_bytes(n_maps, 8, 8)
    _check(heat, want=np.arange(n_maps) % 64)
    out, idx, _ = refine.refine_device(torch.from_numpy(heat).cuda(), 8, 8, _lib.REFINE_TABLE)
    out = out.cpu().numpy()
    assert out.shape == (n_maps, 3) and np.isfinite(out).all() and (out[:, 2] == 1.0).all()
    # the oracle's fit on the first map and on the first and last map of the last 64-lane block (its tail lanes), by the per-window
    # rule; image size = map size, so `out` is in heatmap pixels
    pick = sorted(set([0, n_maps - 1, (n_maps - 1) // 64 * 64]))
    ref = refine_ref.extract_position(heat[pick][:, None], 8, 8, refine_ref.TABLE)[:, 0]
    _, rw = refine_ref.argmax_window(heat[pick])
    bar = R.fit_bar(_fit_radius(rw, refine_ref.TABLE))
    err = np.abs(out[pick, :2] - ref[:, :2]).max(1)
    assert (err <= bar).all(), (pick, err, bar)


@pytest.mark.parametrize('n_maps,slices', R.COUNT_BIG)
def test_slice_count_bounded_by_map_size_and_by_count(n_maps, slices):
    h, w = 64, 128
    assert R.pick_nblk(n_maps, h * w) == slices and _lib.load().ttup_refine_workspace_bytes(n_maps, h, w) == R.workspace_bytes(n_maps, h, w)
    rng = np.random.default_rng(n_maps)
    pos = rng.integers(0, h * w, n_maps)
    pos[:4] = (0, h * w - 1, 4096, 4095)
    _check(R.peaked(rng, h, w, pos), want=pos)


def _raw_refine(heat_dev, n, h, w, variant, out, idx, win, ws, ws_bytes):
    lib = _lib.load()
    return lib.ttup_refine(_lib.ptr(heat_dev), n, h, w, 1920, 1080, variant, _lib.ptr(out), _lib.ptr(idx), _lib.ptr(win), _lib.ptr(ws), ws_bytes, _lib.stream_ptr())


@pytest.mark.parametrize('shape,n_maps', [((64, 128), 5), ((91, 91), 3), ((12, 14), 70)], ids=['64x128', '91x91', '12x14'])
def test_entry_points_agree_and_the_stated_workspace_suffices(shape, n_maps):
    """ttup_refine with null index and window outputs stages both in its workspace: same `out` bits as with both given, in a workspace
    of exactly the size the header's function states (guard bytes behind it stay untouched); one byte less is refused and nothing
    is written; ttup_refine_windows on the returned (index, window) gives the same bits again."""
    h, w = shape
    lib = _lib.load()
    rng = np.random.default_rng(h)
    heat = R.peaked(rng, h, w, rng.integers(0, h * w, n_maps))
    heat += (0.3 * rng.uniform(size=heat.shape)).astype(np.float32)          # windows that are no two alike
    t = torch.from_numpy(heat).cuda()
    need = lib.ttup_refine_workspace_bytes(n_maps, h, w)
    assert need == R.workspace_bytes(n_maps, h, w)
    guard = 256
    for variant in (_lib.REFINE_BALL, _lib.REFINE_TABLE):
        full = torch.full((n_maps, 3), -7.0, dtype=torch.float64, device='cuda')
        idx = torch.full((n_maps,), -1, dtype=torch.int64, device='cuda')
        win = torch.full((n_maps, 9), -7.0, dtype=torch.float32, device='cuda')
        ws = torch.full((need + guard,), 0x5a, dtype=torch.uint8, device='cuda')
        assert _raw_refine(t, n_maps, h, w, variant, full, idx, win, ws, need) == _lib.OK
        ri, rw = refine_ref.argmax_window(heat)
        assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(_bits(win.cpu().numpy().reshape(n_maps, 3, 3)), _bits(rw))
        assert (ws[need:] == 0x5a).all()
        # null outputs: staged in the workspace
        staged = torch.full((n_maps, 3), -7.0, dtype=torch.float64, device='cuda')
        ws2 = torch.full((need + guard,), 0x5a, dtype=torch.uint8, device='cuda')
        assert _raw_refine(t, n_maps, h, w, variant, staged, None, None, ws2, need) == _lib.OK
        assert (ws2[need:] == 0x5a).all()
        assert torch.equal(staged.view(torch.int64), full.view(torch.int64))
        assert (full[:, 2] == 1.0).all() and torch.isfinite(full).all()
        # one byte short: refused, nothing written
        short = torch.full((n_maps, 3), -7.0, dtype=torch.float64, device='cuda')
        ws3 = torch.full((need + guard,), 0x5a, dtype=torch.uint8, device='cuda')
        assert _raw_refine(t, n_maps, h, w, variant, short, None, None, ws3, need - 1) == _lib.EINVAL
        assert b'workspace' in lib.ttup_last_error()
        torch.cuda.synchronize()
        assert (short == -7.0).all() and (ws3 == 0x5a).all()
        # the second half alone
        again = refine.refine_windows_device(idx, win, h, w, 1920, 1080, variant)
        assert torch.equal(again.view(torch.int64), full.view(torch.int64))


@pytest.mark.parametrize('variant', [R.BALL, R.TABLE], ids=['ball', 'table'])
def test_fit_kernel_tracks_scipy_on_the_edge_windows(variant):
    """refine_windows_device on the 24 edge windows against the reference's scipy answers, with the rescaling to image pixels at
    non-integer scales (1920 / 14, 1080 / 12) undone in float64 for the comparison in heatmap pixels; visibility exactly 1.  The
    peak index goes through float32 as in the reference; indices here are exact in float32."""
    names, wins, ref, ok, rad = R.reference_fits(variant, _fit_radius)
    n, h, w, iw, ih = len(names), 12, 14, 1920, 1080
    idx = (np.arange(n) * 7) % (h * w)
    got = refine.refine_windows_device(torch.from_numpy(idx.astype(np.int64)).cuda(), torch.from_numpy(wins.reshape(n, 9)).cuda(), h, w, iw, ih, variant).cpu().numpy()
    assert got.shape == (n, 3) and (got[:, 2] == 1.0).all()
    # the oracle's rescaling of scipy's offsets (oracle/refine_ref.extract_position)
    want = np.stack([((np.float64(np.float32(idx % w)) - 1 + ref[:, 0]) + 0.5) * (iw / w) - 0.5,
                     ((np.float64(np.float32(idx // w)) - 1 + ref[:, 1]) + 0.5) * (ih / h) - 0.5], axis=1)
    err = (np.abs(got[:, :2] - want) / np.array([iw / w, ih / h])).max(1)          # heatmap pixels
    bar = R.fit_bar(rad)
    worst = int(np.argmax(err / bar))
    share = float((rad > R.ILL_POSED_RADIUS).mean())
    print('\n[%s] worst window %s: %.3e px, bar %.3e; share of windows with a radius above %g px: %.3f'
          % ('ball' if variant == R.BALL else 'table', names[worst], err[worst], bar[worst], R.ILL_POSED_RADIUS, share))
    assert (err <= bar).all(), [(k, e, b) for k, e, b in zip(names, err, bar) if e > b]
