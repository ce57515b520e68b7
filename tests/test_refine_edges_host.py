"""CPU side of the peak refinement's edge sweep (tests/helpers/refine_edge_cases.py): the restated launch arithmetic gives the slice
counts and boundaries the case table claims, the special-value maps have the answers the table states under numpy's and torch's
argmax, and the host build of csrc/lbfgsb.h -- the code every lane of fit_kernel runs -- agrees with the reference's scipy fit on
the 24 edge windows per variant, window by window, by the rule of tests/test_cabi.py: max(1e-6 px, 2 x _fit_radius)."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import refine_edge_cases as R
from oracle import refine_ref
from test_cabi import _fit_radius, host_fit  # noqa: F401  (host_fit: the fixture that builds tests/helpers/host_fit.cpp)


def test_launch_arithmetic_of_the_case_table():
    # what the suite reached before this sweep: one slice everywhere but at full size
    assert [R.pick_nblk(n, hw) for n, hw in ((51, 168), (3, 1961), (2, 4096))] == [1, 1, 1] and R.pick_nblk(6, 901120) == 220
    for b in R.BOUNDARY_SHAPES:
        hw = b.h * b.w
        assert (hw % 4 == 0 and not b.misaligned) == b.vec
        batches = R.boundary_batches(b)
        assert [n for n, _ in batches][:2] == [1, 3]
        for n_maps, pos in batches:
            assert R.pick_nblk(n_maps, hw) == b.slices and len(pos) == n_maps and len(set(pos)) == n_maps
        starts = R.slice_starts(1, hw)
        full = set(batches[-1][1])
        assert {0, hw - 1} <= full and all({s, s - 1} <= full for s in starts[1:])
        assert all({m, m - 1} <= full for m in range(1024, hw, 1024)) and all({m - 1, m + 1} <= full for m in range(4096, hw, 4096))
    quads = lambda hw: np.diff([s // 4 for s in R.slice_starts(1, hw)] + [(hw + 3) // 4]).tolist()
    assert quads(64 * 128) == [1024, 1024] and quads(96 * 128) == [1024, 1024, 1024] and quads(100 * 124) == [1033, 1033, 1034]
    assert R.slice_starts(1, 91 * 91) == [0, 4140] and len(R.slice_starts(1, 127 * 129)) == 3
    # map-count tails: 2048 / n_maps is 2, 1, 1, 0 (clamped to 1); the map size bounds 64x128 at 5 maps, the count at 1500
    assert [2048 // n for n in (1024, 1025, 2048, 2049)] == [2, 1, 1, 0]
    assert all(R.pick_nblk(n, 64) == 1 for n in R.COUNT_TAILS)
    assert [(R.pick_nblk(n, 64 * 128), want) for n, want in R.COUNT_BIG] == [(2, 2), (1, 1)]
    assert R.workspace_bytes(5, 64, 128) == 5 * 2 * 12 + 5 * 44 + 256


@pytest.mark.parametrize('shape', R.SPECIAL_SHAPES, ids=lambda s: '%dx%d' % s)
def test_special_maps_have_the_stated_answers_under_numpy_and_torch(shape):
    heat, names = R.specials(*shape)
    want = np.array([s.want for s in names])
    idx, win = refine_ref.argmax_window(heat)
    assert np.array_equal(idx, want), [(s.name, int(i)) for s, i in zip(names, idx) if i != s.want]
    assert np.array_equal(torch.argmax(torch.from_numpy(heat).view(len(names), -1), 1).numpy(), want)
    second = R.slice_starts(1, shape[0] * shape[1])[1]
    by = {s.name: s.want for s in names}
    assert by['tie_slices'] < second <= by['nan_after_inf'] and by['constant'] == by['all_neg_inf'] == by['all_nan'] == 0
    # the windows carry the special values themselves: compared as bits on the device
    k = [s.name for s in names].index('all_nan')
    assert np.isnan(win[k, 1:, 1:]).all() and (win[k, 0] == 0).all()


def test_sweep_maps_cover_every_position():
    for shape in R.SWEEP_SHAPES:
        heat = R.sweep(shape)
        idx, win = refine_ref.argmax_window(heat)
        assert np.array_equal(idx, np.arange(shape[0] * shape[1])) and (win[:, 1, 1] == R.PEAK).all()
    # a one-row map pads above AND below every window, a one-column map left and right
    _, win = refine_ref.argmax_window(R.sweep((1, 7)))
    assert (win[:, 0] == 0).all() and (win[:, 2] == 0).all()
    _, win = refine_ref.argmax_window(R.sweep((7, 1)))
    assert (win[:, :, 0] == 0).all() and (win[:, :, 2] == 0).all()


def test_fit_windows_are_what_the_table_says():
    names, wins = R.fit_windows()
    nz = {n: int((w != 0).sum()) for n, w in zip(names, wins)}
    assert [nz[k] for k in ('corner_top_left', 'corner_bottom_right', 'corner_top_right')] == [4, 4, 4]
    assert [nz[k] for k in ('edge_top', 'edge_left', 'edge_bottom')] == [6, 6, 6]
    assert [nz[k] for k in ('row_map', 'row_map_off', 'column_map', 'single_pixel')] == [3, 3, 3, 1]
    by = dict(zip(names, wins))
    assert (by['constant_quarter'] == 0.25).all() and (by['all_negative'] < 0).all()
    assert [float(by[k].max()) for k in ('height_1e-3', 'height_1', 'height_60')] == pytest.approx([1e-3, 1.0, 60.0], rel=0.03)
    assert (by['saddle'] == by['saddle'].max()).sum() == 2
    assert len(names) == len(set(names)) == 24 and np.isfinite(wins).all()


@pytest.mark.parametrize('variant', [R.BALL, R.TABLE], ids=['ball', 'table'])
def test_host_build_of_the_fit_tracks_scipy_on_the_edge_windows(host_fit, variant):  # noqa: F811
    names, wins, ref, ok, rad = R.reference_fits(variant, _fit_radius)
    n = len(names)
    out = np.zeros((n, 8))
    w = np.ascontiguousarray(wins.reshape(n, 9), np.float32)
    host_fit.ttup_host_fit(w.ctypes.data_as(ctypes.c_void_p), n, variant, out.ctypes.data_as(ctypes.c_void_p))
    err = np.abs(out[:, :2] - ref).max(1)
    bar = R.fit_bar(rad)
    worst = int(np.argmax(err / bar))
    share = float((rad > R.ILL_POSED_RADIUS).mean())
    print('\n[%s] worst window %s: %.3e px, bar %.3e; %d of %d windows have a radius above %g px (share %.3f); scipy reports success on %d'
          % ('ball' if variant == R.BALL else 'table', names[worst], err[worst], bar[worst], int((rad > R.ILL_POSED_RADIUS).sum()), n, R.ILL_POSED_RADIUS, share, int(ok.sum())))
    assert share <= R.ILL_POSED_SHARE, [(k, r) for k, r in zip(names, rad) if r > R.ILL_POSED_RADIUS]
    assert (err <= bar).all(), [(k, e, b) for k, e, b in zip(names, err, bar) if e > b]
    assert np.array_equal(out[:, 2] != 0, ok)
