"""CPU side of the pre-processing edge sweep (tests/helpers/preprocess_edge_cases.py): the case table reaches the branches it
claims, read from the oracle's own tap tables (oracle/glue_ref.py), and the oracle's fixed-point resize agrees with an exact float64
bilinear at the upscaling, exact-2x and one-pixel cases, by the bar of
tests/test_oracle_golden.py::test_resize_unpinned_agrees_with_an_independent_bilinear."""
import numpy as np
import pytest

from helpers import preprocess_edge_cases as P
from oracle import glue_ref


def test_case_table_reaches_every_branch():
    reach = {c.id: P.reach(c) for c in P.CASES}
    for key in ('left', 'right', 'top_c1', 'bottom_c1', 'all_a1_zero', 'all_b1_zero', 'half_half'):
        hit = [i for i, r in reach.items() if r[key]]
        print('%-12s %s' % (key, ' '.join(hit)))
        assert hit, key
    # what the table says about single cases
    up = reach['24x40_to_32x56']
    assert up['left'] and up['right'] and up['top_c1'] and up['bottom_c1']
    assert reach['64x96_to_32x48']['half_half'] and not reach['16x24_to_32x48']['half_half']
    assert reach['36x48_to_32x48']['all_a1_zero'] and not reach['36x48_to_32x48']['all_b1_zero']
    assert reach['32x50_to_32x48']['all_b1_zero'] and not reach['32x50_to_32x48']['all_a1_zero']
    x0, x1, a0, a1 = glue_ref._axis_taps(48, 48)
    assert (a0 == 2048).all() and (a1 == 0).all() and np.array_equal(x0, np.arange(48))
    for cid in P.LAST_PIXEL_IDS:
        assert reach[cid]['last_reads_last'], cid
    for cid in P.SMALLEST_IDS:
        assert cid in P.BY_ID
    # one-pixel source axes clamp every output index on both sides at once
    y0, y1, b0, b1 = glue_ref._axis_taps_v(1, 8)
    assert (y0 == 0).all() and (y1 == 0).all() and (b1 != 0).any()
    x0, x1, a0, a1 = glue_ref._axis_taps(1, 8)
    assert (x0 == 0).all() and (x1 == 0).all() and (a0 == 2048).all() and (a1 == 0).all()
    # column-block tails: one lane idle, none, one lane of a second block
    assert sorted(c.dw for c in P.CASES if c.group == 'tails') == [255, 256, 257]
    assert any(c.sw % 2 == 1 and c.sh % 2 == 1 for c in P.CASES if c.group == 'odd')
    assert len({c.id for c in P.CASES}) == len(P.CASES) and P.N_FRAMES >= 4


def test_vertical_clamp_keeps_its_coefficient_and_the_result_differs():
    """The two clamps are not interchangeable: on the upscaling case, a vertical pass that reset its coefficient at the clamp (as the
    horizontal one does) gives other grey levels than the oracle on the clamped rows -- so a kernel that confuses them cannot pass
    the bit comparison.  (Both taps read the same row, but (b0 * v >> 16) + (b1 * v >> 16) truncates twice.)"""
    case = P.BY_ID['24x40_to_32x56']
    img = P.frames(case)[0]
    out = glue_ref.resize_linear_u8(img, case.dw, case.dh)
    y0, y1, b0, b1 = glue_ref._axis_taps_v(case.sh, case.dh)
    clamped = np.flatnonzero((y0 == y1) & (b1 != 0))
    assert clamped.size >= 2
    x0, x1, a0, a1 = glue_ref._axis_taps(case.sw, case.dw)
    s = img.astype(np.int64)
    hor = s[:, x0] * a0[None, :, None] + s[:, x1] * a1[None, :, None]
    reset = np.clip((((2048 * (hor[y0[clamped]] >> 4)) >> 16) + 2) >> 2, 0, 255)
    diff = (reset != out[clamped]).mean()
    print('rows %s: %.1f %% of the pixels differ by one level when the vertical clamp resets its coefficient' % (clamped.tolist(), 100 * diff))
    assert diff > 0.05
    # The converse does not hold: a horizontal pass that KEPT its coefficient at a clamp reads one column with (a0, a1), and nothing
    # is truncated between its two products, so v * a0 + v * a1 = 2048 v whenever a0 + a1 = 2048 -- which the rounding of f and 1 - f
    # gives for every f (on a tie one of the two rounds up, the other down).  Only the index clamp of the x axis can be observed.
    sx = P.raw_positions(case.sw, case.dw)
    f = (((np.arange(case.dw) + 0.5) * (case.sw / case.dw) - 0.5).astype(np.float32) - sx).astype(np.float32)
    k1 = np.rint(f * np.float32(2048)).astype(np.int64)
    k0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    right = sx >= case.sw - 1
    assert right.any() and (k1[right] != 0).any() and (k0 + k1 == 2048).all()
    for c in P.CASES:
        for n_src, n_dst, taps in ((c.sw, c.dw, glue_ref._axis_taps), (c.sh, c.dh, glue_ref._axis_taps_v)):
            _, _, c0, c1 = taps(n_src, n_dst)
            assert (c0 + c1 == 2048).all(), c.id


@pytest.mark.parametrize('case', [c for c in P.CASES if c.group in P.BILINEAR_GROUPS], ids=lambda c: c.id)
def test_oracle_resize_agrees_with_an_exact_bilinear(case):
    """Within one grey level of the float64 bilinear everywhere, equal to its rounding on more than 85 % of the values, mean distance
    below 0.3 (the bar of the existing test, on its kind of image)."""
    rng = np.random.default_rng(P.seed_of(case))
    img = P.smooth_image(case, rng)
    out = glue_ref.resize_linear_u8(img, case.dw, case.dh).astype(np.float64)
    ref = P.bilinear_f64(img, case.dw, case.dh)
    assert out.shape == ref.shape == (case.dh, case.dw, 3)
    d = np.abs(out - ref)
    share = (out == np.rint(ref)).mean()
    print('%s: max %.3f, mean %.3f, equal to the rounding on %.3f of %d values' % (case.id, d.max(), d.mean(), share, out.size))
    assert d.max() <= 1.0, (case.id, d.max())
    assert share > 0.85 and d.mean() < 0.3, (case.id, share, d.mean())


def test_bilinear_yardstick_is_the_one_the_existing_test_uses():
    """The numpy bilinear above equals torch's float64 bilinear (align_corners=False), the yardstick of the existing test, to
    rounding error -- on an upscale, a downscale and one-pixel axes."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    for (h, w, dh, dw) in ((24, 40, 32, 56), (45, 70, 32, 48), (1, 5, 8, 8), (9, 13, 1, 16)):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.float64)
        ref = F.interpolate(torch.from_numpy(img).permute(2, 0, 1)[None], size=(dh, dw), mode='bilinear', align_corners=False)[0].permute(1, 2, 0).numpy()
        assert np.abs(P.bilinear_f64(img, dw, dh) - ref).max() < 1e-9
