"""The peak refinement's edge sweep (csrc/refine.hip: argmax_partial_kernel<VEC>, argmax_finish_kernel, fit_kernel; csrc/lbfgsb.h):
the launch arithmetic restated, the heatmaps that put a peak on every boundary that arithmetic creates, the ties and special values,
and the 24 fit windows per variant.  Shared by tests/test_refine_edges_host.py (CPU) and tests/test_refine_edges_gpu.py.

Launch arithmetic (refine_argmax): a map of hw floats is cut into nblk slices of whole QUADS (4 floats), slice b = quads
[quads * b / nblk, quads * (b + 1) / nblk), one 256-thread workgroup each; nblk = pick_nblk(n_maps, hw).  The vector kernel
(hw % 4 == 0 and a 16-byte aligned base) reads quad q0 + tid + 256 * k: four quads per lane and trip while q + 768 < q1, then one
at a time -- 1024 quads = 4096 elements per unrolled trip.  The scalar kernel reads element q0 * 4 + tid + 256 * k.  Partials are
reduced per wave (64 lanes), across the 4 waves through LDS, and across slices by argmax_finish_kernel, which also gathers the
zero-padded 3x3 window.
"""
import collections

import numpy as np

BALL, TABLE = 0, 1


# ------------------------------------------------------------------------------------------ the launch arithmetic, restated
def pick_nblk(n_maps, hw):
    nblk = 2048 // max(n_maps, 1)
    nblk = min(nblk, max(hw // 4096, 1))
    return min(max(nblk, 1), 1024)


def slice_starts(n_maps, hw):
    """First ELEMENT of every slice (the first one included)."""
    quads, nblk = (hw + 3) // 4, pick_nblk(n_maps, hw)
    return [4 * (quads * b // nblk) for b in range(nblk)]


def workspace_bytes(n_maps, h, w):
    """include/ttup.h ttup_refine_workspace_bytes: partials (12 bytes per slice) + index and window staging + 256."""
    return n_maps * pick_nblk(n_maps, h * w) * 12 + n_maps * 44 + 256


# ------------------------------------------------------------------------------------------ heatmaps
NOISE_LO, NOISE_HI, PEAK = -1.0, -0.125, 4.0          # noise stays negative: +0.0 and -0.0 are maxima where they are planted


def noise(rng, n, h, w):
    return rng.uniform(NOISE_LO, NOISE_HI, (n, h, w)).astype(np.float32)


def peaked(rng, h, w, positions):
    """One map per entry of `positions`: noise with the single peak at that flat index."""
    heat = noise(rng, len(positions), h, w)
    heat.reshape(len(positions), -1)[np.arange(len(positions)), np.asarray(positions)] = PEAK
    return heat


# every position of every small shape: all corner, border and interior windows; H == 1 or W == 1 pads two opposite sides at once
SWEEP_SHAPES = ((1, 1), (1, 4), (1, 7), (7, 1), (2, 2), (3, 3), (5, 8), (12, 14))


def sweep(shape):
    h, w = shape
    return peaked(np.random.default_rng(100 * h + w), h, w, np.arange(h * w))


# slice and loop boundaries.  want: the slice count the shape must give while n_maps <= 2048 / want
Boundary = collections.namedtuple('Boundary', 'h w vec slices misaligned')
BOUNDARY_SHAPES = (
    Boundary(64, 128, True, 2, False),          # 2048 quads: two slices of 1024 = one unrolled trip each, no tail trip
    Boundary(96, 128, True, 3, False),          # three slices of exactly 1024 quads
    Boundary(100, 124, True, 3, False),         # 3100 quads in slices of 1033, 1033, 1034: one unrolled trip and a tail of 9 / 10 quads
    Boundary(91, 91, False, 2, False),          # hw = 8281 (odd): scalar kernel, 2071 quads -> slices start at 0 and 4140; the last quad is one element
    Boundary(127, 129, False, 3, False),        # hw = 16383: scalar, three slices
    Boundary(64, 128, False, 2, True),          # hw % 4 == 0 but the base is offset by one float: scalar kernel
)


def boundary_positions(b, n_maps, n_random=6):
    """Flat peak positions for one boundary shape: both ends, every multiple of 1024 elements and the element before it, every
    multiple of 4096 +- 1, every slice's first element and the one before it, a few seeded ones."""
    hw = b.h * b.w
    pos = {0, hw - 1}
    for m in range(1024, hw, 1024):
        pos |= {m, m - 1}
    for m in range(4096, hw, 4096):
        pos |= {m - 1, m + 1}
    for s in slice_starts(n_maps, hw)[1:]:
        pos |= {s, s - 1}
    rng = np.random.default_rng(hw)
    pos |= set(int(v) for v in rng.integers(0, hw, n_random))
    return sorted(p for p in pos if 0 <= p < hw)


def boundary_batches(b):
    """-> [(n_maps, positions)]: one map, three maps, and every position as one batch (which keeps the slice count)."""
    hw = b.h * b.w
    full = boundary_positions(b, 1)
    assert len(full) <= 2048 // b.slices
    starts = slice_starts(1, hw)
    return [(1, [starts[-1]]), (3, [starts[1] - 1, 0, hw - 1]), (len(full), boundary_positions(b, len(full)))]


# ties and special values, on a vector and a scalar shape
SPECIAL_SHAPES = ((64, 128), (91, 91))
Special = collections.namedtuple('Special', 'name want')          # want: the index argmax must return (numpy / torch semantics)


def specials(h, w):
    """-> (heat (n, h, w) float32, [Special]).  Lane of an element: (e / 4 - q0) % 256 in the vector kernel, (e - 4 * q0) % 256 in the
    scalar one; wave = lane / 64.  The pairs below are ties in BOTH readings where the name says so."""
    hw = h * w
    second = slice_starts(1, hw)[1]          # first element of the second slice
    rng = np.random.default_rng(7 * hw)
    maps, names = [], []

    def add(name, want, fill):
        m = noise(rng, 1, h, w)[0]
        fill(m.reshape(-1))
        maps.append(m)
        names.append(Special(name, want))

    def put(pairs):
        def fill(f):
            for i, v in pairs:
                f[i] = v
        return fill

    inf, nan = np.float32(np.inf), np.float32(np.nan)
    # two equal maxima in different slices, the first one late in its slice and the second one early in its own
    add('tie_slices', second - 3, put([(second - 3, PEAK), (second + 5, PEAK)]))
    add('tie_slices_far', 17, put([(17, PEAK), (hw - 1, PEAK)]))
    # different waves of one workgroup, the SMALLER index in the HIGHER wave: vector lanes 70 (wave 1) and 5 (wave 0, second trip of
    # the tail loop or second quad of the unrolled one); scalar lanes 70 and 5
    add('tie_waves_vec', 280, put([(280, PEAK), (4 * (256 + 5), PEAK)]))
    add('tie_waves_scalar', 70, put([(70, PEAK), (256 + 5, PEAK)]))
    add('tie_waves_last', 4 * 200 + 1, put([(4 * 200 + 1, PEAK), (4 * (512 + 3) + 2, PEAK)]))          # waves 3 and 0
    # neighbouring lanes: same trip (the smaller index in the lower lane) and across trips (the smaller index in the higher lane)
    add('tie_lanes_vec', 400, put([(400, PEAK), (404, PEAK)]))
    add('tie_lanes_scalar', 401, put([(401, PEAK), (402, PEAK)]))
    add('tie_lanes_vec_wrap', 4, put([(4, PEAK), (1024, PEAK)]))
    add('tie_lanes_scalar_wrap', 1, put([(1, PEAK), (256, PEAK)]))
    add('tie_same_quad', 2001, put([(2001, PEAK), (2002, PEAK), (2003, PEAK)]))
    add('constant', 0, lambda f: f.fill(0.25))
    add('all_neg_inf', 0, lambda f: f.fill(-inf))
    add('one_pos_inf', second + 77, put([(second + 77, inf), (3, PEAK)]))
    add('nan_after_inf', second + 9, put([(5, inf), (second + 9, nan)]))          # +inf in the first slice, NaN in the second: NaN wins
    add('nan_before_inf', 6, put([(6, nan), (second + 9, inf)]))
    add('two_nans', 123, put([(123, nan), (second + 1, nan), (hw - 1, PEAK)]))
    add('two_nans_one_slice', 1030, put([(1030, nan), (1031, nan)]))
    add('all_nan', 0, lambda f: f.fill(nan))
    add('pos_zero_then_neg_zero', 40, put([(40, np.float32(0.0)), (second + 40, np.float32(-0.0))]))
    add('neg_zero_then_pos_zero', 41, put([(41, np.float32(-0.0)), (second + 41, np.float32(0.0))]))
    add('zeros_neighbours', 500, put([(500, np.float32(-0.0)), (501, np.float32(0.0))]))
    return np.stack(maps), names


# map-count tails: the 64-lane blocks of fit_kernel, grid.y of the partial kernel, 2048 / n_maps falling to 1 and to 0
COUNT_TAILS = (63, 64, 65, 1024, 1025, 2048, 2049)
COUNT_SHAPE = (8, 8)
COUNT_BIG = ((5, 2), (1500, 1))          # 64x128: (n_maps, slices): bounded by the map size / by the count


def count_maps(n_maps, shape=COUNT_SHAPE):
    h, w = shape
    return peaked(np.random.default_rng(n_maps), h, w, np.arange(n_maps) % (h * w))


# ------------------------------------------------------------------------------------------ fit windows
def _gauss(cx, cy, sigma, amp=1.0):
    y, x = np.meshgrid(np.arange(3.0), np.arange(3.0), indexing='ij')
    return (amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma ** 2))).astype(np.float32)


def _masked(win, rows, cols):
    """The window of a peak at a map border: the rows / columns outside the map are zero padding."""
    out = np.zeros((3, 3), np.float32)
    out[np.ix_(rows, cols)] = win[np.ix_(rows, cols)]
    return out


def fit_windows():
    """24 finite 3x3 windows (centre = the map's maximum, as argmax_finish_kernel gathers them) and their names."""
    wins = collections.OrderedDict()
    blob = _gauss(1.0, 1.0, 1.0)
    off = _gauss(1.2, 0.9, 0.8)
    # corners: 4 of 9 entries inside the map
    wins['corner_top_left'] = _masked(blob, [1, 2], [1, 2])
    wins['corner_bottom_right'] = _masked(off, [0, 1], [0, 1])
    wins['corner_top_right'] = _masked(off, [1, 2], [0, 1])
    # edges: 6 of 9
    wins['edge_top'] = _masked(blob, [1, 2], [0, 1, 2])
    wins['edge_left'] = _masked(off, [0, 1, 2], [1, 2])
    wins['edge_bottom'] = _masked(off, [0, 1], [0, 1, 2])
    # H == 1 / W == 1: 3 of 9
    wins['row_map'] = _masked(blob, [1], [0, 1, 2])
    wins['row_map_off'] = _masked(_gauss(1.3, 1.0, 0.7), [1], [0, 1, 2])
    wins['column_map'] = _masked(blob, [0, 1, 2], [1])
    # a 1x1 map: a single non-zero pixel
    wins['single_pixel'] = _masked(blob, [1], [1])
    wins['constant_quarter'] = np.full((3, 3), 0.25, np.float32)
    # raw logits: every entry negative, the centre the least
    wins['all_negative'] = (-3.0 + _gauss(1.0, 1.0, 1.0)).astype(np.float32)
    # peak heights
    wins['height_1e-3'] = _gauss(1.1, 0.9, 1.0, 1e-3)
    wins['height_1'] = _gauss(1.1, 0.9, 1.0, 1.0)
    wins['height_60'] = _gauss(1.1, 0.9, 1.0, 60.0)
    # two equal maxima on a diagonal with a dip between them
    saddle = np.full((3, 3), 0.2, np.float32)
    saddle[0, 0] = saddle[2, 2] = 1.0
    saddle[1, 1] = 0.5
    wins['saddle'] = saddle
    # amplitude-1 Gaussians at and between pixels
    for sigma in (0.5, 1.0, 3.0):
        wins['gauss_s%g_at' % sigma] = _gauss(1.0, 1.0, sigma)
        wins['gauss_s%g_between' % sigma] = _gauss(1.5, 1.0, sigma)
    wins['gauss_s1_diag'] = _gauss(1.25, 1.25, 1.0)
    wins['gauss_s0.5_diag'] = _gauss(0.75, 1.25, 0.5)
    names = list(wins)
    out = np.stack([wins[k] for k in names])
    assert out.shape == (24, 3, 3) and np.isfinite(out).all()
    return names, out


ILL_POSED_RADIUS = 1e-3          # px: a window whose scipy answer moves further under one-ulp changes of exp() says little
ILL_POSED_SHARE = 0.25           # at most this share of a variant's windows


def fit_bar(radius):
    """tests/test_cabi.py's per-window rule: 1e-6 px or twice the radius of the reference's own answer, whichever is larger."""
    return np.maximum(1e-6, 2.0 * np.asarray(radius))


_REFERENCE = {}


def reference_fits(variant, fit_radius):
    """-> (names, windows (24, 3, 3), scipy offsets (24, 2), success (24,), radius (24,)): the reference's own fit of every window
    (oracle/refine_ref.fit_window, once per process) and how far that answer moves under one-ulp changes of exp(): `fit_radius` is
    tests/test_cabi.py::_fit_radius, handed in by the test."""
    if variant not in _REFERENCE:
        from oracle import refine_ref
        names, wins = fit_windows()
        fits = [refine_ref.fit_window(w, variant) for w in wins]
        _REFERENCE[variant] = (names, wins, np.array([f[:2] for f in fits]), np.array([f[2] for f in fits]), fit_radius(wins, variant))
    return _REFERENCE[variant]
