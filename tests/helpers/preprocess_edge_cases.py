"""The pre-processing kernels' edge sweep (csrc/conv_pointwise.h: preprocess_kernel<float>, preprocess_kernel<bf16_t>,
preprocess_frames4_kernel): the shapes at which the fixed-point INTER_LINEAR resize changes path, their seeded clips and the oracle's
answers (oracle/glue_ref.py).  Shared by tests/test_preprocess_edges_host.py (CPU: the table holds what it claims) and
tests/test_preprocess_edges_gpu.py (the kernels against the oracle, bit for bit).

What a shape reaches, in the kernel's terms (one thread per output pixel, 256 columns per workgroup):

  left / right clamp    axis_tap_x: the source position falls before column 0 / at or behind the last column; the coefficient is reset
                        to (2048, 0).  Upscaling reaches both; so does a one-pixel source axis
  top / bottom clamp    axis_tap_y: the ROW index is clamped, the coefficient is not -- both taps read the same row with (c0, c1),
                        c1 != 0.  That is OpenCV's vertical pass, and what separates it from the horizontal one
  a1 == 0 / b1 == 0     a tap with weight 0 is not loaded: equal widths (every x tap is (2048, 0)), integer row positions
  (1024, 1024)          exact 2x downscale
  last pixel            the three channel bytes come in one 4-byte load; only the clip's last pixel falls back to byte loads
  column tails          output widths 255 / 256 / 257: one block with an idle lane, one full block, a second block of one lane
"""
import collections
import functools

import numpy as np

from oracle import glue_ref

Case = collections.namedtuple('Case', 'id sh sw dh dw group')


def _case(group, sh, sw, dh, dw):
    return Case('%dx%d_to_%dx%d' % (sh, sw, dh, dw), sh, sw, dh, dw, group)


CASES = [
    _case('down', 45, 70, 32, 48),           # 1: non-integer downscale on both axes
    _case('up', 24, 40, 32, 56),             # 2: upscale on both axes: all four clamps
    _case('x2', 64, 96, 32, 48),             # 3: exact 2x down, coefficients (1024, 1024)
    _case('x2', 16, 24, 32, 48),             #    exact 2x up
    _case('one_axis', 36, 48, 32, 48),       # 4: equal widths: x taps (2048, 0), the second column tap is never loaded
    _case('one_axis', 32, 50, 32, 48),       #    equal heights: integer rows, b1 == 0
    _case('one_axis', 32, 48, 32, 48),       #    identity
    _case('odd', 33, 51, 32, 48),            # 5: odd source sizes: every row starts at another alignment of the 4-byte loads
    _case('odd', 31, 49, 40, 64),
    _case('one_pixel', 1, 1, 8, 8),          # 6: one-pixel axes, source and output
    _case('one_pixel', 5, 1, 8, 8),
    _case('one_pixel', 1, 5, 8, 8),
    _case('one_pixel', 9, 13, 1, 1),
    _case('one_pixel', 9, 13, 1, 16),
    _case('one_pixel', 9, 13, 16, 1),
    _case('tails', 20, 300, 8, 255),         # 7: column-block tails
    _case('tails', 20, 300, 8, 256),
    _case('tails', 20, 300, 8, 257),
]
BY_ID = {c.id: c for c in CASES}
N_FRAMES = 4          # per case: preprocess_triples gives 2 samples, preprocess_frames 4
# 8: cases whose LAST output pixel reads the clip's last source pixel (asserted by the host test): the upscale clamps both axes
# there, the identity copies it, and at equal widths the bottom row's second tap is the last row
LAST_PIXEL_IDS = ('24x40_to_32x56', '32x48_to_32x48', '36x48_to_32x48')
# 9: the smallest clips (3 frames for triples: one sample; 1 frame for single frames), on a downscale, an upscale and an odd source
SMALLEST_IDS = ('45x70_to_32x48', '24x40_to_32x56', '31x49_to_40x64')
# the float64 bilinear cross-check of the oracle itself runs at cases 2, 3 and 6
BILINEAR_GROUPS = ('up', 'x2', 'one_pixel')


def seed_of(case):
    return 1000 + CASES.index(BY_ID[case.id])


@functools.lru_cache(maxsize=None)
def frames(case, n=N_FRAMES):
    """(n, sh, sw, 3) uint8, seeded uniform noise: every grey level next to every other, so a one-level error shows."""
    a = np.random.default_rng(seed_of(case)).integers(0, 256, (n, case.sh, case.sw, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


def last_pixel_frames(case, n=N_FRAMES):
    """The case's clip with a dark last frame whose last pixel alone is 255."""
    a = frames(case, n).copy()
    a[-1] = 0
    a[-1, -1, -1, :] = 255
    return a


def oracle_frames(clip, case):
    """(n, 3, dh, dw) float32: what wasb.preprocess_frames must return, bit for bit."""
    return np.stack([glue_ref.normalize_image(glue_ref.resize_linear_u8(f, case.dw, case.dh)).transpose(2, 0, 1).astype(np.float32) for f in clip])


def oracle_triples(clip, case):
    """(n - 2, 9, dh, dw) float32: what wasb.preprocess_triples must return, bit for bit."""
    return np.stack([glue_ref.triple_to_tensor(clip[i], clip[i + 1], clip[i + 2], (case.dw, case.dh)) for i in range(len(clip) - 2)])


# ------------------------------------------------------------------------------------------ what a case reaches
def raw_positions(src_n, dst_n):
    """floor of the float32 source position of every output index, before any clamp (cv::resize: fx = (float)((dx + 0.5) * scale - 0.5))."""
    f = ((np.arange(dst_n) + 0.5) * (src_n / dst_n) - 0.5).astype(np.float32)
    return np.floor(f).astype(np.int64)


def reach(case):
    """The branches the case's shape takes, from the oracle's own tap tables.  The identity takes none: the oracle copies and the
    kernel's `same` path reads one pixel."""
    out = dict.fromkeys(('left', 'right', 'top_c1', 'bottom_c1', 'all_a1_zero', 'all_b1_zero', 'half_half', 'last_reads_last'), False)
    if (case.sh, case.sw) == (case.dh, case.dw):
        out['last_reads_last'] = True
        return out
    x0, x1, a0, a1 = glue_ref._axis_taps(case.sw, case.dw)
    y0, y1, b0, b1 = glue_ref._axis_taps_v(case.sh, case.dh)
    sx, sy = raw_positions(case.sw, case.dw), raw_positions(case.sh, case.dh)
    left, right = sx < 0, sx >= case.sw - 1
    # the horizontal clamp resets the coefficient
    assert (a1[left | right] == 0).all() and (a0[left | right] == 2048).all() and (x0[left] == 0).all() and (x0[right] == case.sw - 1).all()
    top, bottom = sy < 0, sy + 1 > case.sh - 1
    # the vertical clamp moves the rows only
    assert (y0[top] == 0).all() and (y1[top] == 0).all() and (y0[bottom] == case.sh - 1).all() and (y1[bottom] == case.sh - 1).all()
    out['left'], out['right'] = bool(left.any()), bool(right.any())
    out['top_c1'], out['bottom_c1'] = bool((b1[top] != 0).any()), bool((b1[bottom] != 0).any())
    out['all_a1_zero'], out['all_b1_zero'] = bool((a1 == 0).all()), bool((b1 == 0).all())
    out['half_half'] = bool((a0 == 1024).all() and (a1 == 1024).all() and (b0 == 1024).all() and (b1 == 1024).all())
    # the last output pixel reads source pixel (sh - 1, sw - 1) with a non-zero weight
    wx = (a0[-1] if x0[-1] == case.sw - 1 else 0) + (a1[-1] if x1[-1] == case.sw - 1 else 0)
    wy = (b0[-1] if y0[-1] == case.sh - 1 else 0) + (b1[-1] if y1[-1] == case.sh - 1 else 0)
    out['last_reads_last'] = bool(wx > 0 and wy > 0)
    return out


# ------------------------------------------------------------------------------------------ an independent bilinear
def bilinear_f64(img, dw, dh):
    """Exact float64 bilinear resize of an (H, W, C) image with half-pixel centres and edge replication: what the 11-bit fixed-point
    scheme approximates.  Written from the definition; it shares nothing with the oracle's tap tables."""
    img = np.asarray(img, np.float64)
    h, w, _ = img.shape

    def axis(src_n, dst_n):
        p = (np.arange(dst_n, dtype=np.float64) + 0.5) * src_n / dst_n - 0.5
        p = np.clip(p, 0.0, src_n - 1.0)          # replicate the edge: outside the centres of the first / last pixel the image is constant
        i0 = np.minimum(np.floor(p).astype(np.int64), src_n - 1)
        return i0, np.minimum(i0 + 1, src_n - 1), p - i0

    y0, y1, fy = axis(h, dh)
    x0, x1, fx = axis(w, dw)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = img[y0][:, x0] * (1 - fx) + img[y0][:, x1] * fx
    bot = img[y1][:, x0] * (1 - fx) + img[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def smooth_image(case, rng):
    """The image kind of tests/test_oracle_golden.py::test_resize_unpinned_agrees_with_an_independent_bilinear: 8x8 blocks of random
    levels plus noise of sigma 6."""
    h, w = case.sh, case.sw
    smooth = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3)).astype(np.float64)
    return np.clip(np.kron(smooth, np.ones((8, 8, 1)))[:h, :w] + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------ fast path against general path
# preprocess_frames4_kernel: 4 pixels per thread, 1024 per workgroup, 4 rows per workgroup.  Network widths below one block, one
# record short of a block, one block, one record past it; source rows upscaled, downscaled, identical
FAST_WIDTHS = (8, 1016, 1024, 1032)
FAST_NET_H = 32
FAST_SRC_H = (24, 36, 32)
