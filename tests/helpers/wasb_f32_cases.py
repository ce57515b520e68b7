"""The fp32 CNN's tap-level edge sweep: the shapes at which conv_x3_kernel (csrc/conv_x3.hip) changes tile, trip or instance, the
restated launch arithmetic that says which case reaches what, the float64 oracle with fp32 storage (oracle/wasb_bf16_ref.py,
Weights(rounding='f32')) and the bounds of the teacher-forced comparison.  Shared by tests/test_wasb_f32_oracle.py (CPU) and
tests/test_wasb_f32_taps_gpu.py.  Weights, inputs, frames and statistics are those of tests/helpers/wasb_edge_cases.py.

The fp32 graph is the layer-by-layer one (csrc/wasb_graph.h fuses for bf16 only): every conv is one launch_conv_x3, every fuse sum
an upsum_kernel<float>, the head head_kernel<float, 16>, and stem1, stem2, layer1, trans1_*, stage2_*, stage3_*, stage4_0 are all
stored.  Tile arithmetic of launch_x3 (csrc = upliftingtabletennis_amd/csrc), by (k, stride) and (chunk width CK, couts per block
MT * 16):

  3x3 s1   8x32 output tiles, 8 waves; 4x32 for CK = 32 with MT = 4 (64 couts per block: the LDS budget)
  3x3 s2   CK = 32: 4x16 tiles, 4 waves (MT <= 2: at most 32 couts per block); CK = 16: 4x32 tiles, 8 waves
  1x1      8x32 tiles, 8 waves (CK = 32 only)
  LDS      2 * 3 * (round8(IH * IW * CK) + KSTEPS * MT * 512) bytes, IH = (TH - 1) * S + K, KSTEPS = K * K (CK = 32) or (K * K + 1) / 2
  grid.x   min(tiles, max(1, 256 * per_cu / cout_blocks)), per_cu = min(160 KB / LDS, 2 for 8 waves or 4 for 4 waves), at least 1
  grid.y   cout_blocks = cout / (MT * 16)

Trip t of workgroup g takes raster tile g + t * grid.x, image-major, with no XCD remap: the second and later trips are the TAIL of
the batch, so a case made for them checks the first and the last image.  A trip reuses the LDS image of the one before, and a
single-chunk conv (cin_total == CK) keeps the weights it staged with its first item (w_loaded / w_stored).

What is asserted per tap (bounds() below): device max <= M_MAX x spread max and <= 1e-5 of the tap's scale, device mean <= M_MEAN x
spread mean -- and <= M_MEAN_NOISE x spread mean on every case with noise weights, which is every case but the planted one --
where the spread is oracle(fp32, reversed K) - oracle(float64) on the same inputs.  No share of differing elements: in fp32 nearly
every element differs.
"""
import collections
import functools

import numpy as np
import torch

from helpers import wasb_edge_cases as E
from oracle import wasb_bf16_ref as R

SEGMENTS = E.SEGMENTS
TAPS = ('stem1', 'stem2', 'layer1', 'trans1_0', 'trans1_1', 'stage2_0', 'stage2_1', 'stage3_0', 'stage3_1', 'stage3_2', 'stage4_0')          # every one stored

# ------------------------------------------------------------------------------------------ bounds
# M_MAX / M_MEAN: what the device may reach in units of the spread, one value per statistic and kernel choice: 2 x the largest ratio
# measured on the MI355X over all cases of that choice (the margins of the bf16 sweep, 3 x max and 2 x mean, turned out too small
# for every choice).  Measured, device / spread per tap (largest; median over all taps of all cases):
#                         max                                    mean
#   x3      6.48 (72x104_frames trans1_1); 1.20     14.53 (72x104_frames trans1_0); 1.34      noise-weight cases alone: 4.99 (8x8 trans1_1) / 2.41 (136x24 trans1_1)
#   exact   3.38 (40x56 trans1_1);         1.35      2.17 (72x104_b8 trans1_0);      1.30
#   direct  3.71 (40x56 trans1_1);         1.21      2.08 (40x56 trans1_0);          1.31
# Where the excess sits: evenly over the plane -- per tap the ratio is the same to a few per cent on the border ring and inside it, in
# the first, middle and last third of rows and columns, on the last row and column, and on the first and the last image of the
# second-trip case -- and it grows with K alone: 0.95 at K = 144 (stem1), 1.1 .. 1.2 at K = 288, 1.5 at K = 576 (stem2), 2.0 .. 2.4
# at K = 1152 (trans1_*), for ALL THREE kernel choices alike, the one-thread-per-output fp32 fma chain included.  So it is the
# yardstick: torch's CPU convolution sums K in blocks and lands closer to float64 than a sequential fp32 chain does.  The split-bf16
# kernel sits another 1.8 x above its own arithmetic evaluated with round-to-nearest accumulation (six exact 32-channel partial sums
# per k-step added to an fp32 accumulator, restated on the CPU: 1.3 x the spread on trans1_0 where the device shows 2.1 x): the
# matrix pipe's accumulate does not round to nearest.  The planted net (72x104_frames) is its own kind: its identity path puts one
# large product per tap into the FIRST chunk of K, every later k-step then rounds at the large accumulator's ulp, and the split-bf16
# kernel (6 accumulator roundings per k-step over 36 k-steps) reaches 5 .. 15 x the spread on layer1 / trans1_* where the kernels
# that sum K in another order stay at 1.0 .. 2.7 x; the CPU restatement of the split-bf16 order shows the same (5.3 x with
# round-to-nearest).  Evenly spread as well (13.7 .. 15.0 x in every region of trans1_0).
# With M_MEAN['x3'] = 29 the bounds no longer catch a lost third bf16 part (6 .. 22 x the spread's mean, tests/test_wasb_f32_oracle.py).
# M_MEAN_NOISE keeps that guarantee on the noise-weight cases, where the ratio does not depend on where a large term sits in K: 2 x
# the largest ratio measured there.  It asks more than M_MEAN, never less.
KERNELS = ('x3', 'exact', 'direct')          # conv_x3_kernel (default) / TTUP_F32_EXACT=1 conv_f32_mfma_kernel / TTUP_F32_DIRECT=1 conv_direct_f32_kernel
KERNEL_ENV = {'x3': None, 'exact': 'TTUP_F32_EXACT', 'direct': 'TTUP_F32_DIRECT'}
M_MAX = {'x3': 12.96, 'exact': 6.76, 'direct': 7.42}
M_MEAN = {'x3': 29.06, 'exact': 4.34, 'direct': 4.16}
M_MEAN_NOISE = {'x3': 4.82, 'exact': 4.34, 'direct': 4.16}
CAP_MAX = 1e-5           # device max on every tap, whatever the spread: the whole chain's measured fp32 error is 1.3e-6 of range
CAP_SPREAD = 2e-6        # the spread of a case must stay below this on every tap, or another seed is chosen
Stats = E.Stats


def bounds(spread, kernels='x3', planted=False):
    m_mean = M_MEAN[kernels] if planted else min(M_MEAN[kernels], M_MEAN_NOISE[kernels])
    return Stats(min(CAP_MAX, M_MAX[kernels] * spread.max), m_mean * spread.mean, 1.0)


# ------------------------------------------------------------------------------------------ cases
def _case(id, h, w, batch, kind='ball', images=None, seed=0, planted=False):
    return E.Case(id, h, w, batch, kind, None, 'layerwise', tuple(range(batch)) if images is None else images, (), ('stem1', 'layer1', 'stage4_0'), seed, planted, ())


CASES = [
    # every plane is one partial tile: 8x8 / 4x4 / 2x2 / 1x1; at 1x1 every 3x3 tap but the centre is padding; the 1/8 term of the
    # stage-4 sum is upsampled by 8
    _case('8x8', 8, 8, 2, seed=71),
    # narrower than any tile (24 / 12 / 6 / 3 columns): 17, 9, 5 and 3 tile rows of 8, the last one 4 / 2 / 1 rows high at 1/2 .. 1/8
    _case('136x24', 136, 24, 2, seed=72),
    # one tile row of 8x32 at 1/1 .. 1/8 (24 / 12 / 6 / 3 rows); 264 = 8 * 32 + 8: nine tile columns, the last 8 wide
    _case('24x264', 24, 264, 2, seed=73),
    # interior tiles down to 1/8 resolution (25x37: 4x16 tiles 7 x 3, 4x32 tiles 7 x 2) with a ragged last row and column everywhere
    _case('200x296', 200, 296, 2, images=(0,), seed=74),
    # second and later persistent trips: 129 tile rows x 8 images = 1032 tiles at full resolution, 65 x 8 = 520 at 1/2 -- the
    # smallest height at which the 1x1 32 -> 16 fuse conv (grid.x = 512) takes a second trip; see coverage()
    _case('1032x8_b8', 1032, 8, 8, images=(0, 7), seed=75),
    # the table detector on uint8 frames: preprocess_kernel<float> writing NHWC16 with one frame per sample (3 channels padded to
    # 16), head_kernel<float, 16> with 13 maps
    _case('72x104_table', 72, 104, 3, kind='table', seed=76),
    # the ball detector on uint8 frames: preprocess_kernel<float> with three frames per sample, 6 frames of 80x104 resized to 72x104
    # (a real vertical interpolation); planted weights, so the argmax must equal the oracle's
    _case('72x104_frames', 72, 104, 4, kind='frames', seed=77, planted=True),
    # preprocess_kernel<float> writing NHWC16 at its own edges (source sizes: E.SOURCE_HW): 24x40 frames upscaled to 32x56 -- all four
    # clamps -- and frames of the network's size (the copy path), with three frames per sample and with one
    _case('32x56_pre_up_frames', 32, 56, 4, kind='frames', seed=82),
    _case('32x56_pre_up_table', 32, 56, 3, kind='table', seed=83),
    _case('32x56_pre_same_frames', 32, 56, 4, kind='frames', seed=84),
    _case('32x56_pre_same_table', 32, 56, 3, kind='table', seed=85),
]
BY_ID = {c.id: c for c in CASES}
# the cross-check kernels (each in a process of its own: csrc/conv.hip reads the switches once)
CROSS_CASES = [
    ('exact', _case('40x56_exact', 40, 56, 3, seed=78)),
    # conv_f32_mfma_kernel is persistent too (4x16 .. 16x16 tiles): 8 images, first and last checked
    ('exact', _case('72x104_b8_exact', 72, 104, 8, images=(0, 7), seed=79)),
    ('direct', _case('40x56_direct', 40, 56, 3, seed=78)),          # one thread per output, no tiles: one ragged case
]
MUTANT_SHAPES = [_case('40x56_mutants', 40, 56, 2, images=(0,), seed=80), _case('8x8_mutants', 8, 8, 2, images=(0,), seed=81)]


@functools.lru_cache(maxsize=2)
def oracle_weights(case):
    return R.Weights(E.state_dict(case), rounding='f32')


# ------------------------------------------------------------------------------------------ the launch arithmetic, restated
Conv = collections.namedtuple('Conv', 'name c0 c1 cout k stride div')          # div: the conv's INPUT plane is (H / div, W / div)
Launch = collections.namedtuple('Launch', 'conv instance tile waves oh ow tiles_y tiles_x tiles grid_x blocks trips')
CH = (16, 32, 64, 128)
TILES = {          # launch_conv_x3, the unpruned branches: (k, stride) -> {(CK, MT): (TH, TW, waves)}
    (3, 1): {(32, 1): (8, 32, 8), (32, 2): (8, 32, 8), (32, 4): (4, 32, 8), (16, 1): (8, 32, 8), (16, 2): (8, 32, 8), (16, 4): (8, 32, 8)},
    (3, 2): {(32, 1): (4, 16, 4), (32, 2): (4, 16, 4), (16, 1): (4, 32, 8), (16, 2): (4, 32, 8), (16, 4): (4, 32, 8)},
    (1, 1): {(32, 1): (8, 32, 8), (32, 2): (8, 32, 8), (32, 4): (8, 32, 8)},
}


def graph_convs():
    """The conv ops of the layer-by-layer graph, named like the state dict's convs, in launch order (csrc/wasb_graph.h with fuse == false): stem, Bottleneck with its
    two-source 1x1 conv, transition1, and per stage the branches' BasicBlocks, then per fused output the 1x1 convs of the lower
    branches and the stride-2 chains of the higher ones.  Stage 4 produces output 0 only.  The input is padded to 16 channels."""
    out = []

    def add(name, c0, cout, k, stride, div, c1=0):
        out.append(Conv(name, c0, c1, cout, k, stride, div))

    def stage(p, nb, n_out):
        for b in range(nb):
            for blk in range(R.BLOCKS_PER_BRANCH):
                for c in (1, 2):
                    add('%s.branches.%d.%d.conv%d' % (p, b, blk, c), CH[b], CH[b], 3, 1, 2 ** b)
        for i in range(n_out):
            for j in range(i + 1, nb):
                add('%s.fuse_layers.%d.%d.0' % (p, i, j), CH[j], CH[i], 1, 1, 2 ** j)
            for j in range(i):
                for k in range(i - j):
                    add('%s.fuse_layers.%d.%d.%d.0' % (p, i, j, k), CH[j], CH[i] if k == i - j - 1 else CH[j], 3, 2, 2 ** (j + k))

    add('conv1', 16, 64, 3, 1, 1)
    add('conv2', 64, 64, 3, 1, 1)
    add('layer1.0.conv1', 64, 32, 1, 1, 1)
    add('layer1.0.conv2', 32, 32, 3, 1, 1)
    add('layer1.0.conv3', 32, 128, 1, 1, 1, c1=64)          # + layer1.0.downsample.0, the second source
    add('transition1.0.0', 128, 16, 3, 1, 1)
    add('transition1.1.0.0', 128, 32, 3, 2, 1)
    stage('stage2.0', 2, 2)
    add('transition2.2.0.0', 32, 64, 3, 2, 2)
    stage('stage3.0', 3, 3)
    add('transition3.3.0.0', 64, 128, 3, 2, 4)
    stage('stage4.0', 4, 1)
    return out


def instance(conv):
    """(CK, MT, k, stride) of the conv_x3_kernel instance that runs `conv`: pack_conv_x3 and conv_x3_block_mt."""
    ck = 32 if conv.c0 % 32 == 0 else 16
    assert ck == 32 or (conv.c1 == 0 and conv.k == 3), conv
    mt = conv.cout // 16
    mt = min(mt, 2) if (conv.k, conv.stride, ck) == (3, 2, 32) else min(mt, 4)
    return ck, mt, conv.k, conv.stride


def launch(conv, h, w, batch):
    """launch_x3 for `conv` on a batch of (h, w) network inputs."""
    ck, mt, k, s = inst = instance(conv)
    th, tw, waves = TILES[(k, s)][(ck, mt)]
    ih, iw = (th - 1) * s + k, (tw - 1) * s + k
    ksteps = k * k if ck == 32 else (k * k + 1) // 2
    lds = (3 * ((ih * iw * ck + 7) & ~7) + 3 * ksteps * mt * 64 * 8) * 2
    assert lds <= 160 * 1024
    hin, win = -(-h // conv.div), -(-w // conv.div)
    oh, ow = -(-hin // s), -(-win // s)
    tiles_y, tiles_x = -(-oh // th), -(-ow // tw)
    tiles = tiles_y * tiles_x * batch
    blocks = conv.cout // (mt * 16)
    per_cu = max(1, min(160 * 1024 // lds, 2 if waves == 8 else 4))
    grid_x = min(tiles, max(1, 256 * per_cu // blocks))
    return Launch(conv, inst, (th, tw), waves, oh, ow, tiles_y, tiles_x, tiles, grid_x, blocks, -(-tiles // grid_x))


def coverage(cases=None):
    """What the case list reaches, from the arithmetic above: per instance the case ids with a launch of >= 2 trips, of a partial
    last tile row / column behind a whole one, of a plane smaller than one tile, and of interior tiles (neither first nor last in
    either axis).  -> {instance: {'trips': [...], 'ragged_y': [...], 'ragged_x': [...], 'small': [...], 'interior': [...]}}"""
    cov = {}
    for case in (CASES if cases is None else cases):
        for conv in graph_convs():
            l = launch(conv, case.h, case.w, case.batch)
            c = cov.setdefault(l.instance, collections.defaultdict(list))
            th, tw = l.tile
            for key, hit in (('trips', l.trips >= 2), ('ragged_y', l.tiles_y >= 2 and l.oh % th != 0), ('ragged_x', l.tiles_x >= 2 and l.ow % tw != 0),
                             ('small', l.oh < th and l.ow < tw), ('interior', l.tiles_y >= 3 and l.tiles_x >= 3)):
                if hit and case.id not in c[key]:
                    c[key].append(case.id)
    return cov


# ------------------------------------------------------------------------------------------ the comparison
def compare_segment(case, seg, x, taps_in, device_out=None, kernels='x3'):
    """Teacher-forced check of one segment, as E.compare_segment: the oracle (float64, fp32 storage) from the inputs `taps_in`, the
    spread oracle(fp32, reversed K) - oracle, and -- where `device_out` is given -- the device's outputs against the oracle (only
    the taps it holds: bneck_a1 is no tap of the device).
    -> [(tap, spread Stats, device Stats or None, bounds Stats, the oracle's tensor)]"""
    w = oracle_weights(case)
    ins = E.segment_inputs(seg, taps_in, x)
    ref = R.run_segment(seg, ins, w, 'layerwise', 'f64')
    alt = R.run_segment(seg, ins, w, 'layerwise', 'f32r')
    rows = []
    for tap in ref:
        if device_out is not None and tap not in device_out:
            continue
        sp = E.stats(alt[tap], ref[tap])
        dev = E.stats(device_out[tap], ref[tap]) if device_out is not None else None
        rows.append((tap, sp, dev, bounds(sp, kernels, case.planted), ref[tap]))
    return rows


def format_row(case, seg, tap, sp, dev, bd):
    d = 'device %.2e %.2e ratio %5.2f %5.2f' % (dev.max, dev.mean, dev.max / max(sp.max, 1e-300), dev.mean / max(sp.mean, 1e-300)) if dev else 'device -'
    return '%-18s %s %-9s %s | spread %.2e %.2e | bound %.2e %.2e' % (case.id, seg, tap, d, sp.max, sp.mean, bd.max, bd.mean)


def check_taps(case, taps, heat, idx=None, kernels='x3'):
    """Every stored tap and the heatmap of a device run (host tensors over the whole batch) against the oracle, segment by segment
    from the device's own input taps (S0: from E.inputs, the oracle's pre-processing for the frame cases), on the case's checked
    images.  Prints one row per tap.  -> (failures, the set of taps compared)"""
    dev = dict(taps, heat=heat)
    x = torch.from_numpy(E.inputs(case))
    im = list(case.images)
    failures, compared = [], set()
    for seg in SEGMENTS:
        picked = {k: v[im] for k, v in dev.items()}
        for tap, sp, d, bd, ref in compare_segment(case, seg, x[im], picked, picked, kernels):
            print(format_row(case, seg, tap, sp, d, bd))
            compared.add(tap)
            if not sp.max < CAP_SPREAD:
                failures.append((seg, tap, 'spread', sp.max))
            if not d.max <= bd.max:
                failures.append((seg, tap, 'max', d.max, bd.max))
            if not d.mean <= bd.mean:
                failures.append((seg, tap, 'mean', d.mean, bd.mean))
            if tap == 'heat' and case.planted and idx is not None:
                k = ref.shape[1]
                want = ref.reshape(len(im) * k, -1).argmax(1)
                got = idx.reshape(case.batch, k)[im].reshape(-1)
                if not torch.equal(got, want):
                    failures.append((seg, tap, 'argmax', got.tolist(), want.tolist()))
    return failures, compared


def device_run(case, batch=None, first=0):
    """One pass of an fp32 handle sized for `batch` samples (default: the case's batch) starting at sample `first`, and a second pass
    of the same handle on the same input.  -> (taps {name: (batch, C, h, w) float32 on the host}, heat, argmax), the same of pass 2"""
    from upliftingtabletennis_amd import wasb
    batch = case.batch if batch is None else batch
    sd = E.state_dict(case)
    if case.kind == 'table':
        net = wasb.get_table_model('hrnet', resolution=(case.w, case.h), state_dict=sd, max_batch=batch, dtype='f32')
    else:
        net = wasb.WASBNet(sd, resolution=(case.w, case.h), max_batch=batch, dtype='f32')
    runs = []
    for _ in range(2):
        if case.kind in ('frames', 'table'):
            nf = E.head_shape(case)[0] // 3
            f = torch.from_numpy(E.frames(case)[first:first + batch + nf - 1]).cuda()
            heat, idx, _w = wasb.WASBNet.forward_frames(net, f, want_heatmap=True)
        else:
            x = torch.from_numpy(E.inputs(case)[first:first + batch])
            heat, idx, _w = wasb.WASBNet.forward(net, x, want_heatmap=True, want_peaks=True)
        runs.append(({name: net.read_tap(name, batch).cpu() for name in TAPS}, heat.cpu(), idx.cpu()))
    return runs


def child_main(case_id, out):
    """The body of a cross-check child process: run the case under the kernel switch of the environment, save taps and heatmap."""
    case = {c.id: c for _, c in CROSS_CASES}[case_id]
    taps, heat, idx = device_run(case)[0]
    np.savez(out, heat=heat.numpy(), idx=idx.numpy(), **{k: v.numpy() for k, v in taps.items()})
