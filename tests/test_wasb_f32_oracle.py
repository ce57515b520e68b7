"""The fp32 CNN's yardstick on the CPU (tests/helpers/wasb_f32_cases.py, oracle/wasb_bf16_ref.py with Weights(rounding='f32')):
the fp32-storage oracle is the fp32 oracle's graph on the weights the device stores; its fp32 spread is small, stable from one
summation order to the next and accepted by the device bounds; the bounds reject a segment whose inputs lost their corner pixel or
their third bf16 part; and the case list, by the restated launch arithmetic of csrc/conv_x3.hip, reaches a second persistent trip
of every conv_x3_kernel instance the graph uses, ragged last tiles, planes smaller than a tile and interior tiles."""
import numpy as np
import pytest
import torch

from helpers import wasb_edge_cases as E
from helpers import wasb_f32_cases as F
from oracle import wasb_bf16_ref as R
from oracle import wasb_ref
from upliftingtabletennis_amd import arch, weights


def _device_stored_state_dict(sd, in_ch, head_out):
    """`sd` as the fp32 net stores it (csrc/wasb_blob.h, csrc/conv.hip pack_conv), in reference format: BatchNorm folded in double and
    rounded to float32 once, written as the conv's weight with an identity BatchNorm that carries the folded bias; the two biases of
    the Bottleneck's two-source conv added in float and carried by bn3."""
    out = {}
    for s in arch.hrnet_convs(in_ch, head_out):
        w = np.asarray(sd[s.conv + '.weight'], np.float64)
        b = np.asarray(sd[s.conv + '.bias'], np.float64) if s.has_bias else np.zeros(s.cout)
        if s.bn:
            g, beta, mu, var = [np.asarray(sd['%s.%s' % (s.bn, f)], np.float64) for f in ('weight', 'bias', 'running_mean', 'running_var')]
            scale = g / np.sqrt(var + wasb_ref.BN_EPS)
            w, b = w * scale[:, None, None, None], (b - mu) * scale + beta
        out[s.conv + '.weight'] = w.astype(np.float32)
        if s.bn:
            out[s.bn + '.weight'], out[s.bn + '.bias'] = np.ones(s.cout), b.astype(np.float32)
            out[s.bn + '.running_mean'], out[s.bn + '.running_var'] = np.zeros(s.cout), np.ones(s.cout) - wasb_ref.BN_EPS
        else:
            out[s.conv + '.bias'] = b.astype(np.float32)
    b3, bd = out['model.layer1.0.bn3.bias'], out['model.layer1.0.downsample.1.bias']
    out['model.layer1.0.bn3.bias'], out['model.layer1.0.downsample.1.bias'] = b3 + bd, np.zeros_like(bd)          # float32 + float32
    return {k: torch.as_tensor(v).double() for k, v in out.items()}


@pytest.mark.parametrize('hw', [(40, 56), (8, 8)])
@pytest.mark.parametrize('in_ch,head_out', [(9, 3), (3, 13)])
def test_fp32_storage_is_the_fp32_oracles_graph_on_the_stored_weights(hw, in_ch, head_out):
    """S0 .. S4 chained with Weights(rounding='f32') equal wasb_ref's taps and heatmap, evaluated in float64 on the state dict as
    the device stores it, to 1e-10 of each tap's scale; stage4_0 is among the taps."""
    sd = weights.random_wasb_state_dict(5, in_ch=in_ch, head_out=head_out)
    x = torch.from_numpy(np.random.default_rng(6).standard_normal((2, in_ch) + hw))
    stored = _device_stored_state_dict(sd, in_ch, head_out)
    with torch.no_grad():
        _, taps = wasb_ref.hrnet_features(x, stored, return_taps=True)
        heat = wasb_ref.hrnet_forward(x, stored)[0]
    heat = heat[:, 1:2] if head_out == 3 else heat
    got = R.run_all(x, R.Weights(sd, rounding='f32'), 'layerwise')
    assert set(F.TAPS) <= set(got) and set(F.TAPS) <= set(taps)
    for k in F.TAPS:
        assert got[k].shape == taps[k].shape
        assert (got[k] - taps[k]).abs().max().item() <= 1e-10 * taps[k].abs().max().item(), k
    assert got['heat'].shape == heat.shape
    assert (got['heat'] - heat).abs().max().item() <= 1e-10 * heat.abs().max().item()
    # and the storage matters: against the unrounded weights the same taps differ by float32 rounding, far above 1e-10
    plain = R.run_all(x, R.Weights(sd, rounding=False), 'layerwise')
    assert (got['heat'] - plain['heat']).abs().max().item() > 1e-9 * heat.abs().max().item()


def _chained(case, image):
    """The oracle's own taps of one image, chained S0 .. S4 and stored as float32 like the device's."""
    taps = {'input': torch.from_numpy(E.inputs(case))[[image]]}
    for seg in F.SEGMENTS:
        for k, v in R.run_segment(seg, taps, F.oracle_weights(case), 'layerwise').items():
            taps[k] = v.float()
    return taps


@pytest.mark.parametrize('case', F.CASES + [c for _, c in F.CROSS_CASES] + F.MUTANT_SHAPES, ids=lambda c: c.id)
def test_spread_is_small_and_a_second_fp32_order_passes_the_bounds(case):
    """Per tap, teacher-forced from the oracle's own float32 taps of the first checked image: the spread (fp32, reversed K, against
    float64) stays below 2e-6 of the tap's scale, and the oracle's other fp32 order (K as stored) lies inside the bounds the device
    is held to, for every kernel choice -- the yardstick accepts a legitimate fp32 evaluation."""
    taps = _chained(case, case.images[0])
    w, seen = F.oracle_weights(case), set()
    for seg in F.SEGMENTS:
        other = R.run_segment(seg, taps, w, 'layerwise', 'f32')
        for tap, sp, _, _, ref in F.compare_segment(case, seg, taps['input'], taps):
            second = E.stats(other[tap], ref)
            print(F.format_row(case, seg, tap, sp, second, F.bounds(sp, 'x3', case.planted)))
            assert sp.max < F.CAP_SPREAD, (seg, tap, sp)
            seen.add(tap)
            if tap == 'bneck_a1':          # no tap of the device: the bounds are never applied to it
                continue
            for kernels in F.KERNELS:
                bd = F.bounds(sp, kernels, case.planted)
                assert second.max <= bd.max and second.mean <= bd.mean, (seg, tap, kernels, second, bd)
    assert seen == set(F.TAPS) | {'heat', 'bneck_a1'}


def _two_parts(v):
    """p0 + p1 of the three-way bf16 split of csrc/conv_x3.hip (x3_split8): the value without its third part."""
    v = v.float()
    p0 = v.to(torch.bfloat16).float()
    return p0 + (v - p0).to(torch.bfloat16).float()


def _corner_zeroed(v):
    v = v.clone()
    v[:, :, -1, -1] = 0
    return v


@pytest.mark.parametrize('case', F.MUTANT_SHAPES, ids=lambda c: c.id)
def test_the_bounds_reject_wrong_kernels(case):
    """Two mutants of every segment, run in float64 so that nothing but the mutation differs.
    (a) The bottom-right pixel of the segment's inputs zeroed -- a halo or mask error at the last tile -- exceeds the max bound of
    every output tap by 2 x, under every kernel choice's constants and with the planted case's wider mean constant as well.
    (b) The inputs without the third bf16 part of the split -- a lost low-order partial-product plane of conv_x3_kernel -- moves the
    mean of every output tap by 6 .. 22 x the spread's.  M_MEAN['x3'] (29, set by the planted case) no longer catches that; the
    noise-weight constant M_MEAN_NOISE['x3'] (4.82), which every case but the planted one has to meet, still does: the mutant
    exceeds that bound on every tap (by 1.3 x at least, not by the 2 x it had against the starting constant of 2)."""
    assert not case.planted
    taps = _chained(case, case.images[0])
    w = F.oracle_weights(case)
    for seg in F.SEGMENTS:
        ins = E.segment_inputs(seg, taps, taps['input'])
        corner = R.run_segment(seg, {k: _corner_zeroed(v) for k, v in ins.items()}, w, 'layerwise')
        parts = R.run_segment(seg, {k: _two_parts(v) for k, v in ins.items()}, w, 'layerwise')
        for tap, sp, _, bd, ref in F.compare_segment(case, seg, taps['input'], taps):
            c, p = E.stats(corner[tap], ref), E.stats(parts[tap], ref)
            print('%-14s %s %-9s corner max %.2e (%.1e x bound)  two-part mean %.2e (%.2f x bound, %.1f x spread)'
                  % (case.id, seg, tap, c.max, c.max / bd.max, p.mean, p.mean / bd.mean, p.mean / sp.mean))
            for kernels in F.KERNELS:
                for planted in (False, True):
                    assert c.max >= 2 * F.bounds(sp, kernels, planted).max, (seg, tap, kernels, c, sp)
            assert bd == F.bounds(sp, 'x3', False) and p.mean > bd.mean, (seg, tap, p, bd)
            assert p.mean >= 6 * sp.mean, (seg, tap, p, sp)


def test_the_restated_graph_is_the_architectures_conv_list():
    """graph_convs() holds every conv of the architecture that the graph computes (csrc/wasb_graph.h skips the fuse layers of
    stage 4's outputs 1 .. 3), with its shape."""
    spec = {s.conv[len('model.'):]: s for s in arch.hrnet_convs(9, 3)}
    convs = F.graph_convs()
    for c in convs:
        s = spec[c.name]
        assert (s.cout, s.k, s.stride) == (c.cout, c.k, c.stride) and s.cin == (9 if c.name == 'conv1' else c.c0), c
        assert c.c1 == (spec['layer1.0.downsample.0'].cin if c.name == 'layer1.0.conv3' else 0), c
    dead = {k for k in spec if k.startswith('stage4.0.fuse_layers.') and not k.startswith('stage4.0.fuse_layers.0.')}
    assert {c.name for c in convs} == set(spec) - dead - {'layer1.0.downsample.0', 'final_layers.0'} and len(convs) == len({c.name for c in convs})


def test_the_case_list_reaches_every_instance_at_its_edges():
    """From the restated launch arithmetic: every (chunk width, couts per block, k, stride) instance of conv_x3_kernel that the
    fp32 graph uses runs, in some case, a launch of >= 2 persistent trips, a partial last tile column behind a whole one and tiles
    that are neither first nor last in either axis; a partial last tile ROW and a plane smaller than one tile wherever the instance
    can have one at all (heights are multiples of 8, so a plane at 1/d of the input comes in units of 8 / d rows).  In the
    trip case the first image holds first-trip tiles and the last image later-trip tiles of every such launch; both are checked."""
    cov = F.coverage()
    used = {F.instance(c) for c in F.graph_convs()}
    assert set(cov) == used
    assert used == {(16, 1, 3, 1), (16, 4, 3, 1), (32, 1, 3, 1), (32, 2, 3, 1), (32, 4, 3, 1),
                    (16, 1, 3, 2), (16, 2, 3, 2), (16, 4, 3, 2), (32, 2, 3, 2), (32, 1, 1, 1), (32, 2, 1, 1), (32, 4, 1, 1)}
    for inst in used:
        units = {8 // (c.div * c.stride) for c in F.graph_convs() if F.instance(c) == inst}          # rows of output per 8 rows of input
        th = F.TILES[inst[2:]][inst[:2]][0]
        for key in ('trips', 'ragged_x', 'interior'):
            assert cov[inst][key], (inst, key)
        if any(u % th for u in units):
            assert cov[inst]['ragged_y'], inst
        if any(u < th for u in units):
            assert cov[inst]['small'], inst
    assert any(cov[i]['ragged_y'] for i in used) and any(cov[i]['small'] for i in used)
    trip = F.BY_ID['1032x8_b8']
    assert trip.batch <= 8 and trip.images == (0, trip.batch - 1)
    single = []
    for c in F.graph_convs():
        l = F.launch(c, trip.h, trip.w, trip.batch)
        if l.trips >= 2:
            assert 0 // l.grid_x == 0 and (l.tiles - 1) // l.grid_x >= 1          # trips of the first tile of image 0 and of the last tile of the last image
        else:
            single.append(c.name)
    # the launches of that case that stay at one trip: 1x1 fuse convs at 1/4 and 1/8 resolution, whose instances take >= 2 trips at 1/2
    assert single == ['stage3.0.fuse_layers.0.2.0', 'stage3.0.fuse_layers.1.2.0', 'stage4.0.fuse_layers.0.2.0', 'stage4.0.fuse_layers.0.3.0']
    # and 1032 rows is the smallest height (at 8 columns, 8 images) for which every instance takes a second trip
    smaller = F.coverage([F._case('smaller', trip.h - 8, trip.w, trip.batch)])
    assert not all(smaller[i]['trips'] for i in used)
