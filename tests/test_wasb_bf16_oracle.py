"""The bf16-rounding segment oracle (oracle/wasb_bf16_ref.py) on the CPU: with rounding off it is the fp32 oracle's graph, with
rounding on it stays inside the bf16 path's end-to-end bars, its rounding helper is torch's bf16 conversion, and the spread of its
fp32 variant -- the yardstick of tests/test_wasb_taps_gpu.py -- stays below 2^-7 on the small cases of the edge sweep."""
import numpy as np
import pytest
import torch

from helpers import wasb_edge_cases as E
from oracle import wasb_bf16_ref as R
from oracle import wasb_ref
from upliftingtabletennis_amd import weights


@pytest.mark.parametrize('hw', [(40, 56), (8, 8)])
@pytest.mark.parametrize('in_ch,head_out', [(9, 3), (3, 13)])
def test_rounding_off_is_the_fp32_oracles_graph(hw, in_ch, head_out):
    """Rounding replaced by the identity: S0 .. S4 chained equal wasb_ref's taps and heatmap to 1e-10 of each tap's scale -- in
    float64 on both sides (wasb_ref evaluates in the dtype of its state dict).  `wasb_forward` itself casts its input to float32,
    so against it the same heatmap agrees to float32 precision."""
    sd = weights.random_wasb_state_dict(5, in_ch=in_ch, head_out=head_out)
    x = torch.from_numpy(np.random.default_rng(6).standard_normal((2, in_ch) + hw))
    sd64 = {k: torch.as_tensor(v).double() for k, v in sd.items()}
    with torch.no_grad():
        _, taps = wasb_ref.hrnet_features(x, sd64, return_taps=True)
        heat = wasb_ref.hrnet_forward(x, sd64)[0]
    heat = heat[:, 1:2] if head_out == 3 else heat
    for model in R.MODELS:
        got = R.run_all(x, R.Weights(sd, rounding=False), model)
        names = [k for k in got if k in taps]
        assert set(E.BASE_TAPS + ('layer1',)) <= set(names)
        for k in names:
            assert got[k].shape == taps[k].shape
            assert (got[k] - taps[k]).abs().max().item() <= 1e-10 * taps[k].abs().max().item(), (model, k)
        assert (got['heat'] - heat).abs().max().item() <= 1e-10 * heat.abs().max().item(), model
        if head_out == 3:
            f32 = wasb_ref.wasb_forward(x.float(), sd).double()
            assert (got['heat'] - f32).abs().max().item() <= 1e-4 * heat.abs().max().item(), model


@pytest.mark.parametrize('model', R.MODELS)
def test_rounding_on_stays_inside_the_end_to_end_bars(golden, model):
    """Chained end to end, the oracle is a bf16 net like the device's: 4 % max / 1 % rms of the fp32 heatmap's range."""
    g = golden('wasb_small.npz')
    seed, planted, b, h, w = [int(v) for v in g['noise_64x96/meta']]
    assert not planted
    sd = weights.random_wasb_state_dict(seed)
    x = np.random.default_rng(seed).standard_normal((b, 9, h, w)).astype(np.float32)
    ref = g['noise_64x96/heat']
    got = R.run_all(x, R.Weights(sd), model)['heat'].numpy()
    scale = ref.max() - ref.min()
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 4e-2 * scale
    assert np.sqrt(np.mean((got - ref) ** 2)) <= 1e-2 * scale


def test_bf16_round_is_torchs_conversion():
    """On float32 values -- a dense grid, ties to even on both sides of an even / odd mantissa, bf16 and float32 subnormals,
    overflow to infinity, signed zeros, infinities, NaN."""
    rng = np.random.default_rng(9)
    vals = [rng.standard_normal(4096).astype(np.float32), (rng.standard_normal(4096) * 1e-38).astype(np.float32),
            (rng.standard_normal(512) * 1e38).astype(np.float32)]
    bits = []
    for hi in (0x3f80, 0x3f81, 0x0001, 0x0000, 0x007f, 0x0080, 0x7f7f, 0x7f7e, 0x4049):          # bf16 patterns: the lower half-way, below and above it
        for lo in (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff):
            bits += [hi << 16 | lo, 0x80000000 | hi << 16 | lo]
    vals.append(np.array(bits, np.uint32).view(np.float32))
    vals.append(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 3.3895314e38, -3.3895314e38, 3.39e38, 1e-45, -1e-45], np.float32))
    x = torch.from_numpy(np.concatenate(vals))
    want = x.to(torch.bfloat16).double()
    got = R.bf16_round(x)
    assert got.dtype == torch.float64
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan], want[~nan])
    assert torch.equal(torch.signbit(got[~nan]), torch.signbit(want[~nan]))          # -0 stays -0
    # a float64 value is rounded once, not through float32: just above a bf16 half-way point, by less than a float32 step
    v = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40], dtype=torch.float64)
    assert R.bf16_round(v).item() == 1.0 + 2.0 ** -7


@pytest.mark.parametrize('case', [c for c in E.CASES if c.h * c.w <= 72 * 104], ids=lambda c: c.id)
def test_spread_of_the_small_cases_stays_below_the_cap(case):
    """The yardstick itself, on the oracle's own chained taps of the case's first checked image: oracle(fp32, reversed K) -
    oracle(float64) below 2^-7 of every tap's scale (the GPU test asserts the same on the device's taps, for every case)."""
    x = torch.from_numpy(E.inputs(case))[list(case.images[:1])]
    taps = {}
    for seg in E.SEGMENTS:
        for tap, sp, _, bd, ref in E.compare_segment(case, seg, x, taps):
            print(E.format_row(case, seg, tap, sp, None, bd))
            assert sp.max < E.CAP_SPREAD, (seg, tap, sp)
            taps[tap] = ref
    assert set(E.stored_taps(case)) <= set(taps) and 'heat' in taps
