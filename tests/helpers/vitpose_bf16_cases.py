"""The sweep of the bf16 ViTPose path (tests/test_vitpose_bf16_host.py, tests/test_vitpose_bf16_gpu.py): the cases of
tests/helpers/vitpose_edge_cases.py unchanged, the tile sizes of the bf16 kernels they have to straddle, the oracle's taps of every
case in fp64 and fp32 arithmetic, and the measures and floors the GPU tests compare with.

Tile sizes of the new kernels over the token axis (csrc/gemm_bf16.h, csrc/vitpose_kernels.h):
  gemm_bf16_kernel        TM = 128 rows of M = batch * tokens per workgroup, 64 per wave, 16 per MFMA tile (TN = 128 and TK = 32 cut
                          N and K, which no case varies: every N is a multiple of 128, every K of 32)
  attention_bf16_kernel   64 queries per workgroup (16 per wave), key tiles of 64, MFMA k-steps of 32 keys, score tiles of 16 keys
  conv1x1_kernel<bf16>    64 pixels per workgroup (a token is 16 pixels)
The 17 edge cases hold 1, 3, 15, 63, 64, 65, 127, 128 and 129 tokens with M = 3, 6, 30, 126, 128, 195, 127, 256 and 258: T - 1, T and
T + 1 for the tiles of 64 and 128, but of the 16-wide MFMA / score tile only 15 and of the 32-key k-step nothing.  `EXTRA` adds 16, 17,
31, 32 and 33 tokens as one-row strips at batch 1, so that M in the GEMM is the token count too: a score tile exactly full and with
one key in the next (the per-16 masking), a P V k-step whose second score tile (keys 16 .. 31 of the step) is empty, holds one key,
lacks one key, is full, and a second k-step of one key.  `straddled` demands T - 1, T and T + 1 of every entry of TILES."""
import functools

import torch

from helpers import vitpose_bf16_torch as oracle
from helpers import vitpose_edge_cases as edges

TILES = {'gemm M': 128, 'gemm wave M': 64, 'mfma': 16, 'attention queries': 64, 'attention keys': 64, 'attention k-step': 32, 'conv1x1 pixels': 64}
# (h, w, in_ch, out_ch, batch, gain) like edges.CASES
EXTRA = [
    (16, 256, 9, 1, 1, 1),         # 16 tokens: one MFMA tile exactly, in the GEMM (M = 16) and in the scores
    (16, 272, 3, 13, 1, 1),        # 17: one row / one key in the second 16-tile
    (16, 496, 9, 1, 1, 1),         # 31: the k-step's second score tile lacks one key
    (16, 512, 3, 5, 1, 1),         # 32: one k-step of P V exactly; M = 32
    (16, 528, 9, 1, 1, 1),         # 33: a second k-step holding one key
]
CASES = list(edges.CASES) + EXTRA
PEAKED = [c for c in CASES if c[5] != 1]
assert len(PEAKED) == 4


def straddled(tile):
    """Whether the sweep holds T - 1, T and T + 1 tokens for the tile size T."""
    counts = {edges.tokens(c) for c in CASES}
    return {tile - 1, tile, tile + 1} <= counts


# Floors of the teacher-forced comparison (test_vitpose_bf16_gpu.py): the device may reach 3 x the largest difference and 2 x the
# share of differing elements that the oracle's own fp32- and fp64-arithmetic evaluations of the same step show, but never less than:
ULP_FLOOR = 1.0         # bf16 taps, in bf16 ulps of the oracle value: one rounding flip is one ulp, and a step whose fp32 and fp64
#                         evaluations happen to agree everywhere (small taps: 3 tokens) must still allow the device a flip
SHARE_FLOOR = 2.0 ** -8  # bf16 taps, share of elements that differ: a value flips when it lies within the fp32 evaluation error of
#                         a rounding tie.  bf16 ties are 2^16 fp32 ulps apart; an fp32 sum of K <= 1536 products (plus LN or
#                         erf in front) is off by up to ~sqrt(K) / 2 ulps of its largest partial sum, several times the result:
#                         ~2^7 ulps of the result, so 2 * 2^7 / 2^16 = 2^-8 of the values sit that close to a tie.  Below this share a
#                         tap of a few hundred elements cannot resolve a factor of two either
COUNT_FLOOR = 3         # ... and never fewer than three elements: the smallest taps hold 3 x 384 values
F32_FLOOR = 2.0 ** -21  # fp32 taps, |delta| over the tap's largest magnitude: 8 fp32 ulps of that magnitude -- two evaluation
#                         orders of one fp32 sum differ by a few ulps of the largest term wherever the oracle's two evaluations agree


SMALL = 2.0 ** -12      # bf16 taps: a value below SMALL of the tap's largest magnitude is measured in ulps of THAT magnitude, i.e. held to an
#                         absolute 2^-19 of the largest magnitude instead of a relative cap.  A sum's fp32 error scales with its
#                         terms, not with its result: where the terms cancel (a pre-activation next to a ReLU's zero, a qkv entry
#                         near 0) no relative cap can hold, and 0 against 1e-9 is no finding.  An fp32 sum of K <= 2304 products
#                         is off by up to ~sqrt(K) / 2 = 24 ulps of its largest partial sum: 2^-19.4 of it, taken as 2^-19 of the
#                         tap's largest magnitude; one bf16 ulp is that large at 2^7 * 2^-19 = 2^-12 of the magnitude.
#                         (Measured on the MI355X: the sweep also holds at 2^-14 and first exceeds one ulp, by a half, at 2^-16.)


def measures(got, want, bf16):
    """(max |delta| in bf16 ulps of `want`, share of elements that differ) for a bf16 tap; (max |delta| / max |want|, None) for an
    fp32 tap.  `want` is the oracle's fp64-arithmetic tap (holding bf16 values where the tap is stored as bf16)."""
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    d = (got - want).abs()
    scale = want.abs().max().clamp_min(1e-30)
    if not bf16:
        return float(d.max() / scale), None
    # ulp of a bf16 value v: 2^(floor(log2 |v|) - 7)
    ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp_min(SMALL * scale))) - 7)
    return float((d / ulp).max()), float((d > 0).double().mean())


def allowance(got32, want, bf16, gemm_fed=False):
    """What the device may show against `want` (fp64 arithmetic), from what the oracle's fp32-arithmetic evaluation `got32` of the same
    step shows: 3 x its largest difference and 2 x its share, not below the floors -- and for a GEMM-fed bf16 tap never more than
    one bf16 ulp."""
    big, share = measures(got32, want, bf16)
    if not bf16:
        return max(3 * big, F32_FLOOR), None
    n = torch.as_tensor(want).numel()
    ulps = max(3 * big, ULP_FLOOR)
    return (min(ulps, 1.0) if gemm_fed else ulps), max(2 * share, SHARE_FLOOR, COUNT_FLOOR / n)


class Taps:
    """The oracle's taps of a case, per stage, in fp64 arithmetic (the reference of the GPU tests) and what follows from them."""

    def __init__(self, case):
        sd, x = edges.state_dict(case), edges.inputs(case)
        self.o64 = oracle.Oracle(sd, torch.float64)
        self.o32 = oracle.Oracle(sd, torch.float32)
        self.stages = self.o64.forward(x)
        self.heat = self.stages[-1]['heat'].numpy()
        self.heat.setflags(write=False)

    def stage_input(self, stage):
        """What stage 1..13 takes: the fp64-arithmetic residual stream, as the fp32 values the device is given."""
        return self.stages[stage - 1]['x'].float()


@functools.lru_cache(maxsize=None)
def taps(case):
    return Taps(case)


def heat_error(case):
    """The oracle's own heatmap error against the fp64 restatement, as a share of each map's range (edges.Reference.error)."""
    return edges.reference(case).error(taps(case).heat)


# ---- the bars of the end-to-end comparison (test_vitpose_bf16_gpu.py (b), test_vitpose_bf16_hub_gpu.py): computed, not typed in
POSITION_FLOOR = 0.01          # heatmap px


@functools.lru_cache(maxsize=None)
def heat_bar():
    """Twice the largest heatmap error the ORACLE shows against fp64 over the sweep (of each map's range)."""
    return 2 * max(heat_error(c) for c in CASES)


def positions(heat):
    """(n, h, w) maps -> (n, 3) [x, y, visibility] in heatmap px: the project's own peak refine on the GPU (table variant, as the
    hub runs it)."""
    import numpy as np
    from upliftingtabletennis_amd import _lib, refine
    heat = torch.as_tensor(np.ascontiguousarray(heat, dtype=np.float32)).cuda()
    xyv = refine.refine_device(heat, heat.shape[2], heat.shape[1], _lib.REFINE_TABLE)[0]
    torch.cuda.synchronize()
    return xyv.cpu().numpy()


@functools.lru_cache(maxsize=None)
def position_bar():
    """Twice the oracle's worst shift of a refined position against fp64's over the sweep, at least POSITION_FLOOR (needs a GPU)."""
    import numpy as np
    worst = 0.0
    for c in CASES:
        ref = edges.reference(c)
        n = ref.argmax.size
        hh, ww = c[0] // 4, c[1] // 4
        a, b = positions(taps(c).heat.reshape(n, hh, ww)), positions(ref.heat64.reshape(n, hh, ww))
        worst = max(worst, float(np.abs(a[:, :2] - b[:, :2]).max()))
    print('\noracle: worst refined-position shift against fp64 %.3g heatmap px' % worst)
    return max(2 * worst, POSITION_FLOOR)
