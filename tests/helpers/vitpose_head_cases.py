"""The case table of the ViTPose head's training pass (tests/test_vitpose_head_ref_host.py, tests/test_vitpose_head_grad_gpu.py,
tools/make_goldens_vitpose_head.py): the smallest shapes at which the kernels of csrc/vitpose_head_grad.hip change form, with
seeded inputs.

Rows of the three GEMM levels are B hp wp, 4 B hp wp and 16 B hp wp (tile 64 x 64); every sliced reduction cuts at SLICE_TOKENS
tokens (csrc/vitpose_head_plan.h -- the host test reads the constant from the plan and holds this copy to it).
"""
import numpy as np

SLICE_TOKENS = 512
ZERO_CH = 5            # deconvolution 1's output channel with all-zero weights: variance 0, xhat 0
DEAD1, DEAD2 = 9, 17   # the channel of BN 1 / BN 2 whose beta is so negative that the ReLU kills it

# name: (batch, hp, wp, out_ch, seed, train)
CASES = {
    'g1x1_b1': (1, 1, 1, 1, 1, True),            # every border tap outside the map; BN over 4 and 16 values
    'g1x1_b2': (2, 1, 1, 1, 2, True),
    'g1x3': (2, 1, 3, 3, 3, True),
    'g3x1': (1, 3, 1, 2, 4, True),
    'g2x2': (3, 2, 2, 13, 5, True),
    'g5x7': (1, 5, 7, 16, 6, True),              # 35, 140, 560 rows: no tile multiple
    'g8x8': (1, 8, 8, 1, 7, True),               # exactly 64 rows
    'g5x13': (1, 5, 13, 4, 8, True),             # 65 rows
    'one_slice': (1, 16, 32, 1, 9, True),        # SLICE_TOKENS tokens: one whole slice
    'whole_slices': (2, 16, 32, 2, 10, True),    # 2 SLICE_TOKENS: whole slices only
    'last_of_one': (1, 19, 27, 1, 11, True),     # SLICE_TOKENS + 1: a last slice of one token (one row of the dW1 reduction)
    'g2x2_eval': (3, 2, 2, 13, 12, False),
    'g5x7_eval': (1, 5, 7, 16, 13, False),
}
GOLDEN_CASES = ('g2x2', 'g5x7', 'g2x2_eval')     # the ones tools/make_goldens_vitpose_head.py runs through the reference's own head


def tokens(name):
    b, hp, wp = CASES[name][:3]
    return b * hp * wp


def make_case(name):
    """-> (feat (B,384,hp,wp), params (vitpose_head_ref.PARAMS), dheat (B,C,4hp,4wp)) float64 holding float32 values, from the seed"""
    b, hp, wp, c, seed, _ = CASES[name]
    rng = np.random.default_rng(1000 + seed)
    f32 = lambda v: v.astype(np.float32).astype(np.float64)
    p = {}
    feat = f32(rng.standard_normal((b, 384, hp, wp)))
    for l, cin in (('1', 384), ('2', 256)):
        p['W' + l] = f32(rng.standard_normal((cin, 256, 4, 4)) * 0.03)
        p['g' + l] = f32(rng.uniform(0.5, 1.5, 256))
        p['b' + l] = f32(rng.standard_normal(256) * 0.3)
        p['rm' + l] = f32(rng.standard_normal(256) * 0.1)
        p['rv' + l] = f32(rng.uniform(0.5, 1.5, 256))
    p['W1'][:, ZERO_CH] = 0.0
    p['b1'][DEAD1] = -100.0
    p['b2'][DEAD2] = -100.0
    p['Wf'] = f32(rng.standard_normal((c, 256)) * 0.1)
    p['bf'] = f32(rng.standard_normal(c) * 0.1)
    dheat = f32(rng.standard_normal((b, c, 4 * hp, 4 * wp)))
    return feat, p, dheat
