"""The cases of the ViTPose backbone's training pass (tests/test_vitpose_backbone_grad_gpu.py, tools/make_goldens_vitpose_backbone.py):
seeded weights, images and feature gradients at the smallest shapes at which a kernel of csrc/vitpose_grad.hip changes form.

Token grids 1x1, 1x3, 7x9 (63), 8x8 (64), 5x13 (65), 8x16 (128), 3x43 (129): the edges of the attention kernels' 64-query / 64-key
tiles and of the GEMMs' 64-row tiles.  Batch x tokens of 512, 513 and 1024: one whole slice, a last slice of one token, two whole
slices of every fixed-order sum (SLICE_TOKENS).  Batch 1, 2, 3, 8; in_ch 1, 3, 9.  `sharp`: the q and k rows of every attn.qkv.weight
times 4 (DESIGN.md section 13's sharp-attention variant), so that exp(s - lse) is far from flat.

Branch scales (`mode`): None; 'ones' (explicit ones); 'mixed' (a draw of sample_drop_scale's rule); 'drop5' (every sample dropped in both
branches of block 5); 'one_of_three' (sample 1 of 3 dropped in the attention branch of block 7); 'golden' (what the reference's
DropPath modules drew when the goldens were made: tests/golden/vitpose_backbone_grad.npz, `<case>/scale`)."""
import numpy as np

SLICE_TOKENS = 512
DROPPED_BLOCK = 5
# name: (batch, hp, wp, in_ch, seed, mode, sharp)
CASES = {
    'g1x1': (1, 1, 1, 3, 101, None, False),
    'g1x3': (2, 1, 3, 1, 102, 'golden', False),
    'g7x9': (1, 7, 9, 3, 103, 'golden', False),
    'g8x8': (2, 8, 8, 9, 104, None, False),
    'g5x13': (2, 5, 13, 3, 105, 'golden', False),
    'g8x16': (1, 8, 16, 3, 106, 'drop5', False),
    'g3x43': (2, 3, 43, 3, 107, 'mixed', False),
    'g2x3_one': (3, 2, 3, 3, 108, 'one_of_three', False),
    'g5x13_sharp': (1, 5, 13, 3, 109, None, True),
    'g3x43_sharp': (1, 3, 43, 3, 110, 'ones', True),
    's512': (8, 8, 8, 3, 111, 'mixed', False),
    's513': (1, 27, 19, 3, 112, None, False),
    's1024': (8, 8, 16, 1, 113, 'mixed', False),
}
GOLDEN_CASES = tuple(n for n, c in CASES.items() if c[5] == 'golden')
RATE = 0.3


def tokens(name):
    b, hp, wp = CASES[name][:3]
    return b * hp * wp


def keep(rate=RATE):
    return [1.0 - rate * i / 11 for i in range(12)]


def scales(name, golden=None):
    """The case's (12, 2, B) float32 scales, or None.  golden: the loaded .npz, for the 'golden' cases."""
    b, _, _, _, seed, mode, _ = CASES[name]
    if mode is None:
        return None
    s = np.ones((12, 2, b), np.float32)
    if mode == 'golden':
        return np.asarray(golden[name + '/scale'], np.float32)
    if mode == 'mixed':
        rng = np.random.default_rng(seed + 1000)
        k = np.asarray(keep()).reshape(12, 1, 1)
        s = np.where(rng.random((12, 2, b)) < k, 1.0 / k, 0.0).astype(np.float32)
    elif mode == 'drop5':
        s[DROPPED_BLOCK] = 0
    elif mode == 'one_of_three':
        s[7, 0, 1] = 0
        s[7, 0, [0, 2]] = np.float32(1.0 / keep()[7])
    return s


def make_case(name):
    """-> (x (B, C, 16hp, 16wp) float32, state_dict (the backbone's keys and the rest of a ViTPose), dfeat (B * tokens, 384) float32)"""
    from upliftingtabletennis_amd import weights
    b, hp, wp, c, seed, _, sharp = CASES[name]
    sd = weights.random_vitpose_state_dict(seed, in_ch=c, out_ch=1, resolution=(16 * wp, 16 * hp), planted=False)
    if sharp:
        for i in range(12):
            sd['model.backbone.blocks.%d.attn.qkv.weight' % i][:768] *= 4
    rng = np.random.default_rng(seed + 500)
    x = rng.standard_normal((b, c, 16 * hp, 16 * wp)).astype(np.float32)
    dfeat = rng.standard_normal((b * hp * wp, 384)).astype(np.float32)
    return x, sd, dfeat
