"""The cases of the uplift inference forward's edge sweep, shared by tools/make_goldens_uplift_family.py --edges (which writes
tests/golden/uplift_family_edges.npz), tests/test_uplift_forward_edges_host.py and tests/test_uplift_forward_edges_gpu.py.

Which kernel serves a stage is restated here from csrc/uplift.hip (run_stage, run_layer, run_attention) and NOT read from the library:
the GPU test compares the library's own launch counter with `stage_launches`, and the host test asserts that the sweep reaches every
class of `REQUIRED`, so that an edge cannot drop out of the sweep unnoticed."""
import collections

import numpy as np

from upliftingtabletennis_amd import synth

STAGE_VS = 84          # floats per row of the stage kernel's transposed V: every sequence of a 64-row tile starts at a multiple of 4
# the longest sequence (cls + len tokens) the attention kernels serve: 512 on the matrix pipe (dim 128, 4 heads of 32), else the scalar
# kernel's 64 KB of LDS, (2 S hd + 16 + S) * 4 <= 65536, for head dims 8 / 16 / 24
MAX_SEQ = {'small': 962, 'base': 496, 'large': 512, 'huge': 334}
HEAD_DIM = {'small': 8, 'base': 16, 'large': 32, 'huge': 24}

Case = collections.namedtuple('Case', 'size name mode rot kind b t pad seed')


def key(c):
    return '%s_%s_%s_%s_%s_B%d_T%d' % (c.size, c.name, c.mode, c.rot, c.kind, c.b, c.t + c.pad)


def make_inputs(c):
    """-> ball, table, mask, times (numpy float32).  'edge' / 'ragged' are synth's batches; 'single' is the one-step batch, whose mask
    rows must be [1], [0], [1] for the {0,1} check to see both values."""
    if c.kind == 'single':
        assert (c.b, c.t, c.pad) == (3, 1, 0)
        ball, table, mask, times = synth.edge_uplift_batch(3, 1, seed=c.seed, pad=0)
        mask[1, 0] = 0
        return ball, table, mask, times
    return {'edge': synth.edge_uplift_batch, 'ragged': synth.ragged_uplift_batch}[c.kind](c.b, c.t, seed=c.seed, pad=c.pad)


# ---------------------------------------------------------------- the rules, restated
def stage_accepts(s):
    """run_stage's condition for sequences of s tokens (D = 128, 4 heads, at most 16 layers): 64 // s sequences share a 64-row tile."""
    return s <= 64 and (64 // s) * ((s + 3) & ~3) <= STAGE_VS


def stage_sequences(c):
    """The token counts of the stages after the table stage: temporal and spin for the two-stage models, cls + tokens for singlestage."""
    length = c.t + c.pad
    return [length + 1] if c.name == 'singlestage' else [length, length + 1]


def stage_launches(c):
    """stage_x3_kernel launches per forward of a `large` model whose batch is one chunk."""
    assert c.size == 'large'
    return (1 if c.mode == 'dynamic' else 0) + sum(stage_accepts(s) for s in stage_sequences(c))


def attention_form(c, s, no_stage=False):
    """The kernel that computes attention for a stage of s-token sequences (no_stage: under TTUP_UPLIFT_NO_STAGE=1)."""
    if c.size != 'large':
        return 'scalar%d' % (16 if s <= 16 else 32 if s <= 32 else 64 if s <= 64 else 128)
    if stage_accepts(s) and not no_stage:
        return 'stage'
    if s <= 16:
        return 'attn_block'
    return 'mfma8_1' if s <= 64 else 'mfma8_2' if s <= 128 else 'mfma'


QKV_BLOCK_TOKENS = 64 * 256          # run_layer: qkv_block8_x3_kernel up to here, linear_x3_kernel above


def classes(c, no_stage=False):
    """The labels of `REQUIRED` (or, with no_stage, `REQUIRED_NO_STAGE`) this case reaches."""
    length, out = c.t + c.pad, set()
    _, _, mask, _ = make_inputs(c)
    later_valid = np.flip(np.maximum.accumulate(np.flip(mask, 1), 1), 1) > 0
    hole = (mask == 0) & later_valid          # a masked step with a valid one after it
    for s in stage_sequences(c):
        form = attention_form(c, s, no_stage)
        out.add('%s/%s' % (c.size, form))
        if form == 'stage':
            out.add('stage/seqs%d' % (64 // s))
            if 64 // s * s < 64:
                out.add('stage/dead_rows')
        if form == 'attn_block':
            out.add('attn_block/S%d' % s)
        if form == 'mfma':
            out.add('mfma/tiles%d' % ((s + 15) // 16))
            if s % 16:
                out.add('mfma/partial_tile')
        if form == 'mfma8_2' and hole[:, 64:].any():
            out.add('mfma8/hole_past_64')
        if form in ('mfma8_1', 'mfma8_2', 'mfma'):
            if QKV_BLOCK_TOKENS - 64 < c.b * s <= QKV_BLOCK_TOKENS:
                out.add('qkv/last_block8_launch')
            if QKV_BLOCK_TOKENS < c.b * s <= QKV_BLOCK_TOKENS + 192:
                out.add('qkv/first_linear_launch')
        if s == MAX_SEQ[c.size]:
            out.add('%s/limit' % c.size)
    if hole.any():
        out.add('%s/hole' % c.size)
    if c.rot == 'old':
        out.add('%s/old' % c.size)
    if (c.name, c.mode) != ('connectstage', 'dynamic'):
        out.add('variant/%s/%s' % (c.name, c.mode))
    return out


REQUIRED = {
    # whether the stage kernel is used (S = 1, 2, 5 are declined), and how many sequences share its tile (64 // S changes at 16 -> 17, 21 -> 22, 32 -> 33)
    'stage/seqs21', 'stage/seqs16', 'stage/seqs10', 'stage/seqs8', 'stage/seqs7', 'stage/seqs4', 'stage/seqs3', 'stage/seqs2', 'stage/seqs1', 'stage/dead_rows',
    'attn_block/S1', 'attn_block/S2', 'attn_block/S5',
    # the matrix-pipe attention: <= 128 tokens with a hole past token 64, 9 / 13 / 32 key tiles, a partial last tile, the longest launch
    'large/stage', 'large/attn_block', 'large/mfma8_2', 'large/mfma', 'large/hole', 'mfma8/hole_past_64',
    'mfma/tiles9', 'mfma/tiles13', 'mfma/tiles32', 'mfma/partial_tile', 'large/limit', 'large/old',
    'qkv/last_block8_launch', 'qkv/first_linear_launch',
    # the scalar kernel's four widths, three sizes, and its LDS limit
    'small/scalar16', 'small/scalar32', 'small/scalar64', 'small/scalar128', 'small/hole', 'base/scalar128', 'huge/scalar64', 'huge/scalar128', 'huge/limit', 'huge/old',
    # the fixture's variants
    'variant/singlestage/free', 'variant/singlestage/dynamic', 'variant/singlestage/stacked', 'variant/multistage/dynamic', 'variant/multistage/stacked',
    'variant/connectstage/originalmethod', 'variant/connectstage/stacked',
}
# with the stage kernel off: attn_block_x3_kernel at every S <= 16 of the sweep, attention_mfma8_kernel<1> (at most 4 key tiles)
REQUIRED_NO_STAGE = {'attn_block/S%d' % s for s in (1, 2, 3, 4, 5, 6, 8, 9, 16)} | {'large/mfma8_1'}


# ---------------------------------------------------------------- the sweep (connectstage / dynamic)
def _default(size, rot, kind, b, length, seed, pad=None):
    if kind == 'single':
        return Case(size, 'connectstage', 'dynamic', rot, kind, 3, 1, 0, seed)
    pad = (3 if length >= 8 else 1) if pad is None else pad
    return Case(size, 'connectstage', 'dynamic', rot, kind, b, length - pad, pad, seed)


SWEEP = (
    # short lengths: stage kernel accepted / declined (S = 1, 2, 5 are declined), sequences per tile
    [_default('large', 'new', 'single', 3, 1, 401)] +
    [_default('large', 'new', 'edge', b, n, 400 + n) for n, b in ((2, 22), (3, 5), (4, 13), (5, 13), (8, 9))] +
    [_default('large', 'new', 'edge', 4, n, 400 + n) for n in (16, 17, 21, 32, 33)] +
    # around the 64-token tile and the three matrix-pipe forms (len 100: holes at tokens >= 64)
    [_default('large', 'new', 'edge', 4, n, 400 + n) for n in (63, 64, 65, 100, 127, 128, 129)] +
    [_default('large', 'old', 'edge', 4, 200, 600), _default('large', 'new', 'ragged', 2, 511, 911)] +
    # the qkv block switch at 64 * 256 tokens: 16 256 / 16 383 tokens against 16 512 / 16 641
    [_default('large', 'new', 'ragged', b, 128, 700 + b) for b in (127, 129)] +
    # the other sizes: scalar attention
    [_default('small', 'new', 'edge', 5, n, 800 + n) for n in (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)] +
    [_default('base', 'new', 'edge', 4, 129, 1029), _default('huge', 'old', 'edge', 4, 64, 1064), _default('huge', 'new', 'ragged', 1, 333, 1333)]
)

# the cases of tests/golden/uplift_family_edges.npz: the reference's own model on every non-default variant edge, and four default
# cases that pin the torch restatement where the sweep goes furthest
FAMILY = [
    Case('large', 'singlestage', 'free', 'new', 'edge', 4, 60, 3, 501),                # S = 64: all 16 layers in one launch, at the upper edge
    Case('large', 'singlestage', 'free', 'new', 'edge', 4, 61, 3, 502),                # S = 65: per-layer kernels, strip_cls3_kernel
    Case('large', 'singlestage', 'dynamic', 'old', 'edge', 4, 3, 1, 503),              # S = 5 is declined; by-index RoPE table
    Case('large', 'multistage', 'dynamic', 'new', 'edge', 4, 14, 3, 504),              # 68 tokens: the last embed3 tile has 4
    Case('large', 'multistage', 'stacked', 'old', 'edge', 4, 30, 3, 505),              # stacked_embed: 32 + 1 tokens per trajectory
    Case('large', 'connectstage', 'originalmethod', 'new', 'edge', 4, 29, 3, 506),
    Case('large', 'connectstage', 'stacked', 'new', 'edge', 3, 126, 3, 507),           # the spin stage has S = 130
    Case('huge', 'singlestage', 'stacked', 'new', 'edge', 4, 62, 3, 508),
    Case('base', 'multistage', 'dynamic', 'old', 'edge', 4, 125, 3, 509),
    Case('small', 'singlestage', 'free', 'new', 'edge', 4, 126, 3, 510),
    _default('large', 'new', 'single', 3, 1, 511),
    _default('large', 'new', 'edge', 4, 5, 512),
    _default('large', 'old', 'edge', 4, 64, 513),
    _default('huge', 'new', 'edge', 3, 129, 514),
]
FAMILY_DEFAULT = [c for c in FAMILY if (c.name, c.mode) == ('connectstage', 'dynamic')]

# one case per attention form for the bit-for-bit test of masked slots
INERT = [c for c in SWEEP if (c.size, c.t + c.pad, c.b) in (('large', 17, 4), ('large', 5, 13), ('large', 100, 4), ('large', 200, 4), ('small', 33, 5))]
# the `large` lengths the per-layer kernels are run at with the stage kernel switched off
NO_STAGE = [c for c in SWEEP if c.size == 'large' and (c.t + c.pad <= 17 or c.t + c.pad == 21)]


def rel(x, ref):
    """max|x - ref| / max|ref|, in float64"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / np.abs(ref).max())
