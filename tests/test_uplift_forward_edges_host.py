"""The uplift forward's edge sweep, CPU side: the fixture tests/golden/uplift_family_edges.npz (the reference's own models,
tools/make_goldens_uplift_family.py --edges) holds exactly the cases of tests/helpers/uplift_forward_cases.py; the torch restatement
the GPU sweep is compared with (tests/helpers/uplift_torch_grad.py) reproduces the reference where the sweep goes furthest; and the
case table reaches every kernel-selection class it is there for."""
import numpy as np
import pytest

from helpers import uplift_forward_cases as C
from helpers import uplift_torch_grad as R
from upliftingtabletennis_amd import weights

# a tenth of the parity bar (1e-4, BASELINE.json north_star): what the restatement may be off cannot eat into the bar
RESTATEMENT_BAR = 1e-5


def test_fixture_holds_exactly_the_cases(golden):
    g = golden('uplift_family_edges.npz')
    assert sorted({k.split('/')[0] for k in g.files}) == sorted(C.key(c) for c in C.FAMILY)
    assert sorted({k.split('/')[1] for k in g.files}) == ['kind', 'meta', 'pos', 'rot', 'variant']
    for c in C.FAMILY:
        k = C.key(c)
        assert [int(v) for v in g[k + '/meta']] == [c.seed, c.b, c.t, c.pad], k
        assert [str(v) for v in g[k + '/variant']] == [c.size, c.name, c.mode, c.rot] and str(g[k + '/kind']) == c.kind, k
        assert g[k + '/rot'].shape == (c.b, 3) and g[k + '/pos'].shape == (c.b, c.t + c.pad, 3), k
        assert g[k + '/rot'].dtype == g[k + '/pos'].dtype == np.float32 and np.isfinite(g[k + '/rot']).all() and np.isfinite(g[k + '/pos']).all(), k
    assert len(C.FAMILY_DEFAULT) == 4 and {(c.size, c.rot, c.b, c.t + c.pad) for c in C.FAMILY_DEFAULT} == {
        ('large', 'new', 3, 1), ('large', 'new', 4, 5), ('large', 'old', 4, 64), ('huge', 'new', 3, 129)}


@pytest.mark.parametrize('case', C.FAMILY_DEFAULT, ids=C.key)
def test_restatement_matches_the_reference_at_the_sweep_ends(golden, case):
    """fp32 restatement against the reference's get_model(...).eval() on the regenerated inputs, max|a - ref| / max|ref| <= 1e-5 for
    rot and pos; the distance of the high-precision mode to the same fixture is printed beside it (the reference's own fp32 noise)."""
    g = golden('uplift_family_edges.npz')
    k = C.key(case)
    sd, inputs = weights.random_uplift_state_dict(case.seed, case.size, case.name, case.mode, case.rot), C.make_inputs(case)
    rot, pos = R.forward_np(sd, case.size, *inputs, time_rotation=case.rot)
    assert rot.dtype == pos.dtype == np.float32
    hrot, hpos = R.forward_np(sd, case.size, *inputs, time_rotation=case.rot, high_precision=True)
    assert hrot.dtype == hpos.dtype == np.float64
    e_rot, e_pos = C.rel(rot, g[k + '/rot']), C.rel(pos, g[k + '/pos'])
    print('\n%s: fp32 restatement vs reference rot %.3e pos %.3e; high-precision mode vs reference rot %.3e pos %.3e'
          % (k, e_rot, e_pos, C.rel(hrot, g[k + '/rot']), C.rel(hpos, g[k + '/pos'])))
    assert e_rot <= RESTATEMENT_BAR and e_pos <= RESTATEMENT_BAR


def test_high_precision_mode_keeps_the_rope_index_in_float32():
    """A time stamp such as 0.0250000003 s (float32 of 0.025) gives round(t / 0.002) = 12 in float32 and 13 in float64: the
    high-precision mode must turn by the float32 index, so on stamps on such ties it stays a rounding away from the fp32 path."""
    c = C.Case('small', 'connectstage', 'dynamic', 'new', 'edge', 3, 5, 1, 77)
    sd, (ball, table, mask, times) = weights.random_uplift_state_dict(c.seed, c.size), C.make_inputs(c)
    times[:, :5] = np.float32(0.025) * np.arange(5, dtype=np.float32)[None]
    t64 = times.astype(np.float64)
    assert (np.round(times / np.float32(1 / 500)) != np.round(t64 / (1 / 500))).any()          # the ties are there
    rot, pos = R.forward_np(sd, c.size, ball, table, mask, times)
    hrot, hpos = R.forward_np(sd, c.size, ball, table, mask, times, high_precision=True)
    assert C.rel(rot, hrot) <= RESTATEMENT_BAR and C.rel(pos, hpos) <= RESTATEMENT_BAR


def test_case_table_reaches_every_class():
    """Every kernel-selection class of the issue is reached by a case, by the helper's own restatement of the rules; the stage
    kernel's acceptance rule declines exactly S = 1, 2 and 5 among S <= 64."""
    assert [s for s in range(1, 65) if not C.stage_accepts(s)] == [1, 2, 5] and not C.stage_accepts(65)
    assert len({C.key(c) for c in C.SWEEP}) == len(C.SWEEP) and len({C.key(c) for c in C.FAMILY}) == len(C.FAMILY) == 14
    got = set()
    for c in C.SWEEP + C.FAMILY:
        assert c.b >= 3 or c.kind == 'ragged'
        got |= C.classes(c)
    assert C.REQUIRED <= got, sorted(C.REQUIRED - got)
    got = set()
    for c in C.NO_STAGE:
        got |= C.classes(c, no_stage=True)
    assert C.REQUIRED_NO_STAGE <= got, sorted(C.REQUIRED_NO_STAGE - got)
    assert sorted(c.t + c.pad for c in C.NO_STAGE) == [1, 2, 3, 4, 5, 8, 16, 17, 21]
    # stage launches per forward at the lengths where the choice changes
    want = {1: 1, 2: 2, 3: 3, 4: 2, 5: 2, 64: 2, 65: 1}
    assert {n: C.stage_launches(c) for c in C.SWEEP if c.size == 'large' and (n := c.t + c.pad) in want and c.b < 100} == want
    # the sweep's lengths and batches, as the issue lists them
    large = {(c.t + c.pad, c.b, c.kind, c.rot) for c in C.SWEEP if c.size == 'large'}
    assert large == ({(1, 3, 'single', 'new'), (2, 22, 'edge', 'new'), (3, 5, 'edge', 'new'), (4, 13, 'edge', 'new'), (5, 13, 'edge', 'new'), (8, 9, 'edge', 'new')}
                     | {(n, 4, 'edge', 'new') for n in (16, 17, 21, 32, 33, 63, 64, 65, 100, 127, 128, 129)}
                     | {(200, 4, 'edge', 'old'), (511, 2, 'ragged', 'new'), (128, 127, 'ragged', 'new'), (128, 129, 'ragged', 'new')})
    assert {(c.t + c.pad, c.b, c.kind) for c in C.SWEEP if c.size == 'small'} == {(n, 5, 'edge') for n in (15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)}
    assert {(c.size, c.t + c.pad, c.b, c.kind, c.rot) for c in C.SWEEP if c.size in ('base', 'huge')} == {
        ('base', 129, 4, 'edge', 'new'), ('huge', 64, 4, 'edge', 'old'), ('huge', 333, 1, 'ragged', 'new')}
    # the two limits are the sweep's longest cases; the masks of the one-step case
    assert 511 + 1 == C.MAX_SEQ['large'] and 333 + 1 == C.MAX_SEQ['huge']
    for size, hd in C.HEAD_DIM.items():
        if size != 'large':
            s = C.MAX_SEQ[size]
            assert (2 * s * hd + 16 + s) * 4 <= 65536 < (2 * (s + 1) * hd + 16 + s + 1) * 4
    assert C.make_inputs(C.SWEEP[0])[2].tolist() == [[1.0], [0.0], [1.0]]
    mask100 = C.make_inputs(next(c for c in C.SWEEP if c.size == 'large' and c.t + c.pad == 100))[2]
    assert mask100[0, 67] == 0 and mask100[0, 68] == 1          # a hole past token 64
    assert len(C.INERT) == 5
