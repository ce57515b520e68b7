"""CPU side of the ViTPose edge sweep (tests/helpers/vitpose_edge_cases.py): the torch restatement that the GPU tests use as their
fp64 reference is pinned at the edge shapes by the reference's own heatmaps (tests/golden/vitpose_edges.npz, made by
tools/make_goldens_vitpose.py --edges), and the premises the GPU tests rest on hold on the reference side alone."""
import numpy as np
import pytest

from helpers import vitpose_edge_cases as edges
from test_vitpose_gpu import HEAT_BAR

GOLDEN = edges.golden_cases()


def test_fixture_holds_the_golden_cases(golden):
    g = golden('vitpose_edges.npz')
    assert sorted({n.split('/')[0] for n in g.files}) == sorted('edge_' + edges.case_id(c) for c in GOLDEN)
    assert sorted(edges.tokens(c) for c in GOLDEN) == [1, 3, 3, 63, 65, 127]
    for c in GOLDEN:
        h, w, cin, cout, b, _ = c
        assert [int(v) for v in g['edge_%s/meta' % edges.case_id(c)]] == [edges.WEIGHT_SEED, edges.INPUT_SEED, b, cin, cout, h, w, 1]


@pytest.mark.parametrize('case', GOLDEN, ids=edges.case_id)
def test_restatement_matches_reference_at_the_edges(golden, case):
    """fp32 and fp64 restatement within 1e-5 of the range of the reference's heatmaps (the bar of test_vitpose_oracle.py), equal argmax."""
    g = golden('vitpose_edges.npz')
    name = 'edge_' + edges.case_id(case)
    h, w, _, cout, b, _ = case
    want = g[name + '/heat']
    ref = edges.reference(case)
    assert want.shape == (b, cout, h // 4, w // 4)
    for got in (ref.heat32, ref.heat64):
        err = np.abs(got - want).max() / (want.max() - want.min())
        print('\n%s %s: max |restatement - reference| = %.3g of the range' % (name, got.dtype, err))
        assert err <= 1e-5
        assert np.array_equal(got.reshape(b * cout, -1).argmax(1), g[name + '/argmax'])
    assert np.allclose(ref.range, g[name + '/range'], rtol=1e-5) and np.allclose(ref.margin, g[name + '/margin'], rtol=1e-4)


def test_token_counts_and_strips():
    assert {edges.tokens(c) for c in edges.CASES} == {1, 3, 15, 63, 64, 65, 127, 128, 129}
    assert {edges.tokens(c) for c in edges.CASES if c[5] != 1} == {63, 65, 128, 129}
    assert all(c[5] in (1, edges.PEAKED_GAIN) for c in edges.CASES) and len(set(edges.CASES)) == len(edges.CASES) == 17
    rows = [c for c in edges.CASES if c[0] == 16 and c[1] > 16]
    cols = [c for c in edges.CASES if c[1] == 16 and c[0] > 16]
    assert {edges.tokens(c) for c in rows} == {3, 127} and {edges.tokens(c) for c in cols} == {3, 129}
    assert {c[2] for c in edges.CASES} == {1, 3, 4, 6, 9} and {c[3] for c in edges.CASES} == {1, 4, 5, 13, 16}


@pytest.mark.parametrize('case', edges.CASES, ids=edges.case_id)
def test_reference_precision_and_margins(case):
    """The fp32 restatement is within HEAT_BAR of the fp64 one (so fp32 arithmetic can meet the bar at this shape), and at least
    90 % of the maps have a top-2 margin above twice the bar: the cap on what the GPU test's argmax comparison may leave out."""
    ref = edges.reference(case)
    decided = ref.decided(HEAT_BAR)
    print('\n%s: fp32 vs fp64 %.3g of the range; %d of %d maps decided, smallest margin %.3g of the range'
          % (edges.case_id(case), ref.e32, decided.sum(), decided.size, (ref.margin / ref.range).min()))
    assert ref.e32 <= HEAT_BAR
    assert decided.mean() >= 0.9


def test_peaked_cases_move_the_running_maximum():
    """Gain-4 cases, block 0: a query's largest score lies in a key tile after the first (key >= 64) for at least a quarter of
    the (sample, head, query) rows that have more than 64 keys -- counted over the cases together: with 65 keys the second tile
    holds one key, so that case alone contributes ~1/65 -- and the mean score spread (max - min over the keys) of every case is
    above 5, so `alpha = expf(m_run - m_new)` is far from 1 where the maximum moves.  The gain-1 twin's spread is printed beside it."""
    late = total = 0
    for case in [c for c in edges.CASES if c[5] != 1]:
        s = edges.block0_scores(case)
        spread = (s.max(-1) - s.min(-1)).mean()
        flat = edges.block0_scores(case[:5] + (1,))
        flat_spread = (flat.max(-1) - flat.min(-1)).mean()
        n = s.shape[-1]
        frac = float((s.argmax(-1) >= 64).mean()) if n > 64 else float('nan')
        print('\n%s: mean score spread %.2f (gain 1: %.2f), largest score at key >= 64 in %.3f of the rows' % (edges.case_id(case), spread, flat_spread, frac))
        assert spread > 5
        if n > 64:
            late += int((s.argmax(-1) >= 64).sum())
            total += s.argmax(-1).size
    assert total > 0 and late >= 0.25 * total
