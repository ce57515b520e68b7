"""The crafted tracks and seed lists of tests/helpers/trajgen_edge_cases.py under the CPU oracle (no GPU): every named case
takes the rule and the cut arm it was written for, named cases and random sweep reach every reachable (mode, rule, arm) triple,
the oracle's `count_hits` equals the REFERENCE's `_count_hits` on the named cases bit for bit (tests/golden/trajgen_edges.npz,
tools/make_goldens.py trajgen_edges), and the seed lists of the stop-rule tests keep their distance from every threshold."""
import collections

import numpy as np
import pytest

from oracle import trajgen_ref as T
from helpers import trajgen_edge_cases as C

TIMES = T.save_times()


def _label(track, mode, direction):
    why = []
    res = T.select(track, TIMES, mode, direction, why=why)
    assert len(why) == 2 and (res is not None) == (why[0] == 'accepted')
    return res, tuple(why)


def test_case_tracks_fit_the_sample_buffer():
    assert C.S == len(TIMES)
    for c in C.all_named_cases():
        assert C.track(c).shape == (c['script']['n'], 3) and c['script']['n'] <= C.S
    assert {len(C.track(c)) for c in C.all_named_cases()} >= {99, 100, 101, C.S}


def test_every_named_case_takes_its_rule_and_cut_arm():
    cases = C.all_named_cases()
    assert len({c['name'] for c in cases}) == len(cases)
    for c in cases:
        tr = C.track(c)
        res, why = _label(tr, c['mode'], c['direction'])
        assert why == (c['why'], c['branch']), (c['name'], why)
        if c['keep'] is not None:
            assert res is not None and res[0] == c['keep'], (c['name'], res)
        plain = T.select(tr, TIMES, c['mode'], c['direction'])          # `why` changes nothing
        assert (plain is None) == (res is None)
        assert res is None or (plain[0] == res[0] and np.array_equal(plain[1], res[1]))


def test_cut_at_exactly_0_2_leaves_99_frames_and_half_a_sample_later_100():
    for c in C.all_named_cases():
        if '/cut/' not in c['name']:
            continue
        tr = C.track(c)
        hits = [t for h in T.count_hits(tr, c['direction']) for t in h]
        if c['name'].endswith('/at_0.2') or c['name'].endswith('/at_0.2_wide'):
            assert 0.2 in hits and int(np.sum(TIMES[:len(tr)] < 0.2)) - 1 == 99, c['name']
        if c['name'].endswith('/half_below'):
            assert max(hits) < 0.2, c['name']
        if c['name'].endswith('/half_above'):
            assert c['keep'] == 100 and min(t for t in hits if t >= 0.2) == 0.75 * (201 / 2 / 500) + 0.25 * (101 / 500), c['name']


def test_named_cases_and_sweep_cover_every_reachable_triple():
    table = C.required_coverage()
    assert len(table) == len(T.MODES) * len(C.WHY) * len(C.CUT_BRANCHES) == 210
    required = [k for k, reason in table.items() if reason is None]
    assert len(required) == 73 and all(isinstance(r, str) and r for k, r in table.items() if k not in required)
    named, overall = collections.Counter(), collections.Counter()
    for c in C.all_named_cases():
        named[(c['mode'], c['why'], c['branch'])] += 1
    overall.update(named)
    accepted_cut = collections.Counter()
    for mode in T.MODES:
        for direction in T.DIRECTIONS:
            tracks = C.random_tracks(mode, direction)
            assert len(tracks) == 1000 and all(len(t) <= C.S for t in tracks)
            for tr in tracks:
                _, why = _label(tr, mode, direction)
                overall[(mode,) + why] += 1
                accepted_cut[(mode, direction)] += why[0] == 'accepted' and why[1] != 'none'
    missing = [(k, named[k], overall[k]) for k in required if named[k] < 1 or overall[k] < 5]
    assert not missing, missing
    assert not [k for k in overall if table[k] is not None]          # nothing the table calls unreachable was reached
    assert min(accepted_cut.values()) >= 20, accepted_cut


def test_no_hit_time_equals_a_time_label():
    """The helper's claim that `times[i] < t` never meets t equal to a label once a cut rule looks one up."""
    assert C.hit_time_equals_a_label() == []
    assert [k for k in range(len(TIMES)) if TIMES[k] == k / T.FPS] == list(range(9))


def test_oracle_count_hits_equals_the_reference_on_the_named_cases(golden):
    g = golden('trajgen_edges.npz')
    cases = C.all_named_cases()
    assert [str(s) for s in g['names']] == [c['name'] for c in cases]
    got = [T.count_hits(C.track(c), c['direction']) for c in cases]
    nonempty = 0
    for j, key in enumerate(('opponent', 'own', 'ground')):
        n, t = g['hits/%s/n' % key], g['hits/%s/t' % key]
        assert [len(h[j]) for h in got] == [int(v) for v in n], key
        assert np.array_equal(np.array([v for h in got for v in h[j]], dtype=np.float64), t), key
        nonempty += int((n > 0).sum())
    assert nonempty >= len(cases)


@pytest.mark.parametrize('direction', T.DIRECTIONS)
@pytest.mark.parametrize('mode', T.MODES)
def test_stop_seed_lists_keep_their_distance(golden, mode, direction):
    """65 seeds per combination; oracle margins at the deciding sample, the one before it and all earlier ones at least 1e-4 m and
    0.05 px (100 times the integrator's own 1e-6 m bar); every stop reason the mode's rule can give; lane 64 holds the most common one.
    The record the GPU test compares with is what the oracle gives."""
    seeds = C.stop_seeds(mode, direction)
    assert len(seeds) == len(set(seeds)) == C.N_STOP_SEEDS == 65
    pos, vel, rot, ns, why, margins = T.simulate(seeds, mode, direction, want_stop=True)
    assert margins.shape == (65, 3, 2)
    assert margins[:, :, 0].min() >= C.STOP_MARGIN_M and margins[:, :, 1].min() >= C.STOP_MARGIN_PX, (margins[:, :, 0].min(), margins[:, :, 1].min())
    census = collections.Counter(why)
    assert set(census) == set(C.STOP_REASONS[mode]), census
    assert why[64] == census.most_common(1)[0][0]
    for i in range(65):
        assert (ns[i] == len(TIMES)) == (why[i] == 'full')
        assert np.isfinite(margins[i, 0, 0]) and (why[i] in ('image', 'full')) == np.isfinite(margins[i, 0, 1])
    g = golden('trajgen_edges.npz')
    key = 'stop/%s/%s' % (mode, direction)
    assert np.array_equal(g[key + '/seeds'], seeds) and np.array_equal(g[key + '/n_saved'], ns)
    assert [T.STOP_REASONS[r] for r in g[key + '/reason']] == why and np.array_equal(g[key + '/margins'], margins)
    print('%s/%s: %s, smallest margins %.3g m %.3g px' % (mode, direction, dict(census), margins[:, :, 0].min(), margins[:, :, 1].min()))


def test_simulate_takes_a_camera(golden):
    """`camera=`: with the principal point moved 300 px only the image rule changes: a track that now stops earlier stops for
    the image, one that now runs longer had stopped for the image."""
    mode, direction = C.CAMERA_COMBO
    g = golden('trajgen_edges.npz')
    seeds = C.stop_seeds(mode, direction)
    _, _, _, ns, why, margins = T.simulate(seeds, mode, direction, camera=C.shifted_camera(), want_stop=True)
    assert margins[:, :, 0].min() >= C.STOP_MARGIN_M and margins[:, :, 1].min() >= C.STOP_MARGIN_PX          # the GPU test's seeds under this camera too
    assert np.array_equal(g['stop_camera/n_saved'], ns) and np.array_equal(g['stop_camera/margins'], margins)
    assert [T.STOP_REASONS[r] for r in g['stop_camera/reason']] == why
    ns0 = g['stop/%s/%s/n_saved' % (mode, direction)]
    why0 = [T.STOP_REASONS[r] for r in g['stop/%s/%s/reason' % (mode, direction)]]
    assert (ns != ns0).sum() >= 10
    assert all(w == 'image' for w, a, b in zip(why, ns, ns0) if a < b)
    assert all(w == 'image' for w, a, b in zip(why0, ns, ns0) if a > b)
    assert any(w == 'image' and 0 < n < len(TIMES) for w, n in zip(why, ns))
