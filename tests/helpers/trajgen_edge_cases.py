"""Crafted position tracks for the trajectory generator's selection rules (csrc/trajgen.hip select_kernel against
oracle/trajgen_ref.select), and the seed lists for its stop rules.  No GPU, no reference tree.

A track is built from a short script: a straight base line (x from the own side to the opponent's, constant y and z,
high enough that nothing counts as a hit and the net is cleared) plus `dips` (start, length, depth pattern, kind) that
pull z below a hit threshold -- 'own' / 'opp' on the table halves, 'ground' beside the table -- plus single-sample
overrides (`set`).  Scripts are written for 'left_to_right' (own side x > 0, opponent's x < 0); the other direction is
the exact mirror x -> -x, so both directions' masks see the same values.  The base line never comes closer than 0.05 m
to the net plane, so the net rule is engaged by net probes only.

Every named case carries the label pair `oracle.trajgen_ref.select(..., why=[])` must give: the rule that decides and the
cut branch taken.  The labels are written down from the reference's rules (mujocosimulation.py:152-219), not read off
the oracle; tests/test_trajgen_edges_host.py checks them.

What the reference's arithmetic makes unreachable (and is therefore not among the cases):
  * a hit time equal to a time label at or after 0.2 s: the labels accumulate 1/FPS in floating point and from label 9 on
    differ from k/FPS, while hit times are 0.75 * mid + 0.25 * low of exact k/FPS values (searched over every interval of
    up to 8 samples, `hit_time_equals_a_label`); before 0.2 s no cut rule looks a time up;
  * a cut index at or beyond the track's length: the index counts labels among times[:len], so it is at most len - 1;
    the latest possible cut (a one-sample hit at len - 2) is the 'cut/*/latest' case;
  * a difference between `>= 0.2` and `> 0.2` in the cut-time gate: a hit at exactly 0.2 s cuts to 99 frames (label 100
    is 0.2 + 1.5e-16), which rejects; left uncut it stays in its list, and every arm's list then holds one hit more than
    the mode accepts, which rejects too.  The 'cut/*/at_0.2' cases pin the first half (rule and arm under the oracle);
    the device's outputs cannot tell the two operators apart;
  * two equal bounce times: hit intervals of the two table halves are disjoint and ordered, so are their midpoints and
    minima; the sort is exercised by own-before-opponent order (it moves entries) and the reverse.
"""
import numpy as np

from oracle import trajgen_ref as T

MODES, DIRECTIONS = T.MODES, T.DIRECTIONS
S = 500                                     # ttup_trajgen_max_samples(): never build a longer track
WHY = ['too_short', 'too_high', 'cut_too_short', 'net', 'last_side', 'counts', 'accepted']
CUT_BRANCHES = ['none', 'ground', 'opponent_extra', 'own_extra', 'opponent_first']
BRANCHES = {'final_lose': ['none', 'ground'], 'intermediate': ['none', 'ground'], 'first_long': ['none', 'ground'],
            'final_win': ['none', 'opponent_extra', 'ground'], 'first_good': ['none', 'opponent_extra', 'ground'],
            'first_short': ['none', 'own_extra', 'opponent_first', 'ground']}
HITS = {'final_lose': [], 'final_win': ['opp', 'opp'], 'intermediate': ['opp'], 'first_good': ['own', 'opp'],
        'first_short': ['own', 'own'], 'first_long': ['own']}           # the hits of an accepted track, in time order
CUTTER = {'ground': 'ground', 'opponent_extra': 'opp', 'own_extra': 'own', 'opponent_first': 'opp'}
LAST_SIDE_MODES = ('final_lose', 'first_long')
TABLE_DEPTHS, GROUND_DEPTHS = (0.78, 0.77, 0.78), (0.05, 0.03, 0.05)
SIDE_X = 0.7                                # |x| of a table dip
OK = ('accepted', 'none')

# What one more hit BEFORE 0.2 s does to `base(mode)` (hits at samples 130 and 180, no cut):
#   opponent: final_win [p, a, b] -> the third is b >= 0.2: cut there, two remain; first_good [p, b] -> cut at b, one remains;
#             everywhere else the count is off by one and no arm looks at the opponent list
#   own:      first_short [p, a, b] -> cut at b, two remain; everywhere else the count is off by one
#   ground:   its time is below 0.2, so no arm cuts and the ground count of 1 rejects
EXTRA_EARLY = {m: {'opp': ('counts', 'none'), 'own': ('counts', 'none'), 'ground': ('counts', 'none')} for m in MODES}
EXTRA_EARLY['final_win']['opp'] = ('accepted', 'opponent_extra')
EXTRA_EARLY['first_good']['opp'] = ('accepted', 'opponent_extra')
EXTRA_EARLY['first_short']['own'] = ('accepted', 'own_extra')
# a table hit before 0.2 s that spoils the counts of `base(mode, branch)` without touching the list its arms read
COUNT_BREAKER = {'final_lose': 'own', 'intermediate': 'own', 'first_long': 'opp', 'final_win': 'own', 'first_good': 'own'}


def dip(kind, start, length=3, depths=None):
    return (start, length, tuple(depths) if depths is not None else (GROUND_DEPTHS if kind == 'ground' else TABLE_DEPTHS), kind)


def script(n=300, x=(1.2, -1.2), dips=(), sets=()):
    return {'n': n, 'x': x, 'y': 0.2, 'z': 1.0, 'dips': list(dips), 'set': list(sets)}


def extend(sc, dips=(), sets=()):
    return {**sc, 'dips': sc['dips'] + list(dips), 'set': sc['set'] + list(sets)}


def build_track(sc, direction):
    """(n, 3) float64 positions of a script.  Dips are applied in order, then the single-sample overrides (index, axis, value;
    negative indices count from the end)."""
    n = sc['n']
    assert 1 <= n <= S
    x = np.linspace(sc['x'][0], sc['x'][1], n)
    near = np.abs(x) < 0.05
    x[near] = np.where(x[near] >= 0, 0.05, -0.05)
    p = np.stack([x, np.full(n, sc['y']), np.full(n, sc['z'])], axis=1)
    for start, length, depths, kind in sc['dips']:
        for j in range(length):
            i = start + j
            if not 0 <= i < n:
                continue
            p[i, 2] = depths[j % len(depths)]
            if kind == 'ground':
                p[i, 1] = 1.0
            else:
                p[i, 0], p[i, 1] = (SIDE_X if kind == 'own' else -SIDE_X), sc['y']
    for i, axis, value in sc['set']:
        p[i, axis] = value
    if direction == 'right_to_left':
        p[:, 0] = -p[:, 0]
    return p


def base(mode, branch='none', early=False, n=300, cut_at=230):
    """A track `mode` accepts through `branch`: its hits at samples 130 and 180 (early: 20 and 50, before 0.2 s, on a line
    that stays on the opponent's side so that a cut near sample 100 still ends there), the cutting hit at `cut_at`."""
    starts = (20, 50) if early else (130, 180)
    dips = [dip(k, s) for k, s in zip(HITS[mode], starts)]
    if branch != 'none':
        assert branch in BRANCHES[mode]
        dips.append(dip(CUTTER[branch], cut_at))
    return script(n, (-0.3, -1.2) if early else (1.2, -1.2), dips)


def three(v):
    return (('eq', v), ('up', np.nextafter(v, np.inf)), ('dn', np.nextafter(v, -np.inf)))


def _case(out, mode, direction, name, sc, label, keep=None):
    out.append({'name': '%s/%s/%s' % (mode, direction, name), 'mode': mode, 'direction': direction, 'script': sc,
                'why': label[0], 'branch': label[1], 'keep': keep})


def named_cases(mode, direction):
    """The named cases of one mode x direction: list of {'name', 'mode', 'direction', 'script', 'why', 'branch', 'keep'}
    (`keep`: the kept length where the case is about it, else None)."""
    out = []

    def add(name, sc, label, keep=None):
        _case(out, mode, direction, name, sc, label, keep)
    U = base(mode)
    sided = mode in LAST_SIDE_MODES
    # ---- one accepted track per cut branch (uncut included)
    for b in BRANCHES[mode]:
        add('base/%s' % b, base(mode, b), ('accepted', b))
    # ---- lengths
    for n in (99, 100, 101, S):
        add('len/%d' % n, base(mode, early=True, n=n), ('too_short', 'none') if n < 100 else OK, keep=n if n >= 100 else None)
    add('len/late_%d' % S, base(mode, n=S), OK, keep=S)
    # ---- hit-mask thresholds: one probe sample (20) before 0.2 s whose membership hangs on one comparison
    half_l, half_w = T.TABLE_LENGTH / 2, T.TABLE_WIDTH / 2

    def probe(x, y, z):
        return [(20, 0, x), (20, 1, y), (20, 2, z)]
    for tag, v in three(T.HIT_X_MARGIN):            # next to the net plane: sample 21 (z = 1.0) keeps the net rule satisfied
        add('thr/x_own_margin/' + tag, extend(U, sets=probe(v, 0.2, 0.78) + [(21, 0, 0.02)]), EXTRA_EARLY[mode]['own'] if v > T.HIT_X_MARGIN else OK)
        add('thr/x_opp_margin/' + tag, extend(U, sets=probe(-v, 0.2, 0.78) + [(21, 0, -0.02)]), EXTRA_EARLY[mode]['opp'] if v > T.HIT_X_MARGIN else OK)
    for tag, v in three(half_l):
        add('thr/x_own_end/' + tag, extend(U, sets=probe(v, 0.2, 0.78)), EXTRA_EARLY[mode]['own'] if v < half_l else OK)
        add('thr/x_opp_end/' + tag, extend(U, sets=probe(-v, 0.2, 0.78)), EXTRA_EARLY[mode]['opp'] if v < half_l else OK)
    for tag, v in three(half_w):
        add('thr/y_own/' + tag, extend(U, sets=probe(SIDE_X, v, 0.78)), EXTRA_EARLY[mode]['own'] if v < half_w else OK)
        add('thr/y_opp/' + tag, extend(U, sets=probe(-SIDE_X, -v, 0.78)), EXTRA_EARLY[mode]['opp'] if v < half_w else OK)
    for tag, v in three(T.HIT_Z_TABLE):             # strict <
        add('thr/z_table_own/' + tag, extend(U, sets=probe(SIDE_X, 0.2, v)), EXTRA_EARLY[mode]['own'] if v < T.HIT_Z_TABLE else OK)
        add('thr/z_table_opp/' + tag, extend(U, sets=probe(-SIDE_X, 0.2, v)), EXTRA_EARLY[mode]['opp'] if v < T.HIT_Z_TABLE else OK)
    for tag, v in three(T.HIT_Z_GROUND):            # <=
        add('thr/z_ground/' + tag, extend(U, sets=[(20, 1, 1.0), (20, 2, v)]), EXTRA_EARLY[mode]['ground'] if v <= T.HIT_Z_GROUND else OK)
    zmax = 1.4 if 'first' in mode else 1.8
    for tag, v in three(zmax):
        add('thr/z_max/' + tag, extend(U, sets=[(30, 2, v)]), ('too_high', 'none') if v > zmax else OK)
    # ---- net rule: one sample (25) next to the net plane, below the net top and between the posts unless one value says otherwise
    net_h, net_w = T.NET_TOTAL_HEIGHT, T.NET_TOTAL_WIDTH / 2
    for tag, v in three(T.NET_CLEARANCE_X_MARGIN):
        for sgn, side in ((1.0, 'pos'), (-1.0, 'neg')):
            add('thr/net_x_%s/%s' % (side, tag), extend(U, sets=[(25, 0, sgn * v), (25, 2, 0.85)]), ('net', 'none') if v < T.NET_CLEARANCE_X_MARGIN else OK)
    for tag, v in three(net_h):
        add('thr/net_z/' + tag, extend(U, sets=[(25, 0, 0.02), (25, 2, v)]), ('net', 'none') if v < net_h else OK)
    for tag, v in three(net_w):
        add('thr/net_y/' + tag, extend(U, sets=[(25, 0, -0.02), (25, 1, v), (25, 2, 0.85)]), ('net', 'none') if v < net_w else OK)
    # ---- last x: zero and the smallest doubles (a signed zero is on neither side)
    tiny = 5e-324
    for tag, v in (('zero', 0.0), ('pos', tiny), ('neg', -tiny)):
        add('thr/last_x/' + tag, extend(U, sets=[(-1, 0, v)]), ('last_side', 'none') if sided and not v < 0 else OK)
    # ---- shapes of one hit interval: the first hit of the accepted track (final_lose has none: its cutting ground hit)
    P, plabel = (base(mode, 'ground'), ('accepted', 'ground')) if mode == 'final_lose' else (U, OK)
    s0, _, _, kind0 = P['dips'][0]
    hi, mid, lo = (0.07, 0.05, 0.02) if kind0 == 'ground' else (0.78, 0.75, 0.70)
    for name, depths in (('len1', (mid,)), ('tie', (hi, lo, mid, lo, hi)), ('min_first', (lo, mid, hi)), ('min_last', (hi, mid, lo)),
                         ('tie_at_ends', (lo, mid, lo))):
        add('hit/' + name, {**P, 'dips': [dip(kind0, s0, len(depths), depths)] + P['dips'][1:]}, plabel)
    for kind in ('own', 'opp', 'ground'):           # mask true at sample 0
        add('hit/start0/' + kind, extend(U, dips=[dip(kind, 0)]), EXTRA_EARLY[mode][kind])
        add('hit/start0_len1/' + kind, extend(U, dips=[dip(kind, 0, 1)]), EXTRA_EARLY[mode][kind])
    for kind in ('opp', 'ground'):                  # an interval that runs into the last sample is never closed: no hit
        add('hit/end_last/' + kind, extend(U, dips=[dip(kind, 297)]), OK)
        add('hit/end_last_len1/' + kind, extend(U, dips=[dip(kind, 299, 1)]), OK)
    # two intervals of one mask, one sample apart
    adjacent = {'final_lose': ('accepted', 'ground'),            # two ground hits: the first cuts, the list is cleared
                'final_win': ('accepted', 'opponent_extra'),     # [130, 134, 180]: cut at the third
                'intermediate': ('counts', 'none'), 'first_good': ('counts', 'none'), 'first_long': ('counts', 'none'),
                'first_short': ('accepted', 'own_extra')}        # [130, 134, 180]: cut at the third
    add('hit/adjacent', extend(P, dips=[dip(kind0, s0 + 4)]), adjacent[mode])
    # four and five hits of one mask (three slots are stored): nothing else on the track
    many = {'opp': {'final_lose': ('counts', 'none'), 'final_win': ('accepted', 'opponent_extra'), 'intermediate': ('counts', 'none'),
                    'first_good': ('counts', 'opponent_extra'),          # cut at the second, one remains, no own hit
                    'first_short': ('counts', 'opponent_first'),         # no third own hit; cut at the first opponent hit, no own hits
                    'first_long': ('counts', 'none')},
            'own': {m: ('counts', 'none') for m in MODES}}
    many['own']['first_short'] = ('accepted', 'own_extra')
    for kind in ('own', 'opp'):
        add('hit/four/' + kind, script(dips=[dip(kind, s) for s in (130, 160, 190, 220)]), many[kind][mode])
        add('hit/five/' + kind, script(dips=[dip(kind, s) for s in (120, 145, 170, 195, 220)]), many[kind][mode])
    # ---- cut times: the cutting hit of every arm around 0.2 s (0.75 * mid + 0.25 * low; label 100 is 0.2 + 1.5e-16)
    for b in BRANCHES[mode][1:]:
        E = base(mode, b, early=True)
        k = CUTTER[b]

        def at(start, length, depths=None, n=300):
            return {**E, 'n': n, 'dips': E['dips'][:-1] + [dip(k, start, length, depths)]}
        add('cut/%s/at_0.2' % b, at(100, 1), ('cut_too_short', b))                   # exactly 0.2: index 99, 99 frames
        add('cut/%s/at_0.2_wide' % b, at(98, 5, (0.05, 0.05, 0.02, 0.05, 0.05) if k == 'ground' else (0.78, 0.78, 0.7, 0.78, 0.78)), ('cut_too_short', b))
        add('cut/%s/half_below' % b, at(99, 2), ('counts', 'none'))                  # below 0.2: no arm fires, the hit stays counted
        add('cut/%s/half_above' % b, at(100, 2), ('accepted', b), keep=100)          # 0.20075: index 100, 100 frames
        add('cut/%s/between' % b, at(150, 1), ('accepted', b))
        add('cut/%s/latest' % b, at(298, 1), ('accepted', b))
        add('cut/%s/latest_%d' % (b, S), at(S - 2, 1, n=S), ('accepted', b))
    # ---- the arms behind the `else if`
    if mode == 'final_win':
        add('cascade/third_before_0.2_ground_decides', script(dips=[dip('opp', 20), dip('opp', 50), dip('opp', 80), dip('ground', 230)]), ('counts', 'ground'))
        add('cascade/extra_shadows_ground', script(dips=[dip('opp', 20), dip('opp', 50), dip('ground', 150), dip('opp', 230)]), ('accepted', 'opponent_extra'))
    if mode == 'first_good':
        add('cascade/second_before_0.2_ground_decides', script(dips=[dip('own', 20), dip('opp', 50), dip('opp', 80), dip('ground', 230)]), ('counts', 'ground'))
        add('cascade/extra_shadows_ground', script(dips=[dip('own', 20), dip('opp', 50), dip('ground', 150), dip('opp', 230)]), ('accepted', 'opponent_extra'))
        add('sort/opponent_first', script(dips=[dip('opp', 130), dip('own', 180)]), OK)          # `base` has own first: there the sort moves an entry
    if mode == 'first_short':
        add('cascade/third_own_before_0.2_opponent_decides', script(dips=[dip('own', 20), dip('own', 50), dip('own', 80), dip('opp', 230)]), ('counts', 'opponent_first'))
        add('cascade/opponent_before_0.2_ground_decides', script(dips=[dip('own', 20), dip('own', 50), dip('opp', 80), dip('ground', 230)]), ('counts', 'ground'))
        add('cascade/own_extra_shadows_both', script(dips=[dip('own', 20), dip('own', 50), dip('opp', 150), dip('ground', 170), dip('own', 200)]), ('accepted', 'own_extra'))
        add('cascade/opponent_shadows_ground', script(dips=[dip('own', 20), dip('own', 50), dip('ground', 150), dip('opp', 200)]), ('accepted', 'opponent_first'))
    # ---- every rejection after every arm
    for b in BRANCHES[mode]:
        B = base(mode, b)
        add('rej/net/%s' % b, extend(B, sets=[(25, 0, 0.02), (25, 2, 0.85)]), ('net', b))
        if mode == 'first_short':
            if b == 'none':
                add('rej/counts/none', extend(B, dips=[dip('opp', 20)]), ('counts', 'none'))
            elif b != 'own_extra':                  # own_extra leaves exactly (0, 2, 0): see required_coverage()
                add('rej/counts/%s' % b, script(dips=[dip('own', 130), dip(CUTTER[b], 230)]), ('counts', b))
        else:
            add('rej/counts/%s' % b, extend(B, dips=[dip(COUNT_BREAKER[mode], 20)]), ('counts', b))
        if sided:                                   # the last kept sample: the final one, or the one before the cut (index 230)
            add('rej/last_side/%s' % b, extend(B, sets=[(i, 0, 0.5) for i in ((-1,) if b == 'none' else range(224, 230))]), ('last_side', b))
    return out


def all_named_cases():
    return [c for m in MODES for d in DIRECTIONS for c in named_cases(m, d)]


def track(case):
    return build_track(case['script'], case['direction'])


# ---------------------------------------------------------------- random sweep
def random_tracks(mode, direction, count=1000, seed=20240):
    """Seeded tracks from the same building blocks, the threshold values among the choices.  Half start from an accepted
    `base` and are perturbed, half are free-form.  Returns a list of (n, 3) arrays."""
    rng = np.random.default_rng([seed, MODES.index(mode), DIRECTIONS.index(direction)])

    def pick(seq):
        return seq[int(rng.integers(len(seq)))]
    below = lambda v: float(np.nextafter(v, -np.inf))
    table_z = [0.78, 0.77, 0.70, 0.75, below(T.HIT_Z_TABLE), T.HIT_Z_TABLE]
    ground_z = [0.05, 0.03, 0.02, T.HIT_Z_GROUND, float(np.nextafter(T.HIT_Z_GROUND, 1.0))]
    zmax = 1.4 if 'first' in mode else 1.8
    out = []
    for _ in range(count):
        n = pick([99, 100, 101, 120, 150, 200, 300, 300, 300, S])
        if rng.random() < 0.5:
            sc = base(mode, pick(BRANCHES[mode]), early=bool(rng.random() < 0.5), n=n, cut_at=pick([100, 101, 110, 150, 230]))
        else:
            sc = script(n, pick([(1.2, -1.2), (-0.3, -1.2), (0.5, -1.2), (1.2, 0.3)]))
        dips, sets = [], []
        for _ in range(int(rng.integers(0, 5))):
            kind = pick(['own', 'opp', 'ground'])
            start = pick([0, 1, 20, 50, 80, 97, 98, 99, 100, 101, 130, 134, 150, 180, 184, 200, 230, n - 4, n - 3, n - 2, n - 1])
            length = pick([1, 1, 2, 3, 3, 5])
            depths = [pick(ground_z if kind == 'ground' else table_z) for _ in range(length)]
            dips.append(dip(kind, start, length, depths))
        if rng.random() < 0.3:
            i = pick([25, 60, n - 1])
            sets += [(i, 0, pick([0.02, -0.02, T.NET_CLEARANCE_X_MARGIN, below(T.NET_CLEARANCE_X_MARGIN), -below(T.NET_CLEARANCE_X_MARGIN)])),
                     (i, 1, pick([0.2, -0.2, T.NET_TOTAL_WIDTH / 2, below(T.NET_TOTAL_WIDTH / 2), 0.95])),
                     (i, 2, pick([0.85, 0.85, T.NET_TOTAL_HEIGHT, below(T.NET_TOTAL_HEIGHT), 1.0]))]
        if rng.random() < 0.15:
            sets.append((pick([30, n - 1]), 2, pick([zmax, float(np.nextafter(zmax, np.inf)), below(zmax), 1.3])))
        if rng.random() < 0.25:
            sets.append((pick([-1, 99, 100, 229]) if n > 229 else -1, 0, pick([0.0, 5e-324, -5e-324, 0.3, -0.3])))
        out.append(build_track(extend(sc, dips, sets), direction))
    return out


# ---------------------------------------------------------------- coverage table
def required_coverage():
    """{(mode, why, cut branch): None if some track must reach it, else the one-line reason why none can}, over all
    6 x 7 x 5 triples."""
    table = {}
    for mode in MODES:
        for why in WHY:
            for b in CUT_BRANCHES:
                reason = None
                if b not in BRANCHES[mode]:
                    reason = "the mode's cut cascade has no such arm"
                elif why in ('too_short', 'too_high') and b != 'none':
                    reason = 'decided before the cut rules run'
                elif why == 'cut_too_short' and b == 'none':
                    reason = 'without a cut the length is unchanged and was already at least 100'
                elif why == 'last_side' and mode not in LAST_SIDE_MODES:
                    reason = 'the last-side rule applies to final_lose and first_long only'
                elif (mode, why, b) == ('first_short', 'counts', 'own_extra'):
                    reason = 'that arm leaves exactly two own hits and clears both other lists: (0, 2, 0) is what first_short wants'
                table[(mode, why, b)] = reason
    return table


def hit_time_equals_a_label(max_len=8):
    """Every (start, end, argmin) whose hit time is >= 0.2 and equals one of the sampling loop's labels bit for bit."""
    labels = set(T.save_times().tolist())
    found = []
    for s in range(0, S - 1):
        for e in range(s, min(s + max_len, S - 1)):
            for a in range(s, e + 1):
                t = T.HIT_W[0] * ((e + s) / 2 / T.FPS) + T.HIT_W[1] * (a / T.FPS)
                if t >= 0.2 and t in labels:
                    found.append((s, e, a))
    return found


# ---------------------------------------------------------------- seeds for the stop rules
# Per mode x direction 65 seeds (one full workgroup and one lane of a second): the smallest seeds whose oracle margins
# (oracle.trajgen_ref.simulate(want_stop=True)) are at least STOP_MARGIN_M / STOP_MARGIN_PX at the deciding sample, the one before
# it and every earlier one -- `exclude` lists the seeds skipped for that -- plus `force`d ones where a stop reason is rare
# among the small seeds.  `last` is a seed of the list's most common reason, moved to lane 64.
STOP_MARGIN_M, STOP_MARGIN_PX = 1e-4, 0.05
N_STOP_SEEDS = 65
_SEED_RULES = {
    ('final_lose', 'left_to_right'): {'force': [134, 206, 393], 'exclude': [3, 37, 56], 'last': 64},
    ('final_lose', 'right_to_left'): {'force': [221], 'exclude': [40], 'last': 57},
    ('final_win', 'left_to_right'): {'force': [], 'exclude': [], 'last': 62},
    ('final_win', 'right_to_left'): {'force': [], 'exclude': [17, 40, 61], 'last': 67},
    ('intermediate', 'left_to_right'): {'force': [], 'exclude': [3, 42], 'last': 62},
    ('intermediate', 'right_to_left'): {'force': [], 'exclude': [17, 40], 'last': 64},
    ('first_good', 'left_to_right'): {'force': [], 'exclude': [16], 'last': 65},
    ('first_good', 'right_to_left'): {'force': [], 'exclude': [1, 44, 62], 'last': 67},
    ('first_short', 'left_to_right'): {'force': [], 'exclude': [60], 'last': 64},
    ('first_short', 'right_to_left'): {'force': [], 'exclude': [18, 44, 56], 'last': 65},
    ('first_long', 'left_to_right'): {'force': [], 'exclude': [16], 'last': 65},
    ('first_long', 'right_to_left'): {'force': [], 'exclude': [1, 44, 62], 'last': 67},
}
# the stop reasons each mode's rule can give ('image' and 'full' always); intermediate's z bound of -1 m lies below the
# ground plane, which the ball cannot pass, so it has no reachable oob_z
STOP_REASONS = {m: ['oob_x', 'oob_y'] + (['oob_z'] if m in ('final_win', 'first_short') else []) + ['image', 'full'] for m in MODES}


def stop_seeds(mode, direction):
    rule = _SEED_RULES[(mode, direction)]
    skip = set(rule['exclude']) | set(rule['force'])
    fill = [s for s in range(400) if s not in skip][:N_STOP_SEEDS - len(rule['force'])]
    seeds = sorted(fill + rule['force'])
    seeds.remove(rule['last'])
    return seeds + [rule['last']]


CAMERA_COMBO = ('intermediate', 'left_to_right')          # its seed list keeps the same margins under `shifted_camera()`


def shifted_camera(du=-300.0, dv=0.0):
    """The fixed camera with its principal point moved by (du, dv) pixels: other tracks leave the image, at other samples."""
    ex, mint = T.camera_matrices()
    mint = mint.copy()
    mint[0, 2] += du
    mint[1, 2] += dv
    return ex, mint
