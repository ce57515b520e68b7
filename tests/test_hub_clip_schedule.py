"""CPU-only check of the overlapped clip path's schedule (`interface.clip_schedule`: chunk bounds, the ball calls issued after each
upload, the aux ball detector's ranges): against the expressions `TableTennisPipeline._clip_detections` held inline before the
schedule became a function -- transcribed below, not imported -- and against the properties the clip path relies on."""
import pytest

from upliftingtabletennis_amd.interface import TableTennisPipeline, clip_schedule

SETTINGS = {'defaults': dict(chunk=24, chunk_long=64, first=24, max_batch=64),
            'chunk16_first8': dict(chunk=16, chunk_long=64, first=8, max_batch=64),
            'max_batch32': dict(chunk=24, chunk_long=64, first=24, max_batch=32)}


def _inline_schedule(n, CHUNK, CHUNK_LONG, FIRST, max_batch):
    """The loop of the former `_clip_detections` with the GPU work taken out: what it uploaded, and the frame ranges it handed to
    the ball detector and to the aux ball detector after each upload."""
    C = CHUNK if n < 4 * CHUNK else CHUNK_LONG
    F0 = min(FIRST, C, n)
    bounds = [0, F0] + list(range(F0 + C, n, C)) + ([n] if n > F0 else [])
    bounds = sorted(set(bounds))
    ball, aux = [], []
    t_next = a_next = 0
    for ci, (c0, c1) in enumerate(zip(bounds[:-1], bounds[1:])):
        ball.append([])
        while t_next < c1 - 2:
            nt = min(max_batch, c1 - 2 - t_next)
            ball[-1].append((t_next, t_next + nt + 2))
            t_next += nt
        aux.append(None)
        if a_next < c1 - 2:
            aux[-1] = (a_next, c1)
            a_next = c1 - 2
    return bounds, ball, aux


def test_defaults_are_the_pipelines():
    assert (TableTennisPipeline.CHUNK, TableTennisPipeline.CHUNK_LONG, TableTennisPipeline.FIRST) == (24, 64, 24)


@pytest.mark.parametrize('name', list(SETTINGS))
def test_schedule_equals_the_inline_loop_and_covers_the_clip(name):
    s = SETTINGS[name]
    for n in range(1, 301):
        bounds, ball, aux = clip_schedule(n, **s)
        assert (bounds, ball, aux) == _inline_schedule(n, s['chunk'], s['chunk_long'], s['first'], s['max_batch']), n
        # the uploads: 0 .. n in strictly increasing steps, one list of calls and one aux range per chunk
        assert bounds[0] == 0 and bounds[-1] == n and all(a < b for a, b in zip(bounds[:-1], bounds[1:])), (n, bounds)
        assert len(ball) == len(aux) == len(bounds) - 1
        # the ball calls: triples 0 .. n-3 exactly once and in order (a call on frames f0:f1 runs triples f0 .. f1-3), at most
        # max_batch per call, none before its last frame is uploaded
        triples = []
        for c1, calls in zip(bounds[1:], ball):
            for f0, f1 in calls:
                assert 1 <= f1 - f0 - 2 <= s['max_batch'] and f1 <= c1, (n, c1, f0, f1)
                triples += range(f0, f1 - 2)
        assert triples == list(range(n - 2)), n
        if n < 3:
            assert not any(ball) and not any(aux), n
        # the aux ball detector: one range per chunk over the same triples as that chunk's ball calls
        for c1, calls, a in zip(bounds[1:], ball, aux):
            assert a == ((calls[0][0], calls[-1][1]) if calls else None) and (a is None or a[1] == c1), (n, c1)
