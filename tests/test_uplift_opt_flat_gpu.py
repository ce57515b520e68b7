"""The raw optimizer step on flat device buffers (ttup_opt_flat_step, csrc/uplift_opt.hip) against torch on CPU tensors:
torch.nn.utils.clip_grad_norm_, torch.optim.Adam with loaded exp_avg / exp_avg_sq / step, and update_ema's formula.

Metric: the largest distance of param, exp_avg, exp_avg_sq and ema from torch's result in units in the last place of torch's value.
The kernel restates torch's CPU operation order, its two fused multiply-adds included, and the aim is bit equality.  BARS:
  exp_avg, exp_avg_sq, ema   0 ulp: bit equality.
  param                      2 ulp = twice the measured worst (1 ulp, on about one entry per million).  The operation that differs
                             is `exp_avg_sq.sqrt()`: torch's CPU sqrt is a vector-library routine that is not correctly rounded
                             (it differs from IEEE sqrt in the last place on 0.8 % of the entries), the device's sqrtf is.  The
                             quotient exp_avg / denom then differs in its last place there, which now and then moves the rounding
                             of param + quotient.  The inputs keep |param| >= 0.5, some 50 times the largest update: where an
                             update cancels its parameter, one ulp of the QUOTIENT is many ulps of the small result (16 were
                             measured with param ~ N(0, 1)), and the distance in ulps of the value says nothing about the kernel.
The norm is held to 2^-23 of a float64 sum of the same fp32 gradients (the device accumulates in fp64).

Clipping: torch adds the squares in fp32, so its own norm -- and with it the coefficient every gradient entry is multiplied by --
may differ from the device's in the last place (it does in 141 of the 252 clipped cases below, for lengths from 4 up).  A distance in
ulps between results computed from different coefficients measures nothing: where exp_avg's update cancels, one ulp of the
coefficient is 1.9e6 ulps of the result.  So where the two norms are not the same bits, torch's clipping is run on the DEVICE's
norm (torch.nn.utils.clip_grads_with_norm_, the second half of clip_grad_norm_) and the same bars hold; torch's own norm is then held
to the error bound of its fp32 sum.  Where the norms agree, the comparison is with clip_grad_norm_ itself.

Every buffer sits between guard words that must come back untouched, once 16-byte aligned (four guard words: the kernels built for
aligned buffers, whose accesses are 16-byte loads and stores) and once not (one guard word: the kernels for any 4-byte alignment,
written word by word -- the compiler merges those words into wider unaligned accesses, which the hardware takes); both must give
the same bits.  The bars hold for well-conditioned updates only (|param| >= 0.5, above)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import has_gpu

pytestmark = pytest.mark.gpu
if has_gpu():
    from upliftingtabletennis_amd import _lib

HYPER = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, ema_decay=0.999, max_norm=5.0)
BLOCK = 256 * 4                    # parameters per block of the fused pass (OPT_THREADS x 4)
SQSUM_SPAN = 1024 * BLOCK          # gradient entries one sweep of the norm's grid covers (OPT_MAX_BLOCKS blocks)
SIZES = [1, 3, 4, 5, 255, 256, 257, 1023, 1025, 70001, BLOCK, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1]
STEPS = (1, 2, 1000)
NORMS = (2.5, 50.0)                # below / above max_norm: clipping inactive / active
BARS = {'param': 2, 'exp_avg': 0, 'exp_avg_sq': 0, 'ema': 0}          # ulps (module docstring)
BAR_NORM = 2.0 ** -23
GUARD = 1.0e30


def holes(n):
    return [(0, 0), (0, 7), (min(5, n), 3), (n, 4), (n - 1, 1), (n // 2, n + 9)]


def make_inputs(n, hole, norm, seed, hole_nonzero=True):
    """Seeded param, gradient (n + hole entries, scaled to `norm`), exp_avg (either sign), exp_avg_sq (>= 0) and ema.  param and ema
    are drawn away from zero, 0.5 <= |x| < 2, and exp_avg_sq from [0.0025, 0.01), so that an update (at most 1e-2 here) never
    cancels its parameter: the distance in ulps of the value is then a well-conditioned measure (module docstring)."""
    rng = np.random.default_rng(seed)
    f = np.float32
    p, e = [(rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)).astype(f) for _ in range(2)]
    m, v = (0.1 * rng.standard_normal(n)).astype(f), rng.uniform(0.0025, 0.01, n).astype(f)
    g = rng.standard_normal(n + hole[1])
    if not hole_nonzero:
        g[hole[0]:hole[0] + hole[1]] = 0
    g = (g * (norm / np.linalg.norm(g))).astype(f)
    return p, g, m, v, e


def torch_step(p, g, m, v, e, hole, step, hyper=HYPER, total_norm=None):
    """-> (param, exp_avg, exp_avg_sq, ema, norm) after clip_grad_norm_, Adam.step() and the EMA on CPU tensors.  The hole's entries are
    a second parameter's gradient for the clipping -- they count towards the norm -- and belong to no parameter of the optimizer.
    total_norm: clip with torch.nn.utils.clip_grads_with_norm_ on that norm (the second half of clip_grad_norm_) instead."""
    hb, hl = hole
    P = torch.nn.Parameter(torch.from_numpy(p.copy()))
    P.grad = torch.from_numpy(np.concatenate([g[:hb], g[hb + hl:]]))
    params = [P]
    if hl:
        H = torch.nn.Parameter(torch.zeros(hl))
        H.grad = torch.from_numpy(g[hb:hb + hl].copy())
        params.append(H)
    if total_norm is None:
        norm = torch.nn.utils.clip_grad_norm_(params, hyper['max_norm'])
    else:
        norm = torch.tensor(total_norm, dtype=torch.float32)
        torch.nn.utils.clip_grads_with_norm_(params, hyper['max_norm'], norm)
    opt = torch.optim.Adam([P], lr=hyper['lr'], betas=hyper['betas'], eps=hyper['eps'])
    opt.state[P] = {'step': torch.tensor(float(step - 1)), 'exp_avg': torch.from_numpy(m.copy()), 'exp_avg_sq': torch.from_numpy(v.copy())}
    opt.step()
    with torch.no_grad():
        ema = hyper['ema_decay'] * torch.from_numpy(e.copy()) + (1 - hyper['ema_decay']) * P.data
    return P.detach().numpy(), opt.state[P]['exp_avg'].numpy(), opt.state[P]['exp_avg_sq'].numpy(), ema.numpy(), float(norm)


def device_step(p, g, m, v, e, hole, step, guard, hyper=HYPER):
    """The same on the device, every buffer between `guard` guard words on either side -> (param, m, v, ema, norm)."""
    lib = _lib.load()

    def padded(a):
        return torch.from_numpy(np.concatenate([np.full(guard, GUARD, np.float32), a, np.full(guard, GUARD, np.float32)])).cuda()
    bufs = [padded(a) for a in (p, g, m, v, e)]
    scratch = torch.zeros(int(lib.ttup_opt_flat_scratch_bytes()) // 4, dtype=torch.float32, device='cuda')
    norm = padded(np.zeros(1, np.float32))
    ptrs = [ctypes.c_void_p(b.data_ptr() + 4 * guard) for b in bufs]
    _lib.check(lib.ttup_opt_flat_step(*ptrs, p.size, hole[0], hole[1], hyper['lr'], *hyper['betas'], hyper['eps'], hyper['ema_decay'], hyper['max_norm'], step,
                                      _lib.ptr(scratch), ctypes.c_void_p(norm.data_ptr() + 4 * guard), _lib.stream_ptr()))
    out = [b.cpu().numpy() for b in bufs + [norm]]
    for o in out:
        assert (o[:guard] == np.float32(GUARD)).all() and (o[-guard:] == np.float32(GUARD)).all(), 'a guard word was overwritten'
    assert np.array_equal(out[1][guard:-guard], g), 'the gradient buffer was written to'
    return out[0][guard:-guard], out[2][guard:-guard], out[3][guard:-guard], out[4][guard:-guard], float(out[5][guard])


def ulps(got, ref):
    """largest distance in units in the last place, over the entries that are finite in the reference (the others must match in kind)"""
    def ordered(a):
        i = a.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    return int(np.abs(ordered(got[fin]) - ordered(ref[fin])).max()) if fin.any() else 0


def run_case(n, hole, step, norm, seed, worst, inputs=None):
    p, g, m, v, e = inputs if inputs is not None else make_inputs(n, hole, norm, seed, hole_nonzero=hole != (0, 7))
    exact = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    aligned = device_step(p, g, m, v, e, hole, step, 4)
    unaligned = device_step(p, g, m, v, e, hole, step, 1)
    for a, u in zip(aligned, unaligned):
        assert np.array_equal(a, u, equal_nan=True), 'the 16-byte and the scalar access paths differ (n %d hole %s)' % (n, hole)
    clipped = exact > HYPER['max_norm']
    if np.isfinite(exact):
        assert abs(aligned[4] - exact) <= BAR_NORM * exact, (n, hole, aligned[4], exact)
    ref = torch_step(p, g, m, v, e, hole, step)
    own_norm = clipped and np.float32(ref[4]) != np.float32(aligned[4])
    if own_norm:
        # torch's fp32 sum of n squares in vector lanes of at least 8: off by at most (n / 8 + 8) roundings of 2^-24, half of it in the root
        assert abs(ref[4] - exact) <= ((g.size / 8 + 8) * 2.0 ** -25 + 2.0 ** -23) * exact, (n, hole, ref[4], exact)
        ref = torch_step(p, g, m, v, e, hole, step, total_norm=aligned[4])
    worst['device norm'] = worst.get('device norm', 0) + int(own_norm)
    for name, got, want in zip(('param', 'exp_avg', 'exp_avg_sq', 'ema'), aligned, ref):
        d = ulps(got, want)
        key = (name, clipped)
        if d > worst.get(key, (-1,))[0]:
            worst[key] = (d, n, hole, step)
    return aligned


def check(worst, what):
    own = worst.pop('device norm', 0)
    print(what + ': ' + '; '.join('%s %s: %d ulp (n %d hole %s step %d)' % ((k[0], 'clipped' if k[1] else 'unclipped') + worst[k]) for k in sorted(worst))
          + '; %d cases clipped by torch on the device\'s norm' % own)
    for (name, clipped), (d, n, hole, step) in worst.items():
        assert d <= BARS[name], '%s is %d ulp from torch (n %d hole %s step %d, clipping %s)' % (name, d, n, hole, step, clipped)


@pytest.mark.parametrize('n', SIZES)
def test_step_matches_torch(n):
    """Every hole form x steps 1, 2, 1000 x both norms, on aligned and unaligned buffers."""
    worst = {}
    for hi, hole in enumerate(holes(n)):
        for step in STEPS:
            for norm in NORMS:
                run_case(n, hole, step, norm, 1000 * n + 10 * hi + step % 7, worst)
    check(worst, 'n %d' % n)


def test_more_than_one_sweep_of_the_norm_grid():
    """n past what the norm's 1024 blocks cover in one sweep: its grid-stride loop runs twice for some threads."""
    worst = {}
    n = SQSUM_SPAN + 5
    for norm in NORMS:
        run_case(n, (128, 17024 + 3), 3, norm, 77, worst)
    check(worst, 'n %d' % n)


def test_zero_gradient_stretch_divides_by_eps():
    """g = 0 and exp_avg_sq = 0 on a stretch: denom = eps, the update is -step_size * exp_avg / eps; bit-equal to torch."""
    n, hole = 1025, (5, 3)
    p, g, m, v, e = make_inputs(n, hole, 2.5, 5)
    g[300 + hole[1]:700 + hole[1]] = 0
    v[300:700] = 0
    worst = {}
    for step in STEPS:
        got = run_case(n, hole, step, None, 0, worst, inputs=(p, g, m, v, e))
        assert (got[2][300:700] == 0).all() and np.isfinite(got[0]).all()
        assert np.abs(got[0][300:700] - p[300:700]).max() > 100          # lr * m / 1e-8: far from a usual step
    check(worst, 'zero stretch')


def test_nonfinite_gradient_propagates_as_in_torch():
    n, hole = 257, (5, 3)
    p, g, m, v, e = make_inputs(n, hole, 2.5, 6)
    g[100] = np.inf
    worst = {}
    got = run_case(n, hole, 2, None, 0, worst, inputs=(p, g, m, v, e))
    assert np.isinf(got[4]) and np.isnan(got[0][100 - hole[1]]) and np.isfinite(np.delete(got[0], 100 - hole[1])).all()
    check(worst, 'inf in the gradient')


def test_hole_entries_count_towards_the_norm_and_touch_no_parameter():
    """The same parameters' gradients with and without a non-zero hole: the norm grows by the hole's share, and with clipping inactive
    no parameter changes a bit."""
    n, hole = 1023, (5, 3)
    p, g, m, v, e = make_inputs(n, hole, 2.5, 8)
    g0 = g.copy()
    g0[5:8] = 0
    a, b = device_step(p, g, m, v, e, hole, 2, 4), device_step(p, g0, m, v, e, hole, 2, 4)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    want = np.sqrt(b[4] ** 2 + float((g[5:8].astype(np.float64) ** 2).sum()))
    assert a[4] > b[4] and abs(a[4] - want) <= 4 * BAR_NORM * want


def test_two_calls_return_the_same_bits():
    for n, hole in ((70001, (5, 3)), (SQSUM_SPAN + 5, (0, 7))):
        p, g, m, v, e = make_inputs(n, hole, 50.0, 9)
        a, b = device_step(p, g, m, v, e, hole, 3, 4), device_step(p, g, m, v, e, hole, 3, 4)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
