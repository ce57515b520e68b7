"""The bf16 ViTPose path (csrc/gemm_bf16.h, csrc/vitpose_kernels.h; `ViTPoseNet(dtype='bf16')`) against its rounding oracle
(tests/helpers/vitpose_bf16_torch.py) over the sweep of tests/helpers/vitpose_bf16_cases.py.

No oracle reproduces a bf16 forward end to end -- twelve blocks amplify single rounding flips -- so the kernels are checked
(a) teacher-forced: every stage runs alone on the oracle's fp64-arithmetic residual stream (`run_stage`), and every stored tensor it
    leaves (`read_tap`) is compared with the oracle's fp64-arithmetic evaluation of the step that produced it FROM THE TENSORS THE
    DEVICE STORED BEFORE IT in that stage (qkv and ln from the stage's input, att from the device's qkv, x_attn from its att, ...).
    Forcing every step, not only every stage, keeps a difference where it arises: the device rounds the softmax numerators P to
    bf16 and the oracle does not, which moves att within the bound below and everything after it in the block by more than fp32
    round-off.  The allowance of a tap is not typed in: it is what the oracle's fp32- and fp64-arithmetic evaluations of that step
    differ by, times 3 (largest difference) and 2 (share of differing elements), over the floors of the case helper; a GEMM-fed
    bf16 tap is never more than one bf16 ulp off, and att stays within 2^-9 sum_j p_j |v_j| / l + 2^-9 |att| + the fp32 term.
    Both caps are met by construction, not by luck: the LN operands of qkv and fc1, which are stored nowhere and so cannot be
    forced, are evaluated in fp64 on the device (an fp32 LayerNorm lands on the other side of a rounding tie once in a few thousand
    operands and then moves a whole output row by up to 23 ulps), and p enters P V as two bf16 operands (one would cost up to 2^-8
    of each p, bf16's unit round-off, on top of att's own storage rounding of up to 2^-8 |att|; with two, the storage rounding
    alone is within the bound because sum_j p_j |v_j| / l >= |att|);
(b) end to end against the fp64 restatement, with bars computed from what the oracle itself loses over the sweep;
(c) for bits: batch composition, micro-batches, forward_frames, repeated calls, and the f32 handle of the new entry point;
(d) for refusals."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import vitpose_bf16_cases as cases
from helpers import vitpose_bf16_torch as oracle
from helpers import vitpose_edge_cases as edges
from upliftingtabletennis_amd import _lib, synth, vitpose, wasb, weights

pytestmark = pytest.mark.gpu

SRC_HW = (72, 96)


def _net(case, dtype='bf16', max_batch=None, micro_batch=0):
    h, w, cin, cout, b, _ = case
    return vitpose.ViTPoseNet(edges.state_dict(case), in_ch=cin, out_ch=cout, resolution=(w, h), max_batch=max_batch or b, micro_batch=micro_batch,
                              dtype=dtype)


def _forward(net, x):
    out = net.forward(x, want_heatmap=True, want_peaks=True)
    torch.cuda.synchronize()
    return out


def _same(got, want):
    for g, r in zip(got, want):
        assert g.shape == r.shape and g.dtype == r.dtype and torch.equal(g, r)


# ------------------------------------------------------------------------------------------ (a) teacher-forced, step by step
class _Checker:
    def __init__(self):
        self.lines, self.bad = [], []

    def check(self, stage, tap, got, want, got32, gemm_fed=False):
        """got: the device tap; want / got32: the oracle's step in fp64 / fp32 arithmetic from the same inputs."""
        bf16 = tap in oracle.BF16_TAPS
        if bf16:
            assert got.dtype == torch.bfloat16, (tap, got.dtype)
        big, share = cases.measures(got.cpu(), want, bf16)
        big_ok, share_ok = cases.allowance(got32, want, bf16, gemm_fed)
        self.lines.append('stage %2d %-6s max %.3g %s (allowed %.3g)%s' % (stage, tap, big, 'ulp' if bf16 else 'of scale', big_ok,
                                                                         '' if share is None else '  share %.3g (allowed %.3g)' % (share, share_ok)))
        if big > big_ok or (share is not None and share > share_ok):
            self.bad.append(self.lines[-1])


@functools.lru_cache(maxsize=None)
def _teacher_forced(case):
    h, w, cin, cout, b, _ = case
    hp, wp = h // 16, w // 16
    t = cases.taps(case)
    o64, o32 = t.o64, t.o32
    net = _net(case)
    c = _Checker()
    f64 = lambda a: a.cpu().double()          # noqa: E731
    with torch.no_grad():
        x = torch.from_numpy(edges.inputs(case))
        net.run_stage(0, x.cuda())
        c.check(0, 'x', net.read_tap('x'), t.stages[0]['x'], o32.patch(x))
        for s in range(1, oracle.DEPTH + 1):
            i, y = s - 1, t.stage_input(s)
            net.run_stage(s, y.cuda())
            got = {k: net.read_tap(k) for k in oracle.BLOCK_TAPS}
            c.check(s, 'qkv', got['qkv'], o64.qkv(i, y.double()), o32.qkv(i, y), gemm_fed=True)
            # att from the device's qkv, against the oracle's UNROUNDED output: 2^-9 sum p |v| / l, 2^-9 |att|, and the fp32 term (3 x
            # what fp32 arithmetic moves that output, at least the fp32 floor)
            dq = f64(got['qkv'])
            want, raw, pabs = o64.att(dq, b)
            _, raw32, _ = o32.att(dq.float(), b)
            term32 = max(3 * float((raw32.double() - raw).abs().max()), cases.F32_FLOOR * float(raw.abs().max()))
            over = float(((f64(got['att']) - raw).abs() / (2.0 ** -9 * pabs + 2.0 ** -9 * raw.abs() + term32)).max())
            c.lines.append('stage %2d att    max %.3g of its bound; %.3g ulp against the oracle' % (s, over, cases.measures(got['att'].cpu(), want, True)[0]))
            if over > 1:
                c.bad.append(c.lines[-1])
            da = f64(got['att'])
            c.check(s, 'x_attn', got['x_attn'], o64.proj(i, da, y.double()), o32.proj(i, da.float(), y))
            dxa = f64(got['x_attn'])
            c.check(s, 'hid', got['hid'], o64.fc1(i, dxa), o32.fc1(i, dxa.float()), gemm_fed=True)
            dh = f64(got['hid'])
            c.check(s, 'x', got['x'], o64.fc2(i, dh, dxa), o32.fc2(i, dh.float(), dxa.float()))
        y = t.stage_input(oracle.DEPTH + 1)
        net.run_stage(oracle.DEPTH + 1, y.cuda())
        got = {k: net.read_tap(k) for k in oracle.HEAD_TAPS}
        c.check(13, 'ln', got['ln'], o64.ln(y.double()), o32.ln(y), gemm_fed=True)
        dl = f64(got['ln'])
        c.check(13, 'd1', got['d1'], o64.deconv(0, dl, b, hp, wp), o32.deconv(0, dl.float(), b, hp, wp), gemm_fed=True)
        d1 = f64(got['d1'])
        c.check(13, 'd2', got['d2'], o64.deconv(1, d1, b, hp, wp), o32.deconv(1, d1.float(), b, hp, wp), gemm_fed=True)
        d2 = f64(got['d2']).reshape(b, 4 * hp, 4 * wp, 256)
        assert got['heat'].shape == (b, cout, h // 4, w // 4)
        c.check(13, 'heat', got['heat'], o64.final(d2), o32.final(d2.float()))
    return c


@pytest.mark.parametrize('case', cases.CASES, ids=edges.case_id)
def test_every_stage_teacher_forced(case):
    """Every tap within its measured allowance; qkv, hid, ln, d1 and d2 within one bf16 ulp of the oracle; att within
    2^-9 sum_j p_j |v_j| / l + 2^-9 |att| + the fp32 term."""
    c = _teacher_forced(case)
    print('\n%s\n%s' % (edges.case_id(case), '\n'.join(c.lines)))
    assert not c.bad, '\n'.join(c.bad)


# ------------------------------------------------------------------------------------------ (b) end to end
@pytest.mark.parametrize('case', cases.CASES, ids=edges.case_id)
def test_end_to_end_against_fp64(case):
    h, w, cin, cout, b, _ = case
    ref = edges.reference(case)
    heat, idx, win = (a.cpu().numpy() for a in _forward(_net(case), torch.from_numpy(edges.inputs(case)).cuda()))
    assert heat.shape == (b, cout, h // 4, w // 4) and heat.dtype == np.float32 and np.isfinite(heat).all()
    err, bar = ref.error(heat), cases.heat_bar()
    print('\n%s: max |heat - fp64| = %.3g of the range; the oracle %.3g; bar %.3g' % (edges.case_id(case), err, cases.heat_error(case), bar))
    assert err <= bar
    n = b * cout
    maps = heat.reshape(n, h // 4, w // 4)
    assert np.array_equal(idx, maps.reshape(n, -1).argmax(1))
    ok = ref.decided(bar)
    assert ok.mean() >= 0.9
    assert np.array_equal(idx[ok], ref.argmax[ok])
    got, want = cases.positions(maps), cases.positions(ref.heat64.reshape(n, h // 4, w // 4))
    shift = float(np.abs(got[ok, :2] - want[ok, :2]).max())
    print('refined positions: worst shift %.3g heatmap px, bar %.3g' % (shift, cases.position_bar()))
    assert shift <= cases.position_bar()
    assert np.array_equal(got[:, 2], want[:, 2])


# ------------------------------------------------------------------------------------------ (c) bits
@pytest.mark.parametrize('case', [edges.find(16, 16), edges.find(80, 208), edges.find(48, 688)], ids=edges.case_id)
def test_batch_tails_and_micro_batches_are_bit_neutral(case):
    """No output row's reduction order depends on M: batch 5 at micro-batch 1, 2, 3 and 5, its samples one by one, and a second
    call all give the same bits."""
    x = torch.from_numpy(edges.inputs(case, 5)).cuda()
    whole = _net(case, max_batch=5, micro_batch=5)
    first = _forward(whole, x)
    _same(_forward(whole, x), first)
    _same([torch.cat(t) for t in zip(*[_forward(whole, x[i:i + 1]) for i in range(5)])], first)
    for micro in (1, 2, 3):
        net = _net(case, max_batch=5, micro_batch=micro)
        assert net.micro_batch == micro and net.dtype == 'bf16'
        _same(_forward(net, x), first)
        _same(_forward(net, x), first)


@pytest.mark.parametrize('case', [edges.find(48, 16), edges.find(80, 208), edges.find(48, 80, in_ch=6)], ids=edges.case_id)
def test_forward_frames_equals_forward(case):
    h, w, cin, cout, _, _ = case
    nf, samples = cin // 3, 5
    net = _net(case, max_batch=samples, micro_batch=2)
    fr = torch.from_numpy(synth.synth_frames(samples + nf - 1, SRC_HW[0], SRC_HW[1], seed=h + w)[0]).cuda()
    pf = wasb.preprocess_frames(fr, (w, h))
    x = torch.cat([pf[f:f + samples] for f in range(nf)], 1)
    if cin == 9:
        assert torch.equal(x, wasb.preprocess_triples(fr, (w, h)))
    want = _forward(net, x)
    got = net.forward_frames(fr, want_heatmap=True)
    torch.cuda.synchronize()
    _same(got, want)


def test_f32_handle_of_the_new_entry_point_is_the_old_one():
    """ttup_vitpose_create_dtype(..., 0, ...) -- what ViTPoseNet calls for 'f32' -- gives the bits of ttup_vitpose_create's handle."""
    case = edges.find(80, 208)
    h, w, cin, cout, b, _ = case
    x = torch.from_numpy(edges.inputs(case)).cuda()
    new = _net(case, dtype='f32')
    got = _forward(new, x)
    lib = _lib.load()
    blob = weights.pack_vitpose_blob(edges.state_dict(case), in_ch=cin, out_ch=cout)
    old = ctypes.c_void_p()
    assert lib.ttup_vitpose_create(blob, len(blob), h, w, b, 0, cin, cout, ctypes.byref(old)) == _lib.OK
    lib.ttup_vitpose_destroy(new._handle)
    new._handle = old               # the same Python object now drives the old entry point's handle (and destroys it)
    _same(_forward(new, x), got)
    bf = _forward(_net(case), x)
    assert not torch.equal(bf[0], got[0])          # and the bf16 handle is another path


# ------------------------------------------------------------------------------------------ (d) refusals
def test_refusals():
    case = edges.find(16, 48)
    h, w, cin, cout, b, _ = case
    with pytest.raises(ValueError):
        _net(case, dtype='fp16')
    lib = _lib.load()
    blob = weights.pack_vitpose_blob(edges.state_dict(case), in_ch=cin, out_ch=cout)
    handle = ctypes.c_void_p()
    assert lib.ttup_vitpose_create_dtype(blob, len(blob), h, w, b, 0, cin, cout, 2, ctypes.byref(handle)) == _lib.EINVAL and not handle
    net = _net(case, max_batch=4, micro_batch=2)
    y = torch.zeros((3 * edges.tokens(case), 384), device='cuda')
    with pytest.raises(ValueError):
        net.read_tap('x')                          # no stage has run
    for stage in (-1, 14):
        with pytest.raises(ValueError, match='stage'):
            net.run_stage(stage, y[:edges.tokens(case)])
    with pytest.raises(ValueError, match='batch'):
        net.run_stage(1, y)                        # batch 3 above the micro-batch 2
    net.run_stage(1, y[:2 * edges.tokens(case)])
    assert net.read_tap('qkv').shape == (2 * edges.tokens(case), 1152)
    with pytest.raises(ValueError):
        net.read_tap('scores')                     # no such tap
    with pytest.raises(ValueError, match='does not write'):
        net.read_tap('heat')                       # a tap of the head, after a block
    net.forward(torch.zeros((1, cin, h, w), device='cuda'))
    with pytest.raises(ValueError):
        net.read_tap('qkv')                        # a forward since the stage
