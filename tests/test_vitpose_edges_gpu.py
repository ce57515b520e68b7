"""csrc/vitpose.hip at its kernels' token, tile, channel and border edges (the sweep of tests/helpers/vitpose_edge_cases.py) against
the fp64 CPU restatement (tests/helpers/vitpose_torch.py, pinned to the reference at these shapes by test_vitpose_edges_host.py):
heatmaps, fused peaks, bit-neutral batch composition, `forward_frames` against `forward`, nothing written past the batch, and
refusals made on the host before any launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import vitpose_edge_cases as edges
from oracle import refine_ref
from test_vitpose_gpu import HEAT_BAR
from upliftingtabletennis_amd import _lib, synth, vitpose, wasb, weights

pytestmark = pytest.mark.gpu

# Every case meets the project's HEAT_BAR as it stands.  Measured on the MI355X: 0.81e-6 .. 3.03e-6 of the range (largest: 128x128, 3 -> 16,
# 64 tokens), 0.9 .. 3.3 times the case's e32 (the fp32 CPU restatement against fp64, 0.44e-6 .. 1.47e-6); no case has a bar of its own.
SENTINEL32, SENTINEL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
SRC_HW = (72, 96)            # uint8 frame size of the forward_frames tests: no network size of the sweep


def _net(case, max_batch=None, micro_batch=0):
    h, w, cin, cout, b, _ = case
    return vitpose.ViTPoseNet(edges.state_dict(case), in_ch=cin, out_ch=cout, resolution=(w, h), max_batch=max_batch or b, micro_batch=micro_batch)


def _forward(net, x):
    out = net.forward(x, want_heatmap=True, want_peaks=True)
    torch.cuda.synchronize()
    return out


def _same(got, want):
    for g, r in zip(got, want):
        assert g.shape == r.shape and g.dtype == r.dtype and torch.equal(g, r)


@functools.lru_cache(maxsize=None)
def _outcome(case):
    """(heat, idx, win) of the case on one handle of its own, as numpy arrays: computed once for the tests that read it."""
    out = _forward(_net(case), torch.from_numpy(edges.inputs(case)).cuda())
    out = tuple(t.cpu().numpy() for t in out)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize('case', edges.CASES, ids=edges.case_id)
def test_heatmaps_match_fp64_restatement(case):
    h, w, cin, cout, b, _ = case
    ref = edges.reference(case)
    heat, _, _ = _outcome(case)
    assert heat.shape == (b, cout, h // 4, w // 4) and heat.dtype == np.float32 and np.isfinite(heat).all()
    err = ref.error(heat)
    print('\n%s (%d tokens): max |heat - fp64| = %.3g of the range; fp32 CPU restatement %.3g; ratio %.2f'
          % (edges.case_id(case), edges.tokens(case), err, ref.e32, err / ref.e32))
    assert err <= HEAT_BAR


@pytest.mark.parametrize('case', edges.CASES, ids=edges.case_id)
def test_peaks(case):
    """The fused argmax is the argmax of the returned heatmap, the window its zero-padded 3x3 neighbourhood bit for bit (4x4 maps:
    mostly padding), and the argmax is the fp64 reference's wherever that one is decided by more than twice the bar."""
    h, w, _, cout, b, _ = case
    ref = edges.reference(case)
    heat, idx, win = _outcome(case)
    maps = heat.reshape(b * cout, h // 4, w // 4)
    assert idx.shape == (b * cout,) and idx.dtype == np.int64 and win.shape == (b * cout, 9) and win.dtype == np.float32
    assert np.array_equal(idx, torch.from_numpy(maps.copy()).reshape(b * cout, -1).argmax(1).numpy())
    want_idx, want_win = refine_ref.argmax_window(maps)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(win.view(np.uint32), want_win.reshape(b * cout, 9).view(np.uint32))
    ok = ref.decided(HEAT_BAR)
    assert ok.mean() >= 0.9
    assert np.array_equal(idx[ok], ref.argmax[ok])


@pytest.mark.parametrize('case', [edges.find(16, 16), edges.find(48, 16), edges.find(80, 208), edges.find(48, 688)], ids=edges.case_id)
def test_batch_composition_is_bit_neutral(case):
    """Every output row's reduction order in gemm_kernel, attention_kernel, the deconv phases and conv1x1_kernel depends on that
    row alone, never on M: sample i of a batch of 3 equals the one-sample call, whatever the micro-batch (1, 2, default 3), the
    Python chunking (max_batch 2) or the calls made before on the handle."""
    x = torch.from_numpy(edges.inputs(case, 3)).cuda()
    whole = _net(case, max_batch=3)
    assert whole.micro_batch == 3
    first = _forward(whole, x)
    ones = [_forward(whole, x[i:i + 1]) for i in range(3)]          # calls of batch 3, 1, 1, 1, 3 on one handle
    again = _forward(whole, x)
    _same(again, first)
    _same(first, [torch.cat(t) for t in zip(*ones)])
    for max_batch, micro in ((3, 1), (3, 2), (2, 0)):
        net = _net(case, max_batch=max_batch, micro_batch=micro)
        assert net.micro_batch == (micro or max_batch)
        _same(_forward(net, x), first)
        _same(_forward(net, x[2:3]), ones[2])


@pytest.mark.parametrize('case', [edges.find(16, 16), edges.find(48, 16), edges.find(80, 208), edges.find(48, 80, in_ch=6)], ids=edges.case_id)
def test_forward_frames_equals_forward(case):
    """uint8 frames of another size in, five samples on a handle of micro-batch 2 (consecutive micro-batches share frames): the
    outputs of `forward` on the pre-processed frames, bit for bit.  A 6-channel sample is frames t and t+1 (A_PATCH_FRAMES)."""
    h, w, cin, cout, _, _ = case
    nf, samples = cin // 3, 5
    net = _net(case, max_batch=samples, micro_batch=2)
    assert net.micro_batch == 2
    fr = torch.from_numpy(synth.synth_frames(samples + nf - 1, SRC_HW[0], SRC_HW[1], seed=h + w)[0]).cuda()
    assert fr.shape[1:3] != (h, w)
    pf = wasb.preprocess_frames(fr, (w, h))
    x = torch.cat([pf[f:f + samples] for f in range(nf)], 1)
    assert x.shape == (samples, cin, h, w)
    if cin == 9:
        assert torch.equal(x, wasb.preprocess_triples(fr, (w, h)))
    want = _forward(net, x)
    got = net.forward_frames(fr, want_heatmap=True)
    torch.cuda.synchronize()
    _same(got, want)
    _, idx, win = net.forward_frames(fr)
    torch.cuda.synchronize()
    assert torch.equal(idx, want[1]) and torch.equal(win, want[2])


@pytest.mark.parametrize('case', [edges.find(48, 80, in_ch=1), edges.find(48, 80, in_ch=4)], ids=edges.case_id)
def test_forward_frames_refused_without_whole_frames(case):
    net = _net(case)
    fr = torch.zeros((4,) + SRC_HW + (3,), dtype=torch.uint8, device='cuda')
    with pytest.raises(ValueError):
        net.forward_frames(fr)
    idx = torch.full((4 * case[3],), SENTINEL64, dtype=torch.int64, device='cuda')
    win = torch.full((4 * case[3], 9), SENTINEL32, dtype=torch.int32, device='cuda')
    rc = _lib.load().ttup_vitpose_forward_frames(net._handle, _lib.ptr(fr), 2, SRC_HW[0], SRC_HW[1], None, _lib.ptr(idx), _lib.ptr(win), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.EINVAL and bool((idx == SENTINEL64).all()) and bool((win == SENTINEL32).all())


def _sentinel_outputs(case, rows):
    h, w, _, cout, _, _ = case
    heat = torch.full((rows, cout, h // 4, w // 4), SENTINEL32, dtype=torch.int32, device='cuda')
    idx = torch.full((rows * cout,), SENTINEL64, dtype=torch.int64, device='cuda')
    win = torch.full((rows * cout, 9), SENTINEL32, dtype=torch.int32, device='cuda')
    return heat, idx, win


def _untouched(heat, idx, win, row0, cout):
    return bool((heat[row0:] == SENTINEL32).all()) and bool((idx[row0 * cout:] == SENTINEL64).all()) and bool((win[row0 * cout:] == SENTINEL32).all())


@pytest.mark.parametrize('case', [edges.find(16, 16), edges.find(80, 208)], ids=edges.case_id)
def test_nothing_written_past_the_batch(case):
    """ttup_vitpose_forward with batch 3 on a handle of max_batch 4 (micro-batches of 2 and 1): outputs sized for max_batch keep
    their fill at row 3, and rows 0..2 are what `forward` gives."""
    cout = case[3]
    net = _net(case, max_batch=4, micro_batch=2)
    x = torch.from_numpy(edges.inputs(case, 3)).cuda()
    heat, idx, win = _sentinel_outputs(case, 4)
    rc = net._lib.ttup_vitpose_forward(net._handle, _lib.ptr(x), 3, _lib.ptr(heat), _lib.ptr(idx), _lib.ptr(win), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.OK
    assert _untouched(heat, idx, win, 3, cout)
    want = _forward(net, x)
    _same((heat[:3].view(torch.float32), idx[:3 * cout], win[:3 * cout].view(torch.float32)), want)


def test_refusals_on_the_host():
    """Bad sizes and channel counts at create, and batch > max_batch or a misaligned input at forward, are TTUP_EINVAL from the
    requirement checks that precede every launch: no handle is made, and the outputs keep their fill."""
    case = edges.find(16, 16)
    h, w, cin, cout, _, _ = case
    lib = _lib.load()
    blob = weights.pack_vitpose_blob(edges.state_dict(case), in_ch=cin, out_ch=cout)

    def create(height=h, width=w, in_ch=cin, out_ch=cout):
        handle = ctypes.c_void_p()
        rc = lib.ttup_vitpose_create(blob, len(blob), height, width, 2, 0, in_ch, out_ch, ctypes.byref(handle))
        if handle:
            lib.ttup_vitpose_destroy(handle)
        return rc, bool(handle)
    assert create() == (_lib.OK, True)
    for bad in (dict(height=8), dict(width=8), dict(height=8, width=8), dict(out_ch=0), dict(out_ch=17), dict(in_ch=0)):
        assert create(**bad) == (_lib.EINVAL, False), bad
    with pytest.raises(ValueError):
        vitpose.ViTPoseNet(edges.state_dict(case), in_ch=cin, out_ch=cout, resolution=(16, 8))
    with pytest.raises(ValueError):
        vitpose.ViTPoseNet(edges.state_dict(case), in_ch=cin, out_ch=cout, resolution=(8, 16))

    net = _net(case, max_batch=2)
    heat, idx, win = _sentinel_outputs(case, 4)
    buf = torch.zeros(3 * cin * h * w + 1, dtype=torch.float32, device='cuda')

    def forward(x, batch):
        rc = lib.ttup_vitpose_forward(net._handle, _lib.ptr(x), batch, _lib.ptr(heat), _lib.ptr(idx), _lib.ptr(win), _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc
    assert forward(buf, 3) == _lib.EINVAL                   # batch > max_batch
    assert b'batch' in lib.ttup_last_error()
    assert buf[1:].data_ptr() == buf.data_ptr() + 4
    assert forward(buf[1:], 2) == _lib.EINVAL               # input offset by one float
    assert b'aligned' in lib.ttup_last_error()
    assert _untouched(heat, idx, win, 0, cout)
    assert forward(buf, 2) == _lib.OK and not _untouched(heat, idx, win, 0, cout) and _untouched(heat, idx, win, 2, cout)
