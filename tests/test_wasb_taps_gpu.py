"""The bf16 CNN tap by tap, teacher-forced, against the bf16-rounding oracle (oracle/wasb_bf16_ref.py) at the tile, border, channel
and persistent-trip edges of its fused kernels (cases and tile arithmetic: tests/helpers/wasb_edge_cases.py).

Per case the net runs ONCE (batch <= micro-batch, so the taps hold the whole batch).  Every segment of the oracle then starts from
the DEVICE's input taps -- exact bf16 values -- and its output taps are compared with the device's: a kernel's rounding never
leaks into the next segment, so a difference is a few rounding flips inside at most six layers.  How many flips are legitimate is
measured, not fixed: the oracle's fp32 variant (reversed K order) against its float64 evaluation on the same inputs gives the
spread, and the device may reach 3 x its max (floor 2^-8), 2 x its mean and 2 x its share of differing elements (floor: 16
elements per image; a margin of 4 on the taps the case table lists, with the reason beside each), and never more than 2^-6 of a
tap's scale.  Every tap the plan stores is compared (the record cases `32x56_pre_*`: those of S0, the segment that reads the
pre-processing kernels' records -- E.segments); taps it does not store must be unknown to the handle."""
import pytest
import torch

from conftest import has_gpu
from helpers import wasb_edge_cases as E

pytestmark = pytest.mark.gpu
if has_gpu():
    from upliftingtabletennis_amd import wasb


@pytest.fixture(autouse=True)
def _synthetic_weights(monkeypatch):
    monkeypatch.setenv('TTUP_SYNTHETIC_WEIGHTS', '1')
    monkeypatch.delenv('TTUP_WEIGHTS', raising=False)


def _device_run(case):
    """-> (taps {name: (batch,C,h,w) float32 on the host}, heat (batch,K,H,W), argmax (batch*K,))"""
    sd = E.state_dict(case)
    with E.knob_set(case):
        if case.kind == 'table':
            net = wasb.get_table_model('hrnet', resolution=(case.w, case.h), state_dict=sd, max_batch=case.batch, dtype='bf16')
        else:
            net = wasb.WASBNet(sd, resolution=(case.w, case.h), max_batch=case.batch, dtype='bf16')
    if case.kind in ('frames', 'table'):
        heat, idx, _ = wasb.WASBNet.forward_frames(net, torch.from_numpy(E.frames(case)).cuda(), want_heatmap=True)
    else:
        heat, idx, _ = wasb.WASBNet.forward(net, torch.from_numpy(E.inputs(case)), want_heatmap=True, want_peaks=True)
    taps = {name: net.read_tap(name, case.batch).cpu() for name in E.stored_taps(case)}
    for name in E.ALL_TAPS:
        if name not in taps:          # the case table states what the plan stores: nothing stored goes unchecked (the record cases compare S0's taps only: E.segments)
            with pytest.raises(ValueError):
                net.read_tap(name, case.batch)
    return taps, heat.cpu(), idx.cpu()


@pytest.mark.parametrize('case', E.CASES, ids=lambda c: c.id)
def test_taps_match_the_rounding_oracle_teacher_forced(case):
    taps, heat, idx = _device_run(case)
    assert all(torch.isfinite(t).all() for t in taps.values()) and torch.isfinite(heat).all()
    taps['heat'] = heat
    x = torch.from_numpy(E.inputs(case))
    failures, compared = [], set()
    for seg in E.segments(case):
        im = list(E.segment_images(case, seg))
        rows = E.compare_segment(case, seg, x[im], {k: v[im] for k, v in taps.items()}, {k: v[im] for k, v in taps.items()})
        for tap, sp, dev, bd, ref in rows:
            print(E.format_row(case, seg, tap, sp, dev, bd))
            if sp.max >= E.CAP_SPREAD:
                failures.append((seg, tap, 'spread', sp.max))
            if dev is None:
                continue
            compared.add(tap)
            for name, got, bound in zip(dev._fields, dev, bd):
                if not got <= bound:
                    failures.append((seg, tap, name, got, bound))
            if not dev.max <= E.CAP_MAX:
                failures.append((seg, tap, 'cap', dev.max))
            if tap == 'heat' and case.planted:          # planted weights: one dominant peak, the oracle's argmax exactly
                k = ref.shape[1]
                want = ref.reshape(len(im) * k, -1).argmax(1)
                got = idx.reshape(case.batch, k)[im].reshape(-1)
                if not torch.equal(got, want):
                    failures.append((seg, tap, 'argmax', got.tolist(), want.tolist()))
    assert compared == E.compared_taps(case), compared
    assert not failures, failures
