"""Every lane of a CNN handle owns its activation buffers (csrc/wasb_net.hip allocates them in one loop over lanes and tensors):
three micro-batches, the last one ragged, on handles with one, two and three lanes, at the smallest network input that reaches
every lane.  Heatmaps, argmax and windows are bit-identical across lane counts and equal a one-sample handle fed sample by sample
(the same kernels run per sample whatever the micro-batch; no tolerance is involved)."""
import pytest
import torch

from upliftingtabletennis_amd import synth, wasb, weights

pytestmark = pytest.mark.gpu

RES = (96, 64)          # (W, H)
BATCH = 5               # micro-batches of 2, 2 and 1

CASES = {
    'ball-bf16': (wasb.WASBNet, dict(in_ch=9, head_out=3), 'bf16'),          # frames tensor with two extra frames per lane
    'table-bf16': (wasb.MyHRNet, dict(in_ch=3, head_out=13, plant_all_heads=True), 'bf16'),          # one frame per sample, 13 channels
    'ball-f32': (wasb.WASBNet, dict(in_ch=9, head_out=3), 'f32'),          # 4-byte activations, layer by layer
}


def _peaks(net, x):
    return net.forward(x, want_peaks=True) if isinstance(net, wasb.MyHRNet) else net.forward(x, want_heatmap=True, want_peaks=True)


@pytest.mark.parametrize('case', sorted(CASES))
def test_lane_counts_and_one_sample_handles_agree_bit_for_bit(case, monkeypatch):
    cls, wkw, dtype = CASES[case]
    sd = weights.random_wasb_state_dict(7, planted=True, **wkw)
    nf = wkw['in_ch'] // 3
    frames = torch.from_numpy(synth.synth_frames(BATCH + nf - 1, 72, 128, seed=3)[0]).cuda()
    x = wasb.preprocess_triples(frames, RES) if nf == 3 else wasb.preprocess_frames(frames, RES)
    assert x.shape[0] == BATCH
    monkeypatch.setenv('TTUP_MICRO_BATCH', '2')          # sampled by every handle when it is created
    nets = {n: cls(sd, resolution=RES, max_batch=BATCH, dtype=dtype, lanes=n) for n in (1, 2, 3)}
    one = cls(sd, resolution=RES, max_batch=1, dtype=dtype)
    monkeypatch.delenv('TTUP_MICRO_BATCH')
    assert [len(nets[n].internal_streams()) for n in (1, 2, 3)] == [0, 2, 3] and len(one.internal_streams()) == 0
    for name, full, single in (('forward_frames', lambda net: net.forward_frames(frames, want_heatmap=True),
                                lambda i: one.forward_frames(frames[i:i + nf], want_heatmap=True)),
                               ('forward', lambda net: _peaks(net, x), lambda i: _peaks(one, x[i:i + 1]))):
        ref = [torch.cat(parts) for parts in zip(*[single(i) for i in range(BATCH)])]
        assert ref[0].shape == (BATCH, cls.OUT_CH, RES[1], RES[0]) and ref[1].shape == (BATCH * cls.OUT_CH,) and ref[2].shape == (BATCH * cls.OUT_CH, 9)
        for n in (1, 2, 3):
            for _ in range(2):          # the second call reuses every lane's buffers
                got = full(nets[n])
                for what, g, r in zip(('heat', 'argmax', 'windows'), got, ref):
                    assert torch.equal(g, r), (case, name, 'lanes=%d' % n, what)
