"""ViTPose-small on the GPU (csrc/vitpose.hip through the C-ABI) against the reference's own fp32 forward
(tests/golden/vitpose.npz, tools/make_goldens_vitpose.py), and the 'vitpose' detectors of the drop-in interface."""
import numpy as np
import pytest
import torch

from upliftingtabletennis_amd import _lib, refine, synth, vitpose, weights

pytestmark = pytest.mark.gpu

# max |heatmap - reference| / heatmap range: twice the largest value measured on the MI355X over the golden cases (2.65e-6, the
# 13-map table case; 0.7e-6 .. 2.0e-6 on the ball cases).  The reference's own fp32 CPU forward differs from an fp64 one by ~8e-7
# of the range at 640x1152; bf16 arithmetic would give ~1e-2.
HEAT_BAR = 5.3e-6
CASES = ['ball_160x288', 'ball_96x176', 'table_96x176', 'ball_640x1152']


def _net_and_input(g, name, micro_batch=0):
    ws, xs, b, cin, cout, h, w, full = [int(v) for v in g[name + '/meta']]
    sd = weights.random_vitpose_state_dict(ws, in_ch=cin, out_ch=cout, resolution=(w, h))
    x, _ = synth.vitpose_inputs(xs, b, cin, h, w)
    net = vitpose.ViTPoseNet(sd, in_ch=cin, out_ch=cout, resolution=(w, h), max_batch=b, micro_batch=micro_batch)
    return net, torch.from_numpy(x).cuda(), (b, cin, cout, h, w, full)


def _run(g, name, micro_batch=0, batch=None):
    net, x, meta = _net_and_input(g, name, micro_batch)
    heat, idx, win = net.forward(x[:batch], want_heatmap=True, want_peaks=True)
    torch.cuda.synchronize()
    return heat, idx, win, meta


def _heat_err(g, name, heat, full):
    ws, xs, b, cin, cout, h, w, _ = [int(v) for v in g[name + '/meta']]
    rng = g[name + '/range'].astype(np.float64)
    hm = heat.cpu().numpy().reshape(b * cout, h // 4, w // 4)
    if full:
        ref = g[name + '/heat'].reshape(b * cout, h // 4, w // 4)
        return max(float(np.abs(hm[k] - ref[k]).max() / rng[k]) for k in range(b * cout))
    errs = []
    for k, (y0, x0) in enumerate(g[name + '/crop_origin']):
        c = hm[k, y0:y0 + 32, x0:x0 + 32]
        errs.append(float(np.abs(c - g[name + '/crop'][k]).max() / rng[k]))
    st = g[name + '/stats']
    assert np.abs(hm.reshape(b * cout, -1).mean(1) - st[:, 0]).max() <= HEAT_BAR * rng.max()
    return max(errs)


@pytest.mark.parametrize('name', CASES)
def test_heatmaps_argmax_refine_match_reference(golden, name):
    g = golden('vitpose.npz')
    heat, idx, win, (b, cin, cout, h, w, full) = _run(g, name)
    err = _heat_err(g, name, heat, full)
    print('\n%s: max |heat - ref| = %.3g of the range' % (name, err))
    assert err <= HEAT_BAR
    # argmax: equal wherever the reference's top-2 margin exceeds twice the bar, and that must be almost every map
    ok = g[name + '/margin'] > 2 * HEAT_BAR * g[name + '/range']
    assert ok.mean() >= 0.9
    assert np.array_equal(idx.cpu().numpy()[ok], g[name + '/argmax'][ok])
    # the fused argmax equals the argmax of the returned heatmaps
    assert np.array_equal(idx.cpu().numpy(), heat.reshape(b * cout, -1).argmax(1).cpu().numpy())
    xyv = refine.refine_windows_device(idx, win, h // 4, w // 4, 1920, 1080, _lib.REFINE_TABLE).cpu().numpy()
    assert np.abs(xyv[ok] - g[name + '/xyv'][ok]).max() <= 1e-3


@pytest.mark.parametrize('micro,batch', [(2, 3), (2, 1), (1, 3)])
def test_batch_tails(golden, micro, batch):
    """batch 1, an odd batch, and batches larger than the handle's micro-batch give the full batch's per-sample results: the
    reference's within the bar, and the one-sample call's bit for bit (no output row's reduction order depends on the batch)."""
    g = golden('vitpose.npz')
    name = 'ball_96x176'
    net, x, (b, cin, cout, h, w, _) = _net_and_input(g, name, micro_batch=micro)
    heat, idx, win = net.forward(x[:batch], want_heatmap=True, want_peaks=True)
    torch.cuda.synchronize()
    ref = g[name + '/heat'][:batch]
    assert heat.shape == ref.shape
    assert np.abs(heat.cpu().numpy() - ref).max() <= HEAT_BAR * (ref.max() - ref.min())
    assert np.array_equal(idx.cpu().numpy(), g[name + '/argmax'][:batch * cout])
    for i in range(batch):
        h1, i1, w1 = net.forward(x[i:i + 1], want_heatmap=True, want_peaks=True)
        assert torch.equal(h1, heat[i:i + 1]) and torch.equal(i1, idx[i * cout:(i + 1) * cout]) and torch.equal(w1, win[i * cout:(i + 1) * cout])


def test_rejects_bad_sizes():
    sd = weights.random_vitpose_state_dict(1, resolution=(176, 96))
    with pytest.raises(ValueError):
        vitpose.ViTPoseNet(sd, resolution=(176, 100))                 # not a multiple of 16
    with pytest.raises(ValueError):
        vitpose.ViTPoseNet(sd, resolution=(192, 96))                  # pos_embed rows do not match the size
    net = vitpose.ViTPoseNet(sd, resolution=(176, 96), max_batch=2)
    with pytest.raises(ValueError):
        net.forward(torch.zeros(1, 3, 96, 176, device='cuda'))


def _track_error(pos, track):
    exp = (track + 0.5) * 1.5 - 0.5                 # 1280x720 frames -> 1920x1080 coordinates
    return np.hypot(*(pos[:, :2] - exp).T)


def test_ball_detector_vitpose(monkeypatch):
    monkeypatch.setenv('TTUP_SYNTHETIC_WEIGHTS', '1')
    from upliftingtabletennis_amd.interface import BallDetector
    det = BallDetector('vitpose', max_batch=4)
    assert isinstance(det, BallDetector) and det.model_resolution == (1152, 640)
    frames, track = synth.synth_frames(8, 720, 1280, seed=2)
    triples = [[frames[i - 1], frames[i], frames[i + 1]] for i in range(1, 7)]
    pos, heat = det.predict(triples)
    assert pos.shape == (6, 3) and pos.dtype == np.float64 and heat.shape == (6, 1, 160, 288) and heat.dtype == np.float32
    assert (pos[:, 2] == 1).all()
    clip = det.predict_clip(list(frames))
    assert clip.shape == (6, 3) and np.array_equal(clip, pos)
    # planted weights: the detections follow the synthetic blob to within about a patch (16 model px = 27 px at 1920x1080)
    err = _track_error(pos, track[1:7])
    print('\nvitpose ball detections: distance to the blob %s px' % np.round(err, 1))
    assert (err < 30).all()
    # the agreement filter across the two detector families
    wasb_pos, _ = BallDetector('wasb', max_batch=4).predict(triples)
    filt, idx, times = det.filter_trajectory(wasb_pos, pos, 60.0)
    assert filt.shape[1] == 2 and len(times) == filt.shape[0]
    with pytest.raises(NotImplementedError):
        BallDetector('segformerpp_b2')


def test_table_detector_vitpose(monkeypatch):
    monkeypatch.setenv('TTUP_SYNTHETIC_WEIGHTS', '1')
    from upliftingtabletennis_amd.interface import TableDetector
    det = TableDetector('vitpose', max_batch=2)
    frames, _ = synth.synth_frames(3, 720, 1280, seed=4)
    pos, heat = det.predict(list(frames))
    assert pos.shape == (3, 13, 3) and pos.dtype == np.float64 and heat.shape == (3, 1, 13, 160, 288) and heat.dtype == np.float32
    kp = det.predict_keypoints(list(frames))
    assert kp.shape == (3, 13, 3) and np.array_equal(kp, pos)
    with pytest.raises(NotImplementedError):
        TableDetector('segformerpp_b2')
