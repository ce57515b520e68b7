"""The two-detector hub pipeline: ViTPose-small as the aux detector of both agreement filters, fed from the clip's single upload.

* `ViTPoseNet.forward_frames` (uint8 frames in, each pre-processed once) against `forward` on the pre-processed triples / frames,
  bit for bit, and its argument checks;
* `TableTennisPipeline(ball_aux='vitpose', table_aux='vitpose')`: the overlapped clip path against the detectors' own clip calls
  and the reference's filters (oracle/glue_ref.py) composed on them, and against the serial path;
* the default `TableTennisPipeline()`: the same two comparisons at clip lengths around the chunk boundaries;
* the constructor surface (`TableTennisPipeline(ball_aux=, table_aux=)`, `hubconf.full_pipeline_two_detectors`)."""
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import glue_ref
from upliftingtabletennis_amd import _lib, glue, synth, vitpose, wasb, weights

pytestmark = pytest.mark.gpu

RES = weights.VITPOSE_RESOLUTION            # (W, H) = (1152, 640)
MAX_BATCH = 12                              # micro-batch 8 (the handle's default for max_batch >= 8)


@pytest.fixture(scope='module')
def nets():
    sd_ball = weights.random_vitpose_state_dict(11, in_ch=9, out_ch=1, resolution=RES)
    sd_table = weights.random_vitpose_state_dict(12, in_ch=3, out_ch=13, resolution=RES)
    return {9: vitpose.ViTPoseNet(sd_ball, in_ch=9, out_ch=1, resolution=RES, max_batch=MAX_BATCH),
            3: vitpose.ViTPoseNet(sd_table, in_ch=3, out_ch=13, resolution=RES, max_batch=MAX_BATCH)}


@pytest.fixture(scope='module')
def clips():
    return {hw: torch.from_numpy(synth.synth_frames(MAX_BATCH + 6, hw[0], hw[1], seed=hw[0])[0]).cuda() for hw in ((720, 1280), (1080, 1920))}


def _reference(net, fr):
    x = wasb.preprocess_triples(fr, RES) if net.IN_CH == 9 else wasb.preprocess_frames(fr, RES)
    return net.forward(x, want_heatmap=True, want_peaks=True)


def _assert_identical(got, ref):
    for g, r in zip(got, ref):
        assert g.shape == r.shape and torch.equal(g, r)


@pytest.mark.parametrize('hw', [(720, 1280), (1080, 1920)])
@pytest.mark.parametrize('in_ch', [9, 3])
@pytest.mark.parametrize('samples', [1, 8, 9, MAX_BATCH])
def test_forward_frames_is_bit_identical_to_forward(nets, clips, hw, in_ch, samples):
    net = nets[in_ch]
    assert net.micro_batch == 8
    fr = clips[hw][:samples + in_ch // 3 - 1]
    got = net.forward_frames(fr, want_heatmap=True)
    ref = _reference(net, fr)
    torch.cuda.synchronize()
    assert got[1].shape == (samples * net.OUT_CH,)
    _assert_identical(got, ref)
    # without the heatmap: the same peaks
    _, idx, win = net.forward_frames(fr)
    assert torch.equal(idx, ref[1]) and torch.equal(win, ref[2])


@pytest.mark.parametrize('in_ch', [9, 3])
def test_forward_frames_on_a_slice_and_past_max_batch(nets, clips, in_ch):
    """A non-zero-offset slice frames[c0:c1] (what the hub passes), and more samples than max_batch (split into calls)."""
    net, fr = nets[in_ch], clips[(720, 1280)]
    sl = fr[3:3 + 5 + in_ch // 3 - 1]
    _assert_identical(net.forward_frames(sl, want_heatmap=True), _reference(net, sl.clone()))
    # MAX_BATCH + 6 frames: more samples than one call takes
    heat, idx, win = net.forward_frames(fr, want_heatmap=True)
    nf = in_ch // 3
    s = fr.shape[0] - nf + 1
    assert s > MAX_BATCH and heat.shape[0] == s
    first, rest = _reference(net, fr[:MAX_BATCH + nf - 1]), _reference(net, fr[MAX_BATCH:])
    _assert_identical((heat, idx, win), [torch.cat([a, b]) for a, b in zip(first, rest)])


def test_forward_frames_rejections(nets, clips):
    ball, table = nets[9], nets[3]
    fr = clips[(720, 1280)]
    with pytest.raises(ValueError):
        ball.forward_frames(fr.float())                          # not uint8
    with pytest.raises(ValueError):
        ball.forward_frames(fr[..., :2])                         # not BGR
    with pytest.raises(ValueError):
        ball.forward_frames(fr[0])                               # not (N, h, w, 3)
    with pytest.raises(ValueError):
        ball.forward_frames(fr[:2])                              # fewer than 3 frames on the ball handle
    # the C-ABI itself: TTUP_EINVAL with a message, nothing launched
    lib = _lib.load()
    idx = torch.empty((64 * 13,), dtype=torch.int64, device='cuda')
    win = torch.empty((64 * 13, 9), dtype=torch.float32, device='cuda')
    h, w = fr.shape[1], fr.shape[2]

    def call(net, frames, n, sh=h, sw=w, i=idx, wn=win):
        return lib.ttup_vitpose_forward_frames(net._handle, _lib.ptr(frames), n, sh, sw, None, _lib.ptr(i), _lib.ptr(wn), _lib.stream_ptr())
    assert call(ball, fr, MAX_BATCH + 3) == _lib.EINVAL          # MAX_BATCH + 1 triples
    assert b'samples' in lib.ttup_last_error()
    assert call(table, fr, MAX_BATCH + 1) == _lib.EINVAL
    assert call(ball, fr, 2) == _lib.EINVAL
    assert call(table, fr, 0) == _lib.EINVAL
    assert call(ball, fr, 3, sh=0) == _lib.EINVAL
    assert call(ball, fr, 3, sw=-4) == _lib.EINVAL
    assert call(ball, None, 3) == _lib.EINVAL
    assert call(ball, fr, 3, i=None) == _lib.EINVAL              # argmax and window go together
    assert lib.ttup_vitpose_forward_frames(None, _lib.ptr(fr), 3, h, w, None, None, None, _lib.stream_ptr()) == _lib.EINVAL
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the two-detector pipeline

def _synthetic_pipeline(**kw):
    old = os.environ.get('TTUP_SYNTHETIC_WEIGHTS')
    os.environ['TTUP_SYNTHETIC_WEIGHTS'] = '1'
    try:
        from upliftingtabletennis_amd.interface import TableTennisPipeline
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            yield TableTennisPipeline(**kw)
    finally:
        if old is None:
            os.environ.pop('TTUP_SYNTHETIC_WEIGHTS', None)
        else:
            os.environ['TTUP_SYNTHETIC_WEIGHTS'] = old


@pytest.fixture(scope='module')
def pipe():
    yield from _synthetic_pipeline(ball_aux='vitpose', table_aux='vitpose')


@pytest.fixture(scope='module')
def default_pipe():
    yield from _synthetic_pipeline()


def _predict_or_error(f):
    try:
        spin, pos = f()
        return spin.detach().cpu().numpy().copy(), np.asarray(pos).copy()
    except ValueError as e:         # the reference's mask check: 50 or more kept detections in one clip
        return ('ValueError', str(e))


def _same_result(a, b):
    if isinstance(a[0], str) or isinstance(b[0], str):
        return a == b
    return a[1].shape == b[1].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('n_frames', [48, 'long'])
def test_two_detector_pipeline_matches_its_composition(pipe, n_frames, monkeypatch):
    from upliftingtabletennis_amd.interface import ViTPoseBallDetector, ViTPoseTableDetector
    assert isinstance(pipe.ball_detector_aux, ViTPoseBallDetector) and isinstance(pipe.table_detector_aux, ViTPoseTableDetector)
    n = 4 * pipe.CHUNK + 1 if n_frames == 'long' else n_frames          # the long-chunk regime with a partial last chunk
    fps = 60.0
    monkeypatch.delenv('TTUP_HUB_SERIAL', raising=False)
    # the first seeded clip on which the ball filter both keeps and rejects frames (planted ViTPose follows the blob to about
    # 27 px, the filter's bar is 20 px): found and asserted here, not assumed
    for seed in range(7, 15):
        images = [f for f in synth.synth_frames(n, 720, 1280, seed=seed)[0]]
        wasb_pos = pipe.ball_detector.predict_clip(images)
        vit_pos = pipe.ball_detector_aux.predict_clip(images)
        keep = np.flatnonzero((np.hypot(*(wasb_pos[:, :2] - vit_pos[:, :2]).T) <= 20) & (wasb_pos[:, 2] == 1) & (vit_pos[:, 2] == 1))
        if 0 < len(keep) < len(wasb_pos):
            break
    print('\n%d frames, seed %d: the ball filter keeps %d of %d detections' % (n, seed, len(keep), len(wasb_pos)))
    assert 0 < len(keep) < len(wasb_pos)
    hrnet_kp = pipe.table_detector.predict_keypoints(images)
    vit_kp = pipe.table_detector_aux.predict_keypoints(images)

    # 1. the four raw detection arrays of the overlapped clip path
    pos, kp, pos_aux, kp_aux = pipe._clip_detections(images, True, return_aux=True)
    assert np.array_equal(pos, wasb_pos) and np.array_equal(kp, hrnet_kp)
    assert np.array_equal(pos_aux, vit_pos) and np.array_equal(kp_aux, vit_kp)
    assert not np.array_equal(pos, pos_aux) and not np.array_equal(kp, kp_aux)
    # the callers of the single-detector form are served as before
    pos1, kp1 = pipe._clip_detections(images, True)
    assert np.array_equal(pos1, wasb_pos) and np.array_equal(kp1, hrnet_kp)

    # 2. the filters: the reference's, on the two detectors' outputs
    filt, idx, times = pipe.ball_detector.filter_trajectory(pos, pos_aux, fps)
    r_filt, r_idx, r_times = glue_ref.filter_trajectory_ball(wasb_pos, vit_pos, fps)
    assert np.array_equal(filt, r_filt) and np.array_equal(idx, r_idx) and np.array_equal(times, r_times)
    table = np.asarray(pipe._clip_detections(images, True, table_consumer=lambda k, ka: pipe.table_detector_aux.filter_trajectory(k, ka))[1])
    r_table = np.asarray(glue_ref.filter_trajectory_table(hrnet_kp, vit_kp), dtype=np.float64)
    assert np.allclose(table, r_table, rtol=0, atol=1e-9, equal_nan=True), np.abs(table - r_table).max()

    # 3. predict = the uplift of those, and the serial path gives the same
    def composed():
        bc, tc, tm, mk = glue._uplifting_transform(filt, np.asarray(table, dtype=np.float64), times)
        return pipe.uplifting_model.predict_without_normalization(bc, tc, mk, tm)
    expect = _predict_or_error(composed)
    got = _predict_or_error(lambda: pipe.predict(images, fps))
    monkeypatch.setenv('TTUP_HUB_SERIAL', '1')
    serial = _predict_or_error(lambda: pipe.predict(images, fps))
    print('predict: %s' % ('ValueError in all three' if isinstance(expect[0], str) else '%d positions' % expect[1].shape[0]))
    assert _same_result(got, expect) and _same_result(serial, expect)


@pytest.mark.parametrize('n', [3, 25, 96])
def test_default_pipeline_overlapped_path_at_chunk_boundaries(default_pipe, n, monkeypatch):
    """The default (single-detector) pipeline's overlapped clip path against the detectors' own clip calls and against the serial
    path (TTUP_HUB_SERIAL=1, read per call), bit for bit: n = 3 is one triple in one chunk; 25 a second chunk of one frame, whose
    ball call is a single triple straddling the upload boundary; 96 the long-chunk regime with an 8-frame tail."""
    p = default_pipe
    assert p.ball_detector_aux is p.ball_detector and p.table_detector_aux is p.table_detector
    images = [f for f in synth.synth_frames(n, 720, 1280, seed=100 + n)[0]]
    monkeypatch.delenv('TTUP_HUB_SERIAL', raising=False)
    pos, kp = p._clip_detections(images, True)
    assert pos.shape == (n - 2, 3) and kp.shape == (n, 13, 3)
    assert np.array_equal(pos, p.ball_detector.predict_clip(images))
    assert np.array_equal(kp, p.table_detector.predict_keypoints(images))
    overlapped = _predict_or_error(lambda: p.predict(images, 60.0))
    monkeypatch.setenv('TTUP_HUB_SERIAL', '1')
    serial = _predict_or_error(lambda: p.predict(images, 60.0))
    print('\n%d frames: predict %s' % (n, 'raises ValueError in both modes' if isinstance(serial[0], str) else 'gives %d positions' % serial[1].shape[0]))
    assert _same_result(overlapped, serial)


def test_pipeline_aux_surface(monkeypatch):
    monkeypatch.setenv('TTUP_SYNTHETIC_WEIGHTS', '1')
    import hubconf
    from upliftingtabletennis_amd.interface import TableTennisPipeline, ViTPoseBallDetector, ViTPoseTableDetector
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        p = TableTennisPipeline()
        assert p.ball_detector_aux is p.ball_detector and p.table_detector_aux is p.table_detector
        del p
        p = hubconf.full_pipeline_two_detectors()
        assert type(p.ball_detector_aux) is ViTPoseBallDetector and type(p.table_detector_aux) is ViTPoseTableDetector
        del p
        p = hubconf.full_pipeline_two_detectors(ball_aux=None)
        assert p.ball_detector_aux is p.ball_detector and type(p.table_detector_aux) is ViTPoseTableDetector
        del p
    for kw in ({'ball_aux': 'hrnet'}, {'table_aux': 'wasb'}, {'ball_aux': 3}):
        with pytest.raises(ValueError):
            hubconf.full_pipeline_two_detectors(**kw)
    for kw in ({'ball_aux': 'segformerpp_b2'}, {'table_aux': 'segformerpp_b2'}):
        with pytest.raises(NotImplementedError):
            hubconf.full_pipeline_two_detectors(**kw)
