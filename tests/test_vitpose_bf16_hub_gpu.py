"""The bf16 ViTPose detectors on the hub surface, full size (1152x640), synthetic weights, 8 frames: `BallDetector('vitpose',
dtype='bf16')` and the table twin against the f32 detectors (the existing, pinned path), and the two-detector pipeline with
`aux_dtype='bf16'` against `aux_dtype='f32'`.  The bars are those of tests/test_vitpose_bf16_gpu.py (b): computed from what the
rounding oracle itself loses over the sweep, not typed in."""
import os
import warnings

import numpy as np
import pytest
import torch

from helpers.vitpose_bf16_cases import heat_bar as _heat_bar, position_bar as _position_bar
from upliftingtabletennis_amd import synth

pytestmark = pytest.mark.gpu

N_FRAMES = 8


@pytest.fixture(scope='module')
def synthetic_weights():
    old = os.environ.get('TTUP_SYNTHETIC_WEIGHTS')
    os.environ['TTUP_SYNTHETIC_WEIGHTS'] = '1'
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        yield
    if old is None:
        os.environ.pop('TTUP_SYNTHETIC_WEIGHTS', None)
    else:
        os.environ['TTUP_SYNTHETIC_WEIGHTS'] = old


@pytest.fixture(scope='module')
def images():
    return [f for f in synth.synth_frames(N_FRAMES, 720, 1280, seed=7)[0]]


def _compare(det16, det32, images, predict):
    """Shapes, dtypes and visibility of `predict`; argmax and positions map by map where the f32 map is decided."""
    from upliftingtabletennis_amd.interface import _ViTPoseHooks
    for d, dtype in ((det16, 'bf16'), (det32, 'f32')):
        assert isinstance(d, _ViTPoseHooks) and d.model.dtype == dtype and d.cert is None
    got, want = np.asarray(predict(det16)), np.asarray(predict(det32))
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    got, want = got.reshape(-1, 3), want.reshape(-1, 3)
    assert np.array_equal(got[:, 2], want[:, 2])                                   # visibility
    fr = det32._upload(images)
    h16, i16, _ = det16.model.forward_frames(fr, want_heatmap=True)
    h32, i32, _ = det32.model.forward_frames(fr, want_heatmap=True)
    torch.cuda.synchronize()
    assert h16.shape == h32.shape and h16.dtype == h32.dtype == torch.float32 and i16.dtype == i32.dtype == torch.int64
    maps = h32.reshape(i32.numel(), -1).double()
    top = maps.topk(2, dim=1).values
    rng = maps.max(1).values - maps.min(1).values
    decided = ((top[:, 0] - top[:, 1]) > 2 * _heat_bar() * rng).cpu().numpy()
    err = float(((h16.reshape(i32.numel(), -1).double() - maps).abs().max(1).values / rng).max())
    print('\n%s: %d of %d maps decided at twice the bar %.3g; bf16 heatmaps within %.3g of the range of the f32 ones'
          % (type(det16).__name__, decided.sum(), decided.size, _heat_bar(), err))
    assert decided.mean() >= 0.9
    assert np.array_equal(i16.cpu().numpy()[decided], i32.cpu().numpy()[decided])
    hh, ww = det32.heat_hw
    px = _position_bar() * max(det32.resolution[0] / ww, det32.resolution[1] / hh)          # heatmap px -> image px
    shift = float(np.abs(got[decided, :2] - want[decided, :2]).max())
    print('positions: worst shift %.3g image px, bar %.3g' % (shift, px))
    assert shift <= px


def test_ball_detector(synthetic_weights, images):
    from upliftingtabletennis_amd.interface import BallDetector, ViTPoseBallDetector
    det16, det32 = BallDetector('vitpose', max_batch=N_FRAMES, dtype='bf16'), BallDetector('vitpose', max_batch=N_FRAMES)
    assert type(det16) is ViTPoseBallDetector
    _compare(det16, det32, images, lambda d: d.predict_clip(images))
    assert np.asarray(det16.predict_clip(images)).shape == (N_FRAMES - 2, 3)


def test_table_detector(synthetic_weights, images):
    from upliftingtabletennis_amd.interface import TableDetector, ViTPoseTableDetector
    det16, det32 = TableDetector('vitpose', max_batch=N_FRAMES, dtype='bf16'), TableDetector('vitpose', max_batch=N_FRAMES)
    assert type(det16) is ViTPoseTableDetector
    _compare(det16, det32, images, lambda d: d.predict_keypoints(images))
    assert np.asarray(det16.predict_keypoints(images)).shape == (N_FRAMES, 13, 3)


def test_pipeline_keeps_the_same_frames(synthetic_weights, images):
    """`TableTennisPipeline(..., aux_dtype='bf16')` keeps, on the same clip, the frames and keypoints the f32 aux detectors keep: the
    same indices out of the ball filter, the same keypoints visible out of the table filter, and the same `predict` outcome."""
    from upliftingtabletennis_amd.interface import TableTennisPipeline
    out = {}
    for dtype in ('f32', 'bf16'):
        pipe = TableTennisPipeline(max_batch=N_FRAMES, ball_aux='vitpose', table_aux='vitpose', aux_dtype=dtype)
        assert pipe.ball_detector_aux.model.dtype == dtype and pipe.table_detector_aux.model.dtype == dtype
        assert pipe.ball_detector_aux.cert is None and pipe.table_detector_aux.cert is None
        pos, kp, pos_aux, kp_aux = pipe._clip_detections(images, True, return_aux=True)
        _, idx, _ = pipe.ball_detector.filter_trajectory(pos, pos_aux, 60.0)
        table = np.asarray(pipe.table_detector_aux.filter_trajectory(kp, kp_aux))
        spin, traj = pipe.predict(images, 60.0)          # succeeds on this clip: 6 kept detections, fewer than the mask's 50
        pred = np.asarray(traj).shape
        assert pred == (len(idx), 3) and len(idx) > 0
        out[dtype] = (np.asarray(idx), table[:, 2], pred)
        del pipe
        torch.cuda.empty_cache()
    print('\nball filter keeps %s; %d table keypoints visible; predict: %s' % (out['f32'][0].tolist(), int(out['f32'][1].sum()), out['f32'][2]))
    assert np.array_equal(out['bf16'][0], out['f32'][0])
    assert np.array_equal(out['bf16'][1], out['f32'][1])
    assert out['bf16'][2] == out['f32'][2]
