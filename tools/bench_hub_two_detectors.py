#!/usr/bin/env python3
"""The hub with two detectors per agreement filter -- hubconf.full_pipeline_two_detectors() (WASB / HRNet primaries, ViTPose-small
aux) -- against today's single-detector hubconf.full_pipeline(), in one run, on tools/bench_hub.py's synthetic 1280x720 clips:
`predict` on the 48-frame clip and the overlapped clip path (detections, both filters, uplift of the first 49) on the 256-frame
one.  Also reports the share of ball detections the two-detector filter rejects.  --aux-dtype f32 | bf16: the arithmetic of the
ViTPose aux detectors (default f32).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault('TTUP_SYNTHETIC_WEIGHTS', '1')
import hubconf  # noqa: E402
from upliftingtabletennis_amd import glue, synth  # noqa: E402

_ap = argparse.ArgumentParser()
_ap.add_argument('--aux-dtype', choices=('f32', 'bf16'), default='f32')
aux_dtype = _ap.parse_args().aux_dtype

n = int(os.environ.get('TTUP_HUB_FRAMES', '48'))
nl = int(os.environ.get('TTUP_HUB_LONG', '256'))
reps = int(os.environ.get('TTUP_HUB_REPS', '8'))
frames, _ = synth.synth_frames(n, 720, 1280, seed=0)
images = [f for f in frames]
long_images = [f for f in np.concatenate([frames] * ((nl + n - 1) // n))[:nl]]


def timed(f, k):
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k


def long_clip(hub):
    two = hub.ball_detector_aux is not hub.ball_detector
    pos, kp, pos_aux, _ = hub._clip_detections(long_images, want_table=True, return_aux=True,
                                               table_consumer=lambda k, ka=None: hub.table_detector_aux.filter_trajectory(k, k if ka is None else ka))
    filt, _, tb = hub.ball_detector.filter_trajectory(pos, pos_aux if two else pos, 60.0)
    bc, tc, tm, mk = glue._uplifting_transform(filt[:49], np.asarray(kp, dtype=np.float64), tb[:49])
    return hub.uplifting_model.predict_without_normalization(bc, tc, mk, tm)


def rejected_share(hub, clip):
    pos, _, pos_aux, _ = hub._clip_detections(clip, want_table=False, return_aux=True)
    _, keep, _ = hub.ball_detector.filter_trajectory(pos, pos_aux, 60.0)
    return 1.0 - len(keep) / len(pos)


out = {'metric': 'hub_two_detectors_fps', 'frames': n, 'long_frames': nl, 'aux_dtype': aux_dtype}
with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    for key, make in (('single', hubconf.full_pipeline), ('two', lambda: hubconf.full_pipeline_two_detectors(aux_dtype=aux_dtype))):
        hub = make()
        out['%s_fps_%d' % (key, n)] = round(n / timed(lambda: hub.predict(images, 60.0), reps), 1)
        if nl > 0:
            out['%s_fps_%d' % (key, nl)] = round(nl / timed(lambda: long_clip(hub), 3), 1)
        if key == 'two':
            # the two ViTPose passes alone on the device-resident clip: what the HRNet work and the host run beside
            fr = torch.from_numpy(frames).cuda()
            vit = lambda: (hub.ball_detector_aux.model.forward_frames(fr), hub.table_detector_aux.model.forward_frames(fr))
            out['vitpose_only_fps_%d' % n] = round(n / timed(vit, reps), 1)
            out['ball_rejected_share_%d' % n] = round(rejected_share(hub, images), 4)
            if nl > 0:
                out['ball_rejected_share_%d' % nl] = round(rejected_share(hub, long_images), 4)
        del hub
        torch.cuda.empty_cache()
print(json.dumps(out))
