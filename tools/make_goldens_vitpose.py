#!/usr/bin/env python3
"""Generate tests/golden/vitpose.npz by running the REFERENCE's own ViTPose modules (vit_pose/vit_models) on seeded weights.

Runs only where the reference sources are (TTUP_REFERENCE); the GPU tests read the .npz alone.  The reference's ``VitPose``
wrapper reads an MAE initialisation file in its constructor, so the model is built the way the wrapper builds it without that
step: ``ViTPoseModel(get_config())`` with the wrapper's two changes (img_size = resolution, patch embedding with 3*in_frames input
channels; ``num_output_channels``), then ``load_state_dict(strict=True)`` of ``weights.random_vitpose_state_dict`` (the
``model.`` prefix of the wrapper's checkpoint keys dropped).  ``cv2`` is stubbed (imported by vit_utils, unused on the forward).

Cases (inputs regenerated from seeds by ``synth.vitpose_inputs``): ball 9-ch at 160x288 and 96x176 (Hp x Wp = 6 x 11), table 3-ch /
13 maps at 96x176 -- full heatmaps; ball 9-ch at 640x1152 (2 inputs) -- argmax, margins, statistics and a 32x32 crop around each peak.
Every case stores per-map argmax, top-2 margin, range and the refined positions (table variant of the refine, 1920x1080).

    python tools/make_goldens_vitpose.py

``--edges`` writes tests/golden/vitpose_edges.npz instead: full reference heatmaps (with meta, argmax, margin, range) of the
gain-1 cases of tests/helpers/vitpose_edge_cases.py with 1, 3 (one patch row, one patch column), 63, 65 and 127 tokens, which pin
the torch restatement at the shapes where the GPU tests use it as their fp64 reference.

    python tools/make_goldens_vitpose.py --edges
"""
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TTUP_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, REF)

from helpers import vitpose_edge_cases as edges  # noqa: E402
from oracle import refine_ref  # noqa: E402
from upliftingtabletennis_amd import synth, weights  # noqa: E402

# name: (weight seed, input seed, batch, in_ch, out_ch, h, w, full heatmap stored)
CASES = {
    'ball_160x288': (11, 21, 2, 9, 1, 160, 288, 1),
    'ball_96x176': (12, 22, 3, 9, 1, 96, 176, 1),
    'table_96x176': (13, 23, 2, 3, 13, 96, 176, 1),
    'ball_640x1152': (14, 24, 2, 9, 1, 640, 1152, 0),
}
CROP = 32
# --edges: name -> case of the edge sweep (h, w, in_ch, out_ch, batch, gain 1); seeds, weights and inputs are the sweep's own
EDGE_CASES = {'edge_' + edges.case_id(c): c for c in edges.golden_cases()}


def ref_model(sd, in_ch, out_ch, h, w):
    if 'cv2' not in sys.modules:
        sys.modules['cv2'] = types.ModuleType('cv2')
    from balldetection.models.vitpose import get_config
    from vit_pose import ViTPoseModel
    cfg = get_config('small')
    cfg['backbone']['img_size'] = (w, h)
    cfg['backbone']['in_chans'] = in_ch
    cfg['keypoint_head']['out_channels'] = out_ch
    m = ViTPoseModel(cfg).eval()
    m.load_state_dict({k[len('model.'):]: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m


def main_edges():
    torch.set_num_threads(os.cpu_count() or 1)
    out = {}
    for name, case in EDGE_CASES.items():
        h, w, cin, cout, b, gain = case
        assert gain == 1
        with torch.no_grad():
            heat = ref_model(edges.state_dict(case), cin, cout, h, w)(torch.from_numpy(edges.inputs(case))).numpy()
        assert heat.shape == (b, cout, h // 4, w // 4), heat.shape
        maps = heat.reshape(b * cout, -1)
        srt = np.sort(maps, axis=1)
        out[name + '/meta'] = np.array([edges.WEIGHT_SEED, edges.INPUT_SEED, b, cin, cout, h, w, 1], np.int64)
        out[name + '/argmax'] = maps.argmax(1).astype(np.int64)
        out[name + '/margin'] = (srt[:, -1] - srt[:, -2]).astype(np.float32)
        out[name + '/range'] = (srt[:, -1] - srt[:, 0]).astype(np.float32)
        out[name + '/heat'] = heat.astype(np.float32)
        print('%s: heat %s, range %s, margin/range %s' % (name, heat.shape, out[name + '/range'].min(),
                                                          (out[name + '/margin'] / out[name + '/range']).min()))
    path = os.path.join(ROOT, 'tests', 'golden', 'vitpose_edges.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


def main():
    torch.set_num_threads(os.cpu_count() or 1)
    out = {}
    for name, (ws, xs, b, cin, cout, h, w, full) in CASES.items():
        t0 = time.time()
        sd = weights.random_vitpose_state_dict(ws, in_ch=cin, out_ch=cout, resolution=(w, h))
        x, _ = synth.vitpose_inputs(xs, b, cin, h, w)
        with torch.no_grad():
            heat = ref_model(sd, cin, cout, h, w)(torch.from_numpy(x)).numpy()
        assert heat.shape == (b, cout, h // 4, w // 4), heat.shape
        maps = heat.reshape(b * cout, -1)
        srt = np.sort(maps, axis=1)
        out[name + '/meta'] = np.array([ws, xs, b, cin, cout, h, w, full], np.int64)
        out[name + '/argmax'] = maps.argmax(1).astype(np.int64)
        out[name + '/margin'] = (srt[:, -1] - srt[:, -2]).astype(np.float32)
        out[name + '/range'] = (srt[:, -1] - srt[:, 0]).astype(np.float32)
        out[name + '/xyv'] = refine_ref.extract_position_table(heat.reshape(b * cout, 1, h // 4, w // 4), 1920, 1080).reshape(b * cout, 3)
        if full:
            out[name + '/heat'] = heat.astype(np.float32)
        else:
            hh, ww = h // 4, w // 4
            crops, org = [], []
            for k, i in enumerate(out[name + '/argmax']):
                y0 = int(min(max(i // ww - CROP // 2, 0), hh - CROP)); x0 = int(min(max(i % ww - CROP // 2, 0), ww - CROP))
                crops.append(maps[k].reshape(hh, ww)[y0:y0 + CROP, x0:x0 + CROP]); org.append((y0, x0))
            out[name + '/crop'] = np.stack(crops).astype(np.float32)
            out[name + '/crop_origin'] = np.array(org, np.int64)
            out[name + '/stats'] = np.stack([maps.mean(1), maps.std(1)], 1).astype(np.float32)
        print('%s: heat %s, range %s, margin/range %s, %.1f s' % (name, heat.shape, out[name + '/range'].min(),
                                                                  (out[name + '/margin'] / out[name + '/range']).min(), time.time() - t0))
    path = os.path.join(ROOT, 'tests', 'golden', 'vitpose.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if sys.argv[1:] == ['--edges']:
        main_edges()
    elif sys.argv[1:]:
        sys.exit('usage: make_goldens_vitpose.py [--edges]')
    else:
        main()
