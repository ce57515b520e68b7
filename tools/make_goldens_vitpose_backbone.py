#!/usr/bin/env python3
"""Generate tests/golden/vitpose_backbone_grad.npz by driving the REFERENCE's own ViT backbone (vit_pose/vit_models/backbone/vit.py,
``ViTPoseModel(cfg).backbone`` with the detectors' ``drop_path_rate=0.3``) in ``.train()``, float32 with autograd, on the golden
cases of tests/helpers/vitpose_backbone_cases.py.

Runs only where the reference sources are (TTUP_REFERENCE); the tests read the .npz alone.  Inputs are regenerated from the cases'
seeds.  The stochastic-depth factors the reference drew are recorded with forward hooks on its DropPath modules (output / input per
sample, snapped to 0 or float32(1) / float32(keep)); block 0 has rate 0 and is an Identity: ones.  Stored per case:
``<case>/scale`` (12, 2, B); ``<case>/feat`` in full; per backbone tensor ``<case>/<key suffix>``: every ``stride_small``-th element of
the flattened gradient for tensors of up to 1536 elements, every ``stride_large``-th for the others, with its L2 norm
``<case>/<key suffix>/norm``; and ``<case>/<tensor>/dist``: the reference float32 result's relative-L2 distance (over the whole
tensor) from the float64 restatement (tests/helpers/vitpose_backbone_ref.py) run on the recorded factors -- what float32 costs on that
tensor, which the GPU test takes as its measure.

    python tools/make_goldens_vitpose_backbone.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TTUP_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, REF)

from helpers import vitpose_backbone_cases as cases  # noqa: E402
from helpers import vitpose_backbone_ref as ref  # noqa: E402

STRIDE_SMALL, STRIDE_LARGE, SMALL = 7, 2003, 1536          # both prime to 384, 1152 and 1536: every row and column class is met
PREFIX = 'model.backbone.'


def stride_of(n):
    return STRIDE_SMALL if n <= SMALL else STRIDE_LARGE


def ref_backbone(sd, in_ch, hp, wp):
    if 'cv2' not in sys.modules:
        sys.modules['cv2'] = types.ModuleType('cv2')
    from balldetection.models.vitpose import get_config
    from vit_pose import ViTPoseModel
    cfg = get_config('small')
    cfg['backbone']['img_size'] = (16 * hp, 16 * wp)
    cfg['backbone']['in_chans'] = in_ch
    assert cfg['backbone']['drop_path_rate'] == cases.RATE
    net = ViTPoseModel(cfg).backbone
    net.load_state_dict({k[len(PREFIX):]: torch.tensor(np.asarray(v), dtype=torch.float32) for k, v in sd.items() if k.startswith(PREFIX)}, strict=True)
    return net


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {'stride_small': np.int64(STRIDE_SMALL), 'stride_large': np.int64(STRIDE_LARGE), 'small': np.int64(SMALL)}
    for name in cases.GOLDEN_CASES:
        b, hp, wp, c, seed, _, _ = cases.CASES[name]
        x, sd, dfeat = cases.make_case(name)
        net = ref_backbone(sd, c, hp, wp)
        net.train()
        keep = [1.0 - float(v) for v in torch.linspace(0, cases.RATE, 12)]
        scale = np.ones((12, 2, b), np.float32)
        calls = {i: 0 for i in range(12)}
        hooks = []

        def record(i):
            def hook(mod, inp, outp):
                xin, y = inp[0].detach().reshape(b, -1), outp.detach().reshape(b, -1)
                j = xin.abs().argmax(1)
                ratio = (y[torch.arange(b), j] / xin[torch.arange(b), j]).numpy()
                snapped = np.where(ratio > 0.5, np.float32(1) / np.float32(keep[i]), np.float32(0)).astype(np.float32)
                assert np.abs(snapped - ratio).max() <= 1e-6 * snapped.max(initial=1.0), (i, ratio, snapped)
                scale[i, calls[i]] = snapped
                calls[i] += 1
            return hook
        for i, blk in enumerate(net.blocks):
            if type(blk.drop_path).__name__ == 'DropPath':
                hooks.append(blk.drop_path.register_forward_hook(record(i)))
            else:
                assert i == 0, i
        torch.manual_seed(seed)
        feat = net(torch.tensor(x))
        for h in hooks:
            h.remove()
        assert all(calls[i] == 2 for i in range(1, 12)) and calls[0] == 0
        assert (scale == 0).any() and (scale[1:] > 0).any(), 'a golden case should have kept and dropped branches: pick another seed'
        feat = feat.permute(0, 2, 3, 1).reshape(-1, 384)
        feat.backward(torch.tensor(dfeat))
        grads = {PREFIX + k: p.grad for k, p in net.named_parameters()}
        want_feat, want = ref.forward_backward(x, sd, dfeat, scale, dtype=torch.float64)
        assert sorted(grads) == sorted(want) and len(want) == 149
        out[name + '/scale'] = scale
        out[name + '/feat'] = feat.detach().numpy().astype(np.float32)
        out[name + '/feat/dist'] = np.float64(ref.rel_l2(out[name + '/feat'], want_feat))
        print('%s feat: distance from the restatement %.3g; dropped %d of %d' % (name, out[name + '/feat/dist'], int((scale == 0).sum()), scale.size))
        worst = 0.0
        for k, w in want.items():
            v = grads[k].detach().numpy().astype(np.float32) if grads[k] is not None else np.zeros(w.shape, np.float32)
            assert v.shape == w.shape, (k, v.shape, w.shape)
            s = k[len(PREFIX):]
            dist = ref.rel_l2(v, w)
            worst = max(worst, dist)
            out['%s/%s/dist' % (name, s)] = np.float64(dist)
            out['%s/%s/norm' % (name, s)] = np.float64(np.linalg.norm(v.astype(np.float64).ravel()))
            out['%s/%s' % (name, s)] = v.ravel()[::stride_of(v.size)].copy()
        print('%s gradients: worst distance from the restatement %.3g' % (name, worst))
    path = os.path.join(ROOT, 'tests', 'golden', 'vitpose_backbone_grad.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
