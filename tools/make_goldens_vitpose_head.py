#!/usr/bin/env python3
"""Generate tests/golden/vitpose_head_grad.npz by driving the REFERENCE's own keypoint head (vit_pose/vit_models:
``ViTPoseModel(cfg).keypoint_head``, a TopdownHeatmapSimpleHead) in ``.train()`` and ``.eval()``, float32 with autograd, on three
cases of tests/helpers/vitpose_head_cases.py.

Runs only where the reference sources are (TTUP_REFERENCE); the tests read the .npz alone.  Inputs are regenerated from the cases'
seeds.  Stored per case ``<case>/<tensor>``: heat, the running statistics after the forward (rm1, rv1, rm2, rv2),
num_batches_tracked, dfeat and the small gradients (dg1, db1, dg2, db2, dWf, dbf) in full; dW1 and dW2 as every
``subsample_stride``-th element of the flattened tensor (the rule is the file's ``subsample_stride``) with their L2 norms
``<case>/dW1/norm``; and for every tensor ``<case>/<tensor>/dist``, the reference float32 result's relative-L2 distance from the float64
restatement (tests/helpers/vitpose_head_ref.py) -- what float32 costs on that tensor, which the GPU test takes as its measure.

    python tools/make_goldens_vitpose_head.py
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

from helpers import vitpose_head_cases as cases  # noqa: E402
from helpers import vitpose_head_ref as ref  # noqa: E402

STRIDE = 61          # dW1 / dW2: every 61st element of the flattened tensor (coprime to 4, 16, 256 and 384: every tap, row and column class is met)


def ref_head(p, out_ch):
    if 'cv2' not in sys.modules:
        sys.modules['cv2'] = types.ModuleType('cv2')
    from balldetection.models.vitpose import get_config
    from vit_pose import ViTPoseModel
    cfg = get_config('small')
    cfg['backbone']['img_size'] = (32, 32)
    cfg['keypoint_head']['out_channels'] = out_ch
    head = ViTPoseModel(cfg).keypoint_head
    t = lambda v: torch.tensor(np.asarray(v), dtype=torch.float32)
    sd = {'final_layer.weight': t(p['Wf'])[:, :, None, None], 'final_layer.bias': t(p['bf'])}
    for l, i in (('1', 0), ('2', 3)):
        sd['deconv_layers.%d.weight' % i] = t(p['W' + l])
        for k, f in (('weight', 'g'), ('bias', 'b'), ('running_mean', 'rm'), ('running_var', 'rv')):
            sd['deconv_layers.%d.%s' % (i + 1, k)] = t(p[f + l])
        sd['deconv_layers.%d.num_batches_tracked' % (i + 1)] = torch.tensor(0)
    head.load_state_dict(sd, strict=True)
    return head


def main():
    torch.set_num_threads(os.cpu_count() or 1)
    out = {'subsample_stride': np.int64(STRIDE)}
    for name in cases.GOLDEN_CASES:
        b, hp, wp, c, seed, train = cases.CASES[name]
        feat, p, dheat = cases.make_case(name)
        head = ref_head(p, c)
        head.train() if train else head.eval()
        x = torch.tensor(feat, dtype=torch.float32, requires_grad=True)
        heat = head(x)
        assert tuple(heat.shape) == (b, c, 4 * hp, 4 * wp), heat.shape
        heat.backward(torch.tensor(dheat, dtype=torch.float32))
        par = dict(head.named_parameters())
        buf = dict(head.named_buffers())
        got = {'heat': heat.detach(), 'dfeat': x.grad, 'dWf': par['final_layer.weight'].grad[:, :, 0, 0], 'dbf': par['final_layer.bias'].grad}
        for l, i in (('1', 0), ('2', 3)):
            got['dW' + l] = par['deconv_layers.%d.weight' % i].grad
            got['dg' + l], got['db' + l] = par['deconv_layers.%d.weight' % (i + 1)].grad, par['deconv_layers.%d.bias' % (i + 1)].grad
            got['rm' + l], got['rv' + l] = buf['deconv_layers.%d.running_mean' % (i + 1)], buf['deconv_layers.%d.running_var' % (i + 1)]
        tracked = {int(buf['deconv_layers.%d.num_batches_tracked' % i]) for i in (1, 4)}
        assert len(tracked) == 1
        out[name + '/num_batches_tracked'] = np.int64(tracked.pop())
        f = ref.forward(feat, p, train)
        g = ref.backward(f, p, dheat, train)
        want = {'heat': f['heat'], 'rm1': f['rm1'], 'rv1': f['rv1'], 'rm2': f['rm2'], 'rv2': f['rv2'], 'dfeat': g['feat']}
        want.update({'d' + k: g[k] for k in ref.GRADS})
        for k, w in want.items():
            v = got[k].detach().numpy().astype(np.float32)
            assert v.shape == w.shape, (k, v.shape, w.shape)
            dist = ref.rel_l2(v, w)
            out['%s/%s/dist' % (name, k)] = np.float64(dist)
            if k in ('dW1', 'dW2'):
                out['%s/%s/norm' % (name, k)] = np.float64(np.linalg.norm(v.astype(np.float64).ravel()))
                v = v.ravel()[::STRIDE]
            out['%s/%s' % (name, k)] = v
            print('%s %s: %s, distance from the restatement %.3g' % (name, k, v.shape, dist))
    path = os.path.join(ROOT, 'tests', 'golden', 'vitpose_head_grad.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
