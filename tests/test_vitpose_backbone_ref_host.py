"""The float64 oracle of the ViTPose backbone's training pass (tests/helpers/vitpose_backbone_ref.py) held, on the CPU, to the two things
it restates: with unit scales it is tests/helpers/vitpose_torch.py up to last_norm, and with the factors the reference's DropPath
modules drew it is the reference's own ViT in .train() (tests/golden/vitpose_backbone_grad.npz, made by
tools/make_goldens_vitpose_backbone.py: feat in full, a strided sample and the L2 norm of each of the 149 gradients, and per tensor the
reference float32 run's own distance from the restatement).  The bar against the goldens is ten times that recorded distance."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import vitpose_backbone_cases as cases
from helpers import vitpose_backbone_ref as ref
from helpers import vitpose_torch
from upliftingtabletennis_amd import weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vitpose_backbone_grad.npz')
PREFIX = 'model.backbone.'


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def head(feat, sd, b, hp, wp, dtype=torch.float64):
    """vitpose_torch.forward's lines behind last_norm"""
    t = lambda k: torch.as_tensor(sd['model.' + k]).to(dtype)      # noqa: E731
    y = feat.reshape(b, hp * wp, 384).permute(0, 2, 1).reshape(b, 384, hp, wp)
    for i in (0, 3):
        p = 'keypoint_head.deconv_layers.'
        y = F.conv_transpose2d(y, t(p + '%d.weight' % i), stride=2, padding=1)
        y = F.batch_norm(y, t(p + '%d.running_mean' % (i + 1)), t(p + '%d.running_var' % (i + 1)), t(p + '%d.weight' % (i + 1)),
                         t(p + '%d.bias' % (i + 1)), training=False, eps=1e-5)
        y = F.relu(y)
    return F.conv2d(y, t('keypoint_head.final_layer.weight'), t('keypoint_head.final_layer.bias'))


@pytest.mark.parametrize('scale', [None, 'ones'])
def test_unit_scales_are_the_inference_forward(scale):
    b, hp, wp, c = 2, 2, 3, 3
    sd = weights.random_vitpose_state_dict(3, in_ch=c, out_ch=2, resolution=(16 * wp, 16 * hp), planted=False)
    x = np.random.default_rng(4).standard_normal((b, c, 16 * hp, 16 * wp))
    s = None if scale is None else np.ones((12, 2, b))
    feat = ref.forward(x, sd, s, dtype=torch.float64)
    assert tuple(feat.shape) == (b * hp * wp, 384)
    want = vitpose_torch.forward(x, sd, dtype=torch.float64)
    got = head(feat, sd, b, hp, wp)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_a_dropped_branch_is_the_identity_and_has_no_gradient():
    name = 'g2x3_one'
    b = cases.CASES[name][0]
    x, sd, dfeat = cases.make_case(name)
    s = np.ones((12, 2, b), np.float32)
    s[5] = 0
    _, g = ref.forward_backward(x, sd, dfeat, s)
    for k, v in g.items():
        assert (not v.any()) == ('.blocks.5.' in k), k


@pytest.mark.parametrize('name', cases.GOLDEN_CASES)
def test_against_the_reference_in_train_mode(golden, name):
    b, hp, wp, c, _, _, _ = cases.CASES[name]
    x, sd, dfeat = cases.make_case(name)
    scale = cases.scales(name, golden)
    assert scale.shape == (12, 2, b) and (scale[0] == 1).all() and (scale == 0).any()
    keep = np.asarray(cases.keep(), np.float32).reshape(12, 1, 1)
    assert np.all((scale == 0) | (np.abs(scale * keep - 1) <= 1e-6))          # 0 or 1 / keep_i
    feat, grads = ref.forward_backward(x, sd, dfeat, scale, dtype=torch.float64)
    assert len(grads) == 149
    d = float(golden[name + '/feat/dist'])
    assert 0 < d <= 1e-5 and ref.rel_l2(feat, golden[name + '/feat']) <= 10 * d
    small, ss, sl = int(golden['small']), int(golden['stride_small']), int(golden['stride_large'])
    for k, v in grads.items():
        s = k[len(PREFIX):]
        d = float(golden['%s/%s/dist' % (name, s)])
        assert d <= 1e-5, (s, d)
        sample = v.ravel()[::ss if v.size <= small else sl]
        want = golden['%s/%s' % (name, s)]
        assert sample.shape == want.shape, s
        # the sample against the whole tensor's norm scaled to the sample's size: a sample of a few elements has no norm of its own to speak of
        scale_norm = float(golden['%s/%s/norm' % (name, s)]) * np.sqrt(sample.size / v.size)
        err = np.linalg.norm(sample - want)
        assert err <= 10 * d * max(scale_norm, np.linalg.norm(want)), (s, err, d, scale_norm)
        assert abs(np.linalg.norm(v.ravel()) - float(golden['%s/%s/norm' % (name, s)])) <= 10 * d * np.linalg.norm(v.ravel()), s
