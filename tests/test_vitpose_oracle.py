"""CPU checks of the ViTPose contract (tests/golden/vitpose.npz, made by tools/make_goldens_vitpose.py from the reference's own
vit_pose modules): the torch restatement in tests/helpers reproduces the reference heatmaps, and the blob packer's BN-folded
phase form of the head deconvolutions equals ConvTranspose2d + BN."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import vitpose_torch
from upliftingtabletennis_amd import synth, weights

SMALL = ['ball_160x288', 'ball_96x176', 'table_96x176']


def _case(g, name):
    ws, xs, b, cin, cout, h, w, full = [int(v) for v in g[name + '/meta']]
    sd = weights.random_vitpose_state_dict(ws, in_ch=cin, out_ch=cout, resolution=(w, h))
    x, _ = synth.vitpose_inputs(xs, b, cin, h, w)
    return sd, x, (b, cin, cout, h, w)


@pytest.mark.parametrize('name', SMALL)
def test_restatement_matches_reference_heatmaps(golden, name):
    g = golden('vitpose.npz')
    sd, x, (b, cin, cout, h, w) = _case(g, name)
    with torch.no_grad():
        got = vitpose_torch.forward(x, sd).numpy()
    ref = g[name + '/heat']
    assert got.shape == ref.shape == (b, cout, h // 4, w // 4)
    assert np.abs(got - ref).max() <= 1e-5 * (ref.max() - ref.min())
    assert np.array_equal(got.reshape(b * cout, -1).argmax(1), g[name + '/argmax'])


@pytest.mark.parametrize('layer', [0, 1])
def test_packed_deconv_bn_fold_equals_unfolded(layer):
    sd = weights.random_vitpose_state_dict(5, resolution=(176, 96))
    cin = 384 if layer == 0 else 256
    x = torch.from_numpy(np.random.default_rng(layer).standard_normal((2, cin, 6, 11)).astype(np.float32))
    i = 3 * layer
    t = lambda k: torch.from_numpy(sd['model.keypoint_head.deconv_layers.' + k])      # noqa: E731
    ref = F.relu(F.batch_norm(F.conv_transpose2d(x, t('%d.weight' % i), stride=2, padding=1), t('%d.running_mean' % (i + 1)),
                              t('%d.running_var' % (i + 1)), t('%d.weight' % (i + 1)), t('%d.bias' % (i + 1)), training=False, eps=1e-5))
    wp, b = weights.vitpose_fold_head(sd)[layer]
    got = vitpose_torch.deconv_folded(x, wp, b)
    assert np.abs((got - ref).numpy()).max() <= 1e-5 * float(ref.abs().max())


def test_blob_layout():
    sd = weights.random_vitpose_state_dict(1, in_ch=3, out_ch=13, resolution=(176, 96))
    blob = weights.pack_vitpose_blob(sd, in_ch=3, out_ch=13)
    assert blob[:8] == weights.VITPOSE_MAGIC
    hdr = np.frombuffer(blob[8:40], np.int32)
    assert list(hdr) == [3, 13, 384, 12, 12, 1536, 256, 6 * 11 + 1]
    n = sum(int(np.prod(s)) for k, s in weights.vitpose_schema(3, 13, (176, 96)) if 'deconv_layers' not in k)
    n += 4 * 256 * 4 * 384 + 256 + 4 * 256 * 4 * 256 + 256
    assert len(blob) == 40 + 4 * n
    # the packed pos_embed and final layer sit where include/ttup.h says
    f = np.frombuffer(blob[40:], np.float32)
    assert np.array_equal(f[:67 * 384], sd['model.backbone.pos_embed'].ravel())
    assert np.array_equal(f[-13:], sd['model.keypoint_head.final_layer.bias'])
    with pytest.raises(ValueError):
        weights.pack_vitpose_blob(sd, in_ch=9, out_ch=13)
