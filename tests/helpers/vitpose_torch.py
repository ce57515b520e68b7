"""Torch restatement (fp32, or fp64 with ``dtype=torch.float64``) of the reference ViTPose-small forward (balldetection/models/vitpose.py over
vit_pose/vit_models/backbone/vit.py and head/topdown_heatmap_simple_head.py), written from the contract so that the CPU tests can
check it against the goldens the reference itself produced: Conv2d(k16,s16,p2: vit.py:222 with ratio 1) patch embedding, + pos_embed[1:] + pos_embed[:1],
12 pre-LN blocks (LayerNorm eps 1e-6, 12 heads of 32, exact-erf GELU), last_norm, two ConvTranspose2d(k4,s2,p1) + BN (eps 1e-5,
running statistics) + ReLU, final 1x1 conv with bias.  Both precisions are pinned to the reference's heatmaps: at the golden
shapes of tests/golden/vitpose.npz (test_vitpose_oracle.py, fp32) and at the token-count and border edges of
tests/golden/vitpose_edges.npz (test_vitpose_edges_host.py, fp32 and fp64)."""
import torch
import torch.nn.functional as F


def forward(x, sd, prefix='model', dtype=torch.float32):
    t = lambda k: torch.as_tensor(sd[prefix + '.' + k]).to(dtype)      # noqa: E731
    x = torch.as_tensor(x).to(dtype)
    B = x.shape[0]
    y = F.conv2d(x, t('backbone.patch_embed.proj.weight'), t('backbone.patch_embed.proj.bias'), stride=16, padding=2)
    Hp, Wp = y.shape[2:]
    y = y.flatten(2).transpose(1, 2)
    pos = t('backbone.pos_embed')
    y = y + pos[:, 1:] + pos[:, :1]
    D = y.shape[2]
    for i in range(12):
        p = 'backbone.blocks.%d.' % i
        h = F.layer_norm(y, (D,), t(p + 'norm1.weight'), t(p + 'norm1.bias'), eps=1e-6)
        qkv = F.linear(h, t(p + 'attn.qkv.weight'), t(p + 'attn.qkv.bias')).reshape(B, -1, 3, 12, D // 12).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0] * (D // 12) ** -0.5, qkv[1], qkv[2]
        a = (q @ k.transpose(-2, -1)).softmax(-1)
        h = (a @ v).transpose(1, 2).reshape(B, -1, D)
        y = y + F.linear(h, t(p + 'attn.proj.weight'), t(p + 'attn.proj.bias'))
        h = F.layer_norm(y, (D,), t(p + 'norm2.weight'), t(p + 'norm2.bias'), eps=1e-6)
        h = F.linear(F.gelu(F.linear(h, t(p + 'mlp.fc1.weight'), t(p + 'mlp.fc1.bias'))), t(p + 'mlp.fc2.weight'), t(p + 'mlp.fc2.bias'))
        y = y + h
    y = F.layer_norm(y, (D,), t('backbone.last_norm.weight'), t('backbone.last_norm.bias'), eps=1e-6)
    y = y.permute(0, 2, 1).reshape(B, D, Hp, Wp)
    for i in (0, 3):
        p = 'keypoint_head.deconv_layers.'
        y = F.conv_transpose2d(y, t(p + '%d.weight' % i), stride=2, padding=1)
        y = F.batch_norm(y, t(p + '%d.running_mean' % (i + 1)), t(p + '%d.running_var' % (i + 1)), t(p + '%d.weight' % (i + 1)),
                         t(p + '%d.bias' % (i + 1)), training=False, eps=1e-5)
        y = F.relu(y)
    return F.conv2d(y, t('keypoint_head.final_layer.weight'), t('keypoint_head.final_layer.bias'))


def deconv_folded(y, wp, b):
    """One head deconvolution from the packed form (weights.vitpose_fold_head): four 2x2 sub-convolutions, BN folded, ReLU.
    y (B, cin, h, w) -> (B, cout, 2h, 2w)."""
    B, cin, h, w = y.shape
    cout = wp.shape[1]
    wp = torch.as_tensor(wp).to(y.dtype).reshape(4, cout, 2, 2, cin).permute(0, 1, 4, 2, 3)    # (phase, cout, cin, dy, dx)
    out = y.new_zeros(B, cout, 2 * h, 2 * w)
    for py in range(2):
        for px in range(2):
            # input pixel (y+py+dy-1, x+px+dx-1): pad one row/column on the side the phase reaches past
            yp = F.pad(y, (1 - px, px, 1 - py, py))
            out[:, :, py::2, px::2] = F.conv2d(yp, wp[2 * py + px])
    return F.relu(out + torch.as_tensor(b).to(y.dtype)[None, :, None, None])
