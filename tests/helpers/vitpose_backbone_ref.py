"""The ViTPose-small backbone's training-mode forward restated in torch, in float64 or float32 on the CPU, with torch autograd for the
gradients: tests/helpers/vitpose_torch.py up to last_norm, with a per-sample scale on each residual branch.

    x0 = patch_embed(img) + pos[1:] + pos[:1]                    Conv2d(C, 384, k16, s16, p2)
    for i in 0..11:
      x  = x + s[i,0,b] * proj(attn(qkv(LN1(x))))                12 heads of 32, q scaled by 32^-1/2, LN eps 1e-6
      x  = x + s[i,1,b] * fc2(gelu(fc1(LN2(x))))                 exact-erf GELU
    feat = last_norm(x)                                          (B * tokens, 384)

`s` (12, 2, B): the reference's stochastic depth multiplies a branch, per sample, by 0 or 1 / keep (vit.py:19-36, :203-204); None is
all ones, the backbone in eval().  There is no ReLU in the backbone, so no gate needs deciding."""
import numpy as np
import torch
import torch.nn.functional as F

DEPTH, HEADS = 12, 12


def keys(sd, prefix='model'):
    """the backbone's keys of sd in state_dict order"""
    return [k for k in sd if k.startswith(prefix + '.backbone.')]


def forward(x, sd, drop_scale=None, prefix='model', dtype=torch.float64):
    """x (B, C, H, W); sd: {key: array or tensor} (tensors are used as they are, so that autograd reaches them) -> feat (B * tokens, 384)"""
    t = lambda k: sd[prefix + '.backbone.' + k] if torch.is_tensor(sd[prefix + '.backbone.' + k]) else torch.as_tensor(np.asarray(sd[prefix + '.backbone.' + k])).to(dtype)      # noqa: E731
    x = torch.as_tensor(np.asarray(x)).to(dtype)
    B = x.shape[0]
    s = None if drop_scale is None else torch.as_tensor(np.asarray(drop_scale)).to(dtype).reshape(DEPTH, 2, B, 1, 1)
    y = F.conv2d(x, t('patch_embed.proj.weight'), t('patch_embed.proj.bias'), stride=16, padding=2)
    y = y.flatten(2).transpose(1, 2)
    pos = t('pos_embed')
    y = y + pos[:, 1:] + pos[:, :1]
    D = y.shape[2]
    for i in range(DEPTH):
        p = 'blocks.%d.' % i
        h = F.layer_norm(y, (D,), t(p + 'norm1.weight'), t(p + 'norm1.bias'), eps=1e-6)
        qkv = F.linear(h, t(p + 'attn.qkv.weight'), t(p + 'attn.qkv.bias')).reshape(B, -1, 3, HEADS, D // HEADS).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0] * (D // HEADS) ** -0.5, qkv[1], qkv[2]
        a = (q @ k.transpose(-2, -1)).softmax(-1)
        h = (a @ v).transpose(1, 2).reshape(B, -1, D)
        h = F.linear(h, t(p + 'attn.proj.weight'), t(p + 'attn.proj.bias'))
        y = y + (h if s is None else s[i, 0] * h)
        h = F.layer_norm(y, (D,), t(p + 'norm2.weight'), t(p + 'norm2.bias'), eps=1e-6)
        h = F.linear(F.gelu(F.linear(h, t(p + 'mlp.fc1.weight'), t(p + 'mlp.fc1.bias'))), t(p + 'mlp.fc2.weight'), t(p + 'mlp.fc2.bias'))
        y = y + (h if s is None else s[i, 1] * h)
    y = F.layer_norm(y, (D,), t('last_norm.weight'), t('last_norm.bias'), eps=1e-6)
    return y.reshape(-1, D)


def forward_backward(x, sd, dfeat, drop_scale=None, prefix='model', dtype=torch.float64):
    """-> (feat, {key: gradient}) as float64 numpy: the gradient of sum(feat * dfeat) into every backbone tensor, by autograd"""
    ks = keys(sd, prefix)
    leaves = {k: torch.tensor(np.asarray(sd[k]), dtype=dtype, requires_grad=True) for k in ks}
    feat = forward(x, leaves, drop_scale, prefix, dtype)
    feat.backward(torch.as_tensor(np.asarray(dfeat)).to(dtype))
    return feat.detach().double().numpy(), {k: leaves[k].grad.double().numpy() for k in ks}


def rel_l2(a, b):
    """|a - b|_2 / |b|_2 (0 / 0 = 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d, n = np.linalg.norm((a - b).ravel()), np.linalg.norm(b.ravel())
    return 0.0 if d == 0 else d / n if n > 0 else np.inf


def rel_max(a, b):
    """max |a - b| over the largest magnitude of b (0 / 0 = 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d, n = np.abs(a - b).max(initial=0.0), np.abs(b).max(initial=0.0)
    return 0.0 if d == 0 else d / n if n > 0 else np.inf


def family(key):
    """the tensor family of a key, for reporting: 'blocks.3.attn.qkv.weight' -> 'attn.qkv.weight'"""
    k = key.split('.backbone.')[-1]
    return k.split('.', 2)[2] if k.startswith('blocks.') else k
