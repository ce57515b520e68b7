"""Differentiable torch restatement of the reference's uplift training step for get_model('connectstage', size, 'dynamic', rot):
forward (uplifting/model.py:529-571, as oracle/uplift_ref.py restates it under no_grad), the loss of uplifting/train.py:105-127
and `loss.backward()`.  fp32 on the CPU; tests/golden/uplift_grad.npz (the reference's own autograd) pins it, and it gives the GPU
tests full gradients at shapes the fixture only samples.

Do not run ALL of it in float64 as a "ground truth": pos = round(t * 500) rounds differently there for time stamps such as 0.025 s,
which makes it another function.  `forward_np(..., high_precision=True)` is the high-precision mode that keeps the function: weights
and activations in float64, while the time stamps stay float32 so that the RoPE index round(times / (1/500)) (and the table tokens'
arange(13) / 100) is evaluated in float32 exactly as the reference does and only then cast.  `forward` takes the working type from
`ball`; in float32 every operation is what it was before that mode existed (a `.to()` of a tensor to its own type returns it).
tests/test_uplift_grad_oracle.py holds the float32 path to the fixtures."""
import numpy as np
import torch
import torch.nn.functional as F

MAX_FPS = 500
SIZES = {'small': (32, 8, 4), 'base': (64, 12, 4), 'large': (128, 16, 4), 'huge': (192, 16, 8)}


def _linear(x, sd, p):
    return F.linear(x, sd[p + '.weight'], sd.get(p + '.bias'))


RELU_MARGIN = 2.0 ** -24      # fp32's unit roundoff
_margins = None               # while loss_and_grad(..., margins=[]) runs: the list that collects (layer, rows, margin)


def _relu_linear(x, sd, p):
    """relu(linear(x)).  When margins are collected, records how close the layer's ReLU inputs y = sum_k x_k w_k + b come to the
    kink: min |y| / (sum_k |x_k w_k| + |b|) over its rows.  Below 2^-24 a sum is smaller than the rounding error of one of its
    additions, so its sign -- whether a whole token's gradient passes that unit -- depends on the order of summation."""
    y = _linear(x, sd, p)
    if _margins is not None:
        with torch.no_grad():
            scale = x.abs() @ sd[p + '.weight'].abs().T + sd[p + '.bias'].abs()
            _margins.append((p, y.numel() // y.shape[-1], float((y.abs() / scale).min())))
    return F.relu(y)


def relu_margin(margins, max_rows=None):
    """Smallest margin over the ReLU-input layers (those applied to fewer than `max_rows` rows, when given)."""
    return min(m for _, rows, m in margins if max_rows is None or rows < max_rows)


def _mlp2(x, sd, p):
    return _linear(_relu_linear(x, sd, p + '.fc1'), sd, p + '.fc2')


def _head(x, sd, p):
    return _linear(_relu_linear(_relu_linear(x, sd, p + '.fc1'), sd, p + '.fc2'), sd, p + '.fc3')


def rope(x, times, head_dim, time_rotation):
    """model.py:56-102.  x (B,h,T,D), times (B,T)."""
    inv_freq = 1.0 / (10000 ** (torch.arange(0, head_dim, 2).float() / head_dim))
    if time_rotation == 'new':
        pos = torch.round(times / (1 / MAX_FPS))
    else:
        pos = torch.arange(x.shape[2], dtype=x.dtype)[None].expand(x.shape[0], -1)
    freqs = torch.einsum('bi,j->bij', pos.to(x.dtype), inv_freq.to(x.dtype)).unsqueeze(1)          # (index and inv_freq are float32 values in either mode)
    cos, sin = torch.cos(freqs), torch.sin(freqs)
    a, b = x[..., 0::2], x[..., 1::2]
    return torch.stack((a * cos - b * sin, a * sin + b * cos), -1).flatten(-2)


def attention(x, sd, p, mask, times, num_cls, heads, time_rotation):
    """model.py:186-229."""
    B, N, C = x.shape
    qkv = _linear(x, sd, p + '.qkv').reshape(B, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    if num_cls > 0:
        cq, q = q[:, :, :num_cls], q[:, :, num_cls:]
        ck, k = k[:, :, :num_cls], k[:, :, num_cls:]
    q, k = rope(q, times, C // heads, time_rotation), rope(k, times, C // heads, time_rotation)
    if num_cls > 0:
        q, k = torch.cat((cq, q), 2), torch.cat((ck, k), 2)
    add = mask[:, None, None, :] + mask[:, None, :, None]
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=add, dropout_p=0.0, is_causal=False)
    return _linear(o.transpose(1, 2).reshape(B, N, C), sd, p + '.proj')


def layer(x, sd, p, mask, times, num_cls, heads, time_rotation):
    """SimpleStaticLayer.forward model.py:278-300."""
    D = x.shape[-1]
    h = F.layer_norm(x, (D,), sd[p + '.norm1.weight'], sd[p + '.norm1.bias'])
    x = attention(h, sd, p + '.attn', mask, times, num_cls, heads, time_rotation) + x
    h = F.layer_norm(x, (D,), sd[p + '.norm2.weight'], sd[p + '.norm2.bias'])
    return _mlp2(h, sd, p + '.mlp1') + x


def _count(sd, prefix):
    n = 0
    while ('%s.%d.norm1.weight' % (prefix, n)) in sd:
        n += 1
    return n


def forward(ball, table, mask, times, sd, heads, time_rotation='new'):
    """MultiStageModel.forward (use_skipconnection=True, mode='dynamic'), model.py:529-571 -> rot (B,3), pos (B,T,3).
    Works in ball.dtype (sd, table and mask must have it); `times` is float32 in either mode (module docstring)."""
    B, T, _ = ball.shape
    dt = ball.dtype
    mask = torch.where(mask == 0, torch.tensor(float('-inf'), dtype=dt), torch.tensor(0.0, dtype=dt))
    x = _mlp2(ball, sd, 'firststage.ball_embed')
    D = x.shape[-1]
    tmask = torch.where(table[:, :, 2] == 1, 0.0, float('-inf')).to(dt)
    tmask = torch.cat((torch.zeros((B, 1), dtype=dt), tmask), 1)
    tmask = tmask[:, None, :].expand(B, T, -1).reshape(B * T, -1)
    N = table.shape[1]
    ttimes = (torch.arange(N, dtype=torch.float32) / (MAX_FPS / 5))[None].expand(B * T, -1)
    tt = _mlp2(table[..., :2], sd, 'firststage.table_embed')
    xx = torch.cat((x.unsqueeze(2), tt.unsqueeze(1).expand(B, T, N, D)), 2).reshape(B * T, N + 1, D)
    for i in range(_count(sd, 'firststage.pos_layers')):
        xx = layer(xx, sd, 'firststage.pos_layers.%d' % i, tmask, ttimes, 1, heads, time_rotation)
    x = xx.reshape(B, T, N + 1, D)[:, :, 0]
    for i in range(_count(sd, 'firststage.layers')):
        x = layer(x, sd, 'firststage.layers.%d' % i, mask, times, 0, heads, time_rotation)
    pos = _head(x, sd, 'firststage.position_head')
    x = x.detach()          # full_backprop is False (model.py:525, :553-555): the spin loss does not reach the first stage
    x = torch.cat((sd['cls_token'].expand(B, 1, D), x), 1)
    m2 = torch.cat((torch.zeros((B, 1), dtype=dt), mask), 1)
    for i in range(_count(sd, 'secondstage')):
        x = layer(x, sd, 'secondstage.%d' % i, m2, times, 1, heads, time_rotation)
    return _head(x[:, 0], sd, 'rotation_head'), pos


def forward_np(sd_np, size, ball, table, mask, times, time_rotation='new', high_precision=False):
    """`forward` under no_grad on numpy inputs -> (rot, pos) numpy, float32, or float64 with high_precision (module docstring)."""
    dt = torch.float64 if high_precision else torch.float32
    sd = {k: torch.tensor(np.asarray(v), dtype=torch.float32).to(dt) for k, v in sd_np.items()}
    ball, table, mask = [torch.as_tensor(np.asarray(a), dtype=torch.float32).to(dt) for a in (ball, table, mask)]
    with torch.no_grad():
        rot, pos = forward(ball, table, mask, torch.as_tensor(np.asarray(times), dtype=torch.float32), sd, SIZES[size][2], time_rotation)
    return rot.numpy(), pos.numpy()


def transform_rotationaxes(rot, pos):
    """uplifting/helper.py:394-420, batched."""
    v0 = torch.zeros((pos.shape[0], 3))
    v0[:, :2] = pos[:, 1, :2] - pos[:, 0, :2]
    ex = v0 / torch.linalg.norm(v0, dim=-1, keepdim=True)
    ez = torch.tensor([0.0, 0.0, 1.0]).expand_as(ex)
    ey = torch.cross(ez, ex, dim=-1)
    return torch.stack([(rot * ex).sum(-1), (rot * ey).sum(-1), (rot * ez).sum(-1)], -1)


def losses(pred_rot, pred_pos, mask, r_world, rotation, transform_mode='global'):
    """train.py:107, :123-127 -> (loss_rot, loss_pos)."""
    if transform_mode == 'local':
        rotation = transform_rotationaxes(rotation, r_world)
    loss_rot = torch.sum(torch.sqrt(torch.sum((pred_rot - rotation) ** 2, dim=1)))
    loss_pos = torch.sum(F.mse_loss(pred_pos, r_world, reduction='none') * mask.unsqueeze(-1)) / torch.sum(mask)
    return loss_rot, loss_pos


def loss_and_grad(sd_np, size, ball, table, mask, times, r_world, rotation, time_rotation='new', transform_mode='global', margins=None):
    """state dict of numpy arrays + numpy inputs -> (loss_rot, loss_pos, {name: gradient or None}, rot, pos), all numpy.
    A tensor the loss does not depend on (`embed.*`) maps to None, as `.grad` does in the reference.
    margins (a list): receives (layer, rows, margin) of every ReLU-input layer (`_relu_linear`, `relu_margin`)."""
    global _margins
    heads = SIZES[size][2]
    sd = {k: torch.tensor(np.asarray(v), dtype=torch.float32, requires_grad=not k.endswith('inv_freq')) for k, v in sd_np.items()}
    ball, table, mask, times, r_world, rotation = [torch.as_tensor(np.asarray(a), dtype=torch.float32) for a in (ball, table, mask, times, r_world, rotation)]
    _margins = margins
    try:
        rot, pos = forward(ball, table, mask, times, sd, heads, time_rotation)
    finally:
        _margins = None
    loss_rot, loss_pos = losses(rot, pos, mask, r_world, rotation, transform_mode)
    (loss_rot + loss_pos).backward()
    grads = {k: (None if v.grad is None else v.grad.numpy()) for k, v in sd.items() if not k.endswith('inv_freq')}
    return loss_rot.item(), loss_pos.item(), grads, rot.detach().numpy(), pos.detach().numpy()
