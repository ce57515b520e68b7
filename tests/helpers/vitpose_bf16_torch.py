"""The rounding oracle of the bf16 ViTPose path: tests/helpers/vitpose_torch.py's forward with the rounding points of the arithmetic
contract, in fp64 or fp32 arithmetic, step by step so that every stored tensor ("tap") of csrc/vitpose.hip's
bf16 path has its counterpart and any step can be evaluated from a given input (teacher forcing).

Rounding is fp32 -> bf16, round to nearest even (`rne`).  Rounded once: the matrix weights (patch embedding, qkv, proj, fc1, fc2 and
the two BN-folded deconvolutions: weights.vitpose_fold_head first, then rounded).  Stored as bf16: the patch operand, the LN outputs,
qkv after bias, the attention output, fc1's output after GELU, last_norm's output and both deconvolution outputs.  fp32 on the
device (the arithmetic dtype here): biases, LN parameters, pos_embed, the final 1x1 conv, the residual stream, accumulation and the
softmax; the LayerNorms themselves run in fp64 on the device.  The attention keeps P UNROUNDED (the device feeds the softmax
numerators to P V as two bf16 operands, 16 significant bits): `Oracle.att` also returns sum_j p_j |v_j| / l, which the test's bound
on the attention output is stated in.

With `rounding=False` no value is rounded and the head runs as ConvTranspose2d + BatchNorm like vitpose_torch.forward (the folded
weights are themselves rounded to fp32, which would show at 1e-7): then `forward` is vitpose_torch.forward to fp64 round-off."""
import torch
import torch.nn.functional as F

from helpers import vitpose_torch
from upliftingtabletennis_amd import weights

DIM, HEADS, DEPTH = weights.VITPOSE_DIM, weights.VITPOSE_HEADS, weights.VITPOSE_DEPTH
BLOCK_TAPS = ('qkv', 'att', 'x_attn', 'hid', 'x')
HEAD_TAPS = ('ln', 'd1', 'd2', 'heat')
BF16_TAPS = ('qkv', 'att', 'hid', 'ln', 'd1', 'd2')          # stored as bf16; 'x', 'x_attn' and 'heat' are fp32


def rne(t):
    """fp32 -> bf16 round to nearest even, back in t's dtype (an fp64 value goes through fp32 first, as it would on the device)."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


class Oracle:
    def __init__(self, sd, dtype=torch.float64, rounding=True, prefix='model'):
        self.sd, self.dtype, self.rounding, self.prefix = sd, dtype, rounding, prefix
        self.fold = weights.vitpose_fold_head(sd, prefix) if rounding else None

    def t(self, k):
        return torch.as_tensor(self.sd[self.prefix + '.' + k]).to(self.dtype)

    def r(self, t):
        return rne(t) if self.rounding else t

    def w(self, k):
        """A matrix weight: rounded once."""
        return self.r(self.t(k))

    def _ln(self, y, k):
        return self.r(F.layer_norm(y, (DIM,), self.t(k + '.weight'), self.t(k + '.bias'), eps=1e-6))

    # ---- stage 0
    def patch(self, x):
        """x (B, in_ch, H, W) -> the residual stream (B * tokens, 384)."""
        x = self.r(torch.as_tensor(x).to(self.dtype))
        y = F.conv2d(x, self.w('backbone.patch_embed.proj.weight'), self.t('backbone.patch_embed.proj.bias'), stride=16, padding=2)
        y = y.flatten(2).transpose(1, 2)
        pos = self.t('backbone.pos_embed')
        return (y + pos[:, 1:] + pos[:, :1]).reshape(-1, DIM)

    # ---- stages 1..12, step by step: each takes what the device has stored before it
    def qkv(self, i, y):
        p = 'backbone.blocks.%d.' % i
        return self.r(F.linear(self._ln(y, p + 'norm1'), self.w(p + 'attn.qkv.weight'), self.t(p + 'attn.qkv.bias')))

    def att(self, qkv, batch):
        """Stored qkv (B * T, 1152) -> (att rounded, att before its rounding, sum_j p_j |v_j| / l), each (B * T, 384)."""
        q, k, v = qkv.reshape(batch, -1, 3, HEADS, DIM // HEADS).permute(2, 0, 3, 1, 4)
        a = ((q @ k.transpose(-2, -1)) * (DIM // HEADS) ** -0.5).softmax(-1)
        flat = lambda o: o.transpose(1, 2).reshape(-1, DIM)      # noqa: E731
        raw = flat(a @ v)
        return self.r(raw), raw, flat(a @ v.abs())

    def proj(self, i, att, y):
        p = 'backbone.blocks.%d.' % i
        return y + F.linear(att, self.w(p + 'attn.proj.weight'), self.t(p + 'attn.proj.bias'))

    def fc1(self, i, x_attn):
        p = 'backbone.blocks.%d.' % i
        return self.r(F.gelu(F.linear(self._ln(x_attn, p + 'norm2'), self.w(p + 'mlp.fc1.weight'), self.t(p + 'mlp.fc1.bias'))))

    def fc2(self, i, hid, x_attn):
        p = 'backbone.blocks.%d.' % i
        return x_attn + F.linear(hid, self.w(p + 'mlp.fc2.weight'), self.t(p + 'mlp.fc2.bias'))

    def block(self, i, y, batch):
        """Block i on the residual stream y -> its taps (and 'att_raw', 'att_pabs')."""
        o = {'qkv': self.qkv(i, y)}
        o['att'], o['att_raw'], o['att_pabs'] = self.att(o['qkv'], batch)
        o['x_attn'] = self.proj(i, o['att'], y)
        o['hid'] = self.fc1(i, o['x_attn'])
        o['x'] = self.fc2(i, o['hid'], o['x_attn'])
        return o

    # ---- stage 13.  ln is (B * T, 384); d1 / d2 are NHWC (B, 2hp, 2wp, 256) / (B, 4hp, 4wp, 256) as the device stores them
    def ln(self, y):
        return self._ln(y, 'backbone.last_norm')

    def deconv(self, layer, inp, batch, hp, wp):
        """Deconvolution `layer` (0 or 1) + BN + ReLU on its NHWC input (the ln tap for layer 0) -> NHWC."""
        h, w = hp << layer, wp << layer
        y = inp.reshape(batch, h, w, -1).permute(0, 3, 1, 2)
        if self.rounding:
            wf, b = self.fold[layer]
            y = self.r(vitpose_torch.deconv_folded(y, self.r(torch.as_tensor(wf).to(self.dtype)), b))
        else:
            p, i = 'keypoint_head.deconv_layers.', 3 * layer
            y = F.conv_transpose2d(y, self.t(p + '%d.weight' % i), stride=2, padding=1)
            y = F.relu(F.batch_norm(y, self.t(p + '%d.running_mean' % (i + 1)), self.t(p + '%d.running_var' % (i + 1)), self.t(p + '%d.weight' % (i + 1)),
                                    self.t(p + '%d.bias' % (i + 1)), training=False, eps=1e-5))
        return y.permute(0, 2, 3, 1).contiguous()

    def final(self, d2):
        """NHWC d2 -> the heatmap (B, out_ch, 4hp, 4wp): fp32 on the device, never rounded."""
        return F.conv2d(d2.permute(0, 3, 1, 2), self.t('keypoint_head.final_layer.weight'), self.t('keypoint_head.final_layer.bias'))

    def head(self, y, batch, hp, wp):
        o = {'ln': self.ln(y)}
        o['d1'] = self.deconv(0, o['ln'], batch, hp, wp)
        o['d2'] = self.deconv(1, o['d1'], batch, hp, wp)
        o['heat'] = self.final(o['d2'])
        return o

    def forward(self, x):
        """-> the taps of every stage: [{'x'}, 12 x block taps, head taps]; each stage's input is the 'x' of the one before."""
        x = torch.as_tensor(x)
        batch, hp, wp = x.shape[0], x.shape[2] // 16, x.shape[3] // 16
        with torch.no_grad():
            out = [{'x': self.patch(x)}]
            for i in range(DEPTH):
                out.append(self.block(i, out[-1]['x'], batch))
            out.append(self.head(out[-1]['x'], batch, hp, wp))
        return out
