"""Oracle (a2, bf16 path): the WASB / HRNet graph of ``oracle/wasb_ref.py`` in float64 on the CPU, cut into five segments and
rounded to bf16 (round to nearest even) exactly where the device's bf16 graph stores or re-reads a bf16 value -- and nowhere else.

A segment starts from given input tensors (the device's own taps, which are exact bf16 values) and returns its output taps, so a
test can compare every fused kernel with its own layers and a kernel's rounding never leaks into the next segment:

    S0  input (B,C,H,W)            -> stem2, bneck_a1 (Bottleneck conv1's output, which the device keeps for the next kernel)
    S1  stem2                      -> trans1_0, trans1_1          (Bottleneck with its two-source 1x1 conv, transition1)
        (S0 and S1 also return stem1 and layer1, which only the layer-by-layer plan stores)
    S2  trans1_0, trans1_1         -> stage2_0, stage2_1          (HR module of stage 2 with its fuse layer)
    S3  stage2_0, stage2_1         -> stage3_0, stage3_1, stage3_2  (transition2, HR module, fuse layer)
    S4  stage3_0 .. stage3_2       -> heat (and stage4_0 where the graph stores it)  (transition3, HR module, fuse output 0, head)

Rounding points, each with the file that fixes it (csrc = upliftingtabletennis_amd/csrc):

  weights    BatchNorm folded in double and stored as float (csrc/wasb_blob.h parse_blob), then rounded to bf16 when packed
             (csrc/conv.hip pack_conv).  Biases stay float; the two-source conv adds its two biases in float (pack_conv).  The head's
             weights and bias stay float (csrc/wasb_net.hip head_w_dev, csrc/chain16.h hw4, csrc/conv_pointwise.h head_kernel).
  input      rounded when it is laid out as NHWC16 (csrc/conv_pointwise.h nchw_to_nhwc_kernel) or as per-frame records
             (preprocess_kernel / preprocess_frames4_kernel, pack2): the same values.
  stem       conv1 + ReLU rounded into LDS (csrc/conv_stem.h, pack8 into s_t1), conv2 + ReLU rounded (stem2, the T2 store), the
             1x1 follower reads those rounded pairs and its output + ReLU is rounded (A1 store).  TTUP_NO_STEM: the same points in
             csrc/conv_mfma.h (epilogue, F11 follower).
  Bottleneck conv2 3x3 32 -> 32 + ReLU rounded (csrc/conv_mfma.h epilogue).  conv3 + downsample + both biases is ONE accumulator
             (K = 32 + 64): the 128-channel pre-activation is never rounded; after the ReLU it is rounded into LDS
             (csrc/conv_bneck.h phase 1; layer-wise: csrc/conv_mfma.h).  transition1's two convs + ReLU rounded (phases 2a, 2b).
  BasicBlock conv1 + ReLU rounded, conv2 + block input + ReLU rounded: csrc/conv_bb.h bb_conv (epi), csrc/chain16.h
             (c16_conv_lds, c16_conv_out), csrc/conv64.h (epilogue pass 1), csrc/conv_mfma.h (residual in the epilogue).
  1x1 fuse   conv on the rounded branch output, no ReLU, rounded: csrc/conv_bb.h (follower of the 32-channel block),
             csrc/conv64.h (lin16 / lin32 followers), csrc/conv_mfma.h (stand-alone 1x1).
  fuse i=0   relu(bf16(x_0) + upsampled terms) rounded once: csrc/chain16.h MODE 1..3 starts "from the ROUNDED branch output",
             csrc/conv_pointwise.h upsum_bf16x8_kernel reads it back from memory.  Both models are the same here.
  fuse i>0   stride-2 chains: every conv but the last + ReLU rounded.  `layerwise`: the last conv of each chain (+ the running sum
             of the earlier chains) is rounded WITHOUT ReLU (csrc/conv_mfma.h epilogue, residual), then UPSUM rounds
             relu(that + x_i + upsampled terms) (csrc/conv_pointwise.h).  `fused`: the last chain's last conv keeps its float
             accumulator, adds the running sum, x_i and the upsampled term, and rounds ONCE after the ReLU (csrc/conv_mfma.h
             res2 / res3, conv_s2_pair_kernel; planned in csrc/wasb_graph.h finish_sum when at most two terms join).
  head       `layerwise` (TTUP_NO_FUSE, TTUP_NO_FUSE_SUM, and every multi-map head): stage4_0 = relu(bf16(x_0) + terms) rounded
             (csrc/conv_pointwise.h upsum / csrc/refine.hip upsum_head_kernel / csrc/chain16.h MODE 3), head on the rounded values.
             `fused` (one map, default): neither branch 0's last block output nor the sum is stored, so neither is rounded -- the
             head sees relu(relu(conv + block input) + terms) in float (csrc/chain16.h MODE 7, csrc/conv_bb.h exact_tail).
  heat       float, never rounded.

`run_segment(..., variant='f32r')` is the fp32 accumulation variant: the same segment with every conv's operands cast to float32
and its input channels reversed (any fp32 summation order is a legitimate sample).  It measures how much disagreement rounding
flips alone produce; the float64 evaluation is the reference.  variant='f32' is the same with K as stored: a second draw, used
to see how far two legitimate orders differ from each other.

fp32 storage (`Weights(rounding='f32')`, tests/test_wasb_f32_taps_gpu.py): the fp32 net's numbers in float64.  The folded weights
and biases are rounded to float32 once, as csrc/wasb_blob.h stores them, the two-source conv adds its two biases in float
(pack_conv), the head keeps its float weights -- and no activation is ever rounded.  The fp32 graph is the layer-by-layer one
(csrc/wasb_graph.h builds fused ops for bf16 only), so the model is 'layerwise' and stage4_0 is a tap; without activation rounding
the two models compute the same values.  The 'f32r' / 'f32' variants are then two fp32 evaluations of the same segment.

Nothing here comes from the reference project: it is this project's graph (csrc/wasb_graph.h) with rounding added.
"""
import torch
import torch.nn.functional as F

from oracle.wasb_ref import BLOCKS_PER_BRANCH, BN_EPS

MODELS = ('fused', 'layerwise')
SEGMENTS = {          # name: (input taps, output taps; stage4_0 only where the model rounds it)
    'S0': (('input',), ('stem1', 'stem2', 'bneck_a1')),
    'S1': (('stem2',), ('layer1', 'trans1_0', 'trans1_1')),
    'S2': (('trans1_0', 'trans1_1'), ('stage2_0', 'stage2_1')),
    'S3': (('stage2_0', 'stage2_1'), ('stage3_0', 'stage3_1', 'stage3_2')),
    'S4': (('stage3_0', 'stage3_1', 'stage3_2'), ('stage4_0', 'heat')),
}


def bf16_round(x):
    """Round to the nearest bf16 value, ties to even; float64 (or float32) in, float64 out.  bf16 is float32's exponent with 8
    significant bits: subnormals below 2^-126 are multiples of 2^-133, anything that rounds to 2^128 is infinite."""
    x = torch.as_tensor(x).double().contiguous()
    a = x.abs()
    if bool(((a >= 2.0 ** -126) & (a < 2.0 ** 127) | (a == 0)).all()):
        # zeros and bf16-normal values (every activation): round the float64 pattern at its 8th significant bit -- add half a step
        # less one, plus the kept part's last bit, and clear the 45 dropped bits (a carry moves into the exponent as it should)
        u = x.view(torch.int64)
        return ((u + (0x0FFFFFFFFFFF + ((u >> 45) & 1))) & ~((1 << 45) - 1)).view(torch.float64)
    _, e = torch.frexp(x)                                   # |x| = m * 2^e, 0.5 <= m < 1
    q = torch.ldexp(torch.ones_like(x), e.clamp(min=-125) - 8)
    y = torch.round(x / q) * q                              # (torch.round: half to even; x / q is exact)
    y = torch.where(y.abs() >= 2.0 ** 128, torch.copysign(torch.full_like(y, float('inf')), y), y)
    return torch.where(torch.isfinite(x), y, x)


def _identity(x):
    return x


class Weights:
    """The convs of a reference-format state dict with eval-mode BatchNorm folded in (an already folded dict -- conv weights and
    biases, no BatchNorm keys -- is taken as it is).  rounding=True: stored as the device's bf16 net stores them (see the module
    docstring); rounding=False: float64 throughout, for the comparison with oracle/wasb_ref.py; rounding='f32': stored as the
    device's fp32 net stores them -- folded in double, rounded to float32 once -- with activations never rounded."""

    def __init__(self, state_dict, prefix='model', rounding=True):
        assert rounding in (True, False, 'f32'), rounding
        self.sd, self.p, self.rounding = state_dict, prefix, rounding
        self.round_activations = rounding is True
        self._cache = {}

    def _t(self, key):
        v = self.sd[key]
        return (v if isinstance(v, torch.Tensor) else torch.as_tensor(v)).double()

    def conv(self, conv, bn):
        """(weight (cout, cin, k, k), bias (cout,)) of `prefix.conv` with `prefix.bn` folded, float64 tensors."""
        key = (conv, bn)
        if key not in self._cache:
            c, n = '%s.%s' % (self.p, conv), '%s.%s' % (self.p, bn)
            w = self._t(c + '.weight')
            b = self._t(c + '.bias') if c + '.bias' in self.sd else torch.zeros(w.shape[0], dtype=torch.float64)
            if n + '.weight' in self.sd:
                s = self._t(n + '.weight') / torch.sqrt(self._t(n + '.running_var') + BN_EPS)
                w = w * s.view(-1, 1, 1, 1)
                b = (b - self._t(n + '.running_mean')) * s + self._t(n + '.bias')
            if self.rounding == 'f32':
                w, b = w.float().double(), b.float().double()
            elif self.rounding:
                w, b = bf16_round(w.float()), b.float().double()
            self._cache[key] = (w, b)
        return self._cache[key]

    def head(self):
        w, b = self._t(self.p + '.final_layers.0.weight'), self._t(self.p + '.final_layers.0.bias')
        if w.shape[0] == 3:          # the ball detector keeps the middle one of its three maps
            w, b = w[1:2], b[1:2]
        if self.rounding == 'f32':
            w, b = w.float().double(), b.float().double()
        return w, b


class _Eval:
    def __init__(self, weights, model, variant):
        assert model in MODELS and variant in ('f64', 'f32r', 'f32'), (model, variant)
        self.w, self.fused, self.f32, self.flip = weights, model == 'fused', variant != 'f64', variant == 'f32r'
        self.rnd = bf16_round if weights.round_activations else _identity

    def up(self, v):          # the working precision
        return v.float() if self.f32 else v.double()

    def mac(self, x, w, stride=1):
        if self.flip:
            return F.conv2d(x.float().flip(1), w.float().flip(1), None, stride, w.shape[-1] // 2)
        if self.f32:
            return F.conv2d(x.float(), w.float(), None, stride, w.shape[-1] // 2)
        return F.conv2d(x.double(), w, None, stride, w.shape[-1] // 2)

    def cb(self, x, conv, bn, stride=1, relu=False, add=(), rnd=True):
        """round(relu(conv(x) + bias + the `add` terms)): one accumulator, one rounding."""
        w, b = self.w.conv(conv, bn)
        y = self.mac(x, w, stride) + self.up(b).view(1, -1, 1, 1)
        for t in add:
            y = y + self.up(t)
        if relu:
            y = F.relu(y)
        return self.rnd(y) if rnd else y

    # ---- segments
    def s0(self, x):
        x = self.rnd(torch.as_tensor(x))
        t1 = self.cb(x, 'conv1', 'bn1', relu=True)
        stem2 = self.cb(t1, 'conv2', 'bn2', relu=True)
        return {'stem1': t1, 'stem2': stem2, 'bneck_a1': self.cb(stem2, 'layer1.0.conv1', 'layer1.0.bn1', relu=True)}

    def s1(self, stem2):
        a1 = self.cb(stem2, 'layer1.0.conv1', 'layer1.0.bn1', relu=True)
        a2 = self.cb(a1, 'layer1.0.conv2', 'layer1.0.bn2', relu=True)
        w3, b3 = self.w.conv('layer1.0.conv3', 'layer1.0.bn3')
        wd, bd = self.w.conv('layer1.0.downsample.0', 'layer1.0.downsample.1')
        bias = (b3.float() + bd.float()).double() if self.w.rounding else b3 + bd
        y = self.mac(a2, w3) + self.mac(stem2, wd) + self.up(bias).view(1, -1, 1, 1)
        layer1 = self.rnd(F.relu(y))
        return {'layer1': layer1,
                'trans1_0': self.cb(layer1, 'transition1.0.0', 'transition1.0.1', relu=True),
                'trans1_1': self.cb(layer1, 'transition1.1.0.0', 'transition1.1.0.1', stride=2, relu=True)}

    def hr_module(self, xs, p, n_out, exact_tail=False):
        """HighResolutionModule.forward (wasb_ref.hr_module) with the device's rounding; fused outputs 0 .. n_out-1.
        exact_tail: output 0 and the branch-0 tensor it starts from stay unrounded (the fused head)."""
        nb, xs = len(xs), list(xs)
        for b in range(nb):
            for k in range(BLOCKS_PER_BRANCH):
                q = '%s.branches.%d.%d' % (p, b, k)
                t = self.cb(xs[b], q + '.conv1', q + '.bn1', relu=True)
                keep = exact_tail and b == 0 and k == BLOCKS_PER_BRANCH - 1
                xs[b] = self.cb(t, q + '.conv2', q + '.bn2', relu=True, add=(xs[b],), rnd=not keep)
        outs = []
        for i in range(n_out):
            ups = []
            for j in range(i + 1, nb):          # 1x1 conv + BN at the low resolution, nearest upsampling when summed
                q = '%s.fuse_layers.%d.%d' % (p, i, j)
                t = self.cb(xs[j], q + '.0', q + '.1')
                ups.append(t.repeat_interleave(2 ** (j - i), 2).repeat_interleave(2 ** (j - i), 3))
            if i == 0:
                y = self.up(xs[0])
                for t in ups:
                    y = y + self.up(t)
                y = F.relu(y)
                outs.append(y if exact_tail else self.rnd(y))
                continue
            terms = [xs[i]] + ups
            in_epilogue = self.fused and len(terms) <= 2          # csrc/wasb_graph.h finish_sum
            acc, done = None, None
            for j in range(i):
                y = xs[j]
                for k in range(i - j):
                    q = '%s.fuse_layers.%d.%d.%d' % (p, i, j, k)
                    if k != i - j - 1:
                        y = self.cb(y, q + '.0', q + '.1', stride=2, relu=True)
                    elif in_epilogue and j == i - 1:
                        done = self.cb(y, q + '.0', q + '.1', stride=2, relu=True, add=([] if acc is None else [acc]) + terms)
                    else:
                        acc = self.cb(y, q + '.0', q + '.1', stride=2, add=[] if acc is None else [acc])
            if done is None:
                y = self.up(acc)
                for t in terms:
                    y = y + self.up(t)
                done = self.rnd(F.relu(y))
            outs.append(done)
        return outs

    def s2(self, t0, t1):
        ys = self.hr_module([t0, t1], 'stage2.0', 2)
        return {'stage2_0': ys[0], 'stage2_1': ys[1]}

    def s3(self, y0, y1):
        xs = [y0, y1, self.cb(y1, 'transition2.2.0.0', 'transition2.2.0.1', stride=2, relu=True)]
        ys = self.hr_module(xs, 'stage3.0', 3)
        return {'stage3_0': ys[0], 'stage3_1': ys[1], 'stage3_2': ys[2]}

    def s4(self, y0, y1, y2):
        xs = [y0, y1, y2, self.cb(y2, 'transition3.3.0.0', 'transition3.3.0.1', stride=2, relu=True)]
        w, b = self.w.head()
        exact = self.fused and w.shape[0] == 1          # csrc/wasb_graph.h head_in_chain
        y = self.hr_module(xs, 'stage4.0', 1, exact_tail=exact)[0]
        out = {} if exact else {'stage4_0': y}
        hy = self.up(y)
        out['heat'] = F.conv2d(hy, w.to(hy.dtype), b.to(hy.dtype)).double()
        return out


def run_segment(seg, inputs, weights, model='fused', variant='f64'):
    """Output taps {name: float64 (B,C,h,w)} of segment `seg` from `inputs` {name: tensor} (SEGMENTS[seg][0]).  model: 'fused' (the
    default plan) or 'layerwise' (TTUP_NO_FUSE); variant: 'f64' (the reference) or 'f32r' (fp32 accumulation, reversed K)."""
    ev = _Eval(weights, model, variant)
    args = [torch.as_tensor(inputs[k]) for k in SEGMENTS[seg][0]]
    with torch.no_grad():
        out = getattr(ev, seg.lower())(*args)
    return {k: v.double() for k, v in out.items()}


def run_all(x, weights, model='fused', variant='f64'):
    """S0 .. S4 chained on the oracle's own taps: every tap and the heatmap."""
    taps = {'input': torch.as_tensor(x)}
    for seg in SEGMENTS:
        taps.update(run_segment(seg, taps, weights, model, variant))
    return taps
