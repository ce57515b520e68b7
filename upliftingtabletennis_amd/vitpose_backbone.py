"""The ViTPose-small backbone in training mode on the device, and its backward (csrc/vitpose_grad.hip): images
in, last_norm's output out, then the gradient into that output in and the gradients of the 149 backbone tensors out.

The parameters live in ``.params`` as device tensors under the reference's keys and in the reference's layouts (an optimizer can own
them).  ``forward(x, drop_scale)`` keeps every block's activations; ``drop_scale`` (12, 2, B) is the factor on each residual branch
of each sample -- the reference's stochastic depth (``drop_path_rate=0.3`` spread as ``linspace(0, 0.3, 12)``, vit.py:295, :203-204)
multiplies a branch by 0 or 1/keep per sample.  ``None`` is the backbone in ``eval()``: then ``feat`` is ``ViTPoseNet.features``
bit for bit.  ``sample_drop_scale`` draws such scales on the host; it follows the reference's rule, not its random stream (the
reference draws with ``bernoulli_`` on the training device, once per branch), so a run is reproducible here but not bit-comparable
with a reference run of the same seed.
"""
import ctypes

import torch

from . import _lib

DIM, MLP, DEPTH, TENSORS = 384, 1536, 12, 149
TAPS = {'x': (DIM, 12), 'x_mid': (DIM, 11), 'att': (DIM, 11), 'qkv': (3 * DIM, 11), 'lse': (12, 11), 'pre': (MLP, 11), 'dqkv': (3 * DIM, 0)}   # columns, last block
_BLOCK = (('norm1.weight', (DIM,)), ('norm1.bias', (DIM,)), ('attn.qkv.weight', (3 * DIM, DIM)), ('attn.qkv.bias', (3 * DIM,)),
          ('attn.proj.weight', (DIM, DIM)), ('attn.proj.bias', (DIM,)), ('norm2.weight', (DIM,)), ('norm2.bias', (DIM,)),
          ('mlp.fc1.weight', (MLP, DIM)), ('mlp.fc1.bias', (MLP,)), ('mlp.fc2.weight', (DIM, MLP)), ('mlp.fc2.bias', (DIM,)))


class _Ptrs(ctypes.Structure):            # ttup_vitpose_backbone_params / ttup_vitpose_backbone_grads
    _fields_ = [('t', ctypes.c_void_p * TENSORS)]


def backbone_shapes(in_ch, tokens):
    """[(key suffix behind '<prefix>.backbone.', shape)] of the 149 tensors in the reference's state_dict order: csrc/vitpose_grad_plan.h's
    gradient table (tests/test_vitpose_grad_plan_host.py holds the two together)."""
    out = [('pos_embed', (1, tokens + 1, DIM)), ('patch_embed.proj.weight', (DIM, in_ch, 16, 16)), ('patch_embed.proj.bias', (DIM,))]
    for i in range(DEPTH):
        out += [('blocks.%d.%s' % (i, k), s) for k, s in _BLOCK]
    return out + [('last_norm.weight', (DIM,)), ('last_norm.bias', (DIM,))]


def keep_probabilities(rate=0.3):
    """keep_i = 1 - rate * i / 11, the reference's linspace(0, rate, 12)"""
    return [1.0 - rate * i / (DEPTH - 1) for i in range(DEPTH)]


def sample_drop_scale(batch, rate=0.3, generator=None):
    """(12, 2, batch) float32 on the host: entry (i, half, b) is 0 with probability rate * i / 11, else 1 / keep_i; block 0 is all ones.
    Draws from ``generator`` (a torch.Generator) or torch's global one -- the reference's rule, not its random stream."""
    keep = torch.tensor(keep_probabilities(rate), dtype=torch.float64).view(DEPTH, 1, 1).expand(DEPTH, 2, int(batch))
    kept = torch.rand((DEPTH, 2, int(batch)), dtype=torch.float64, generator=generator) < keep
    return torch.where(kept, 1.0 / keep, torch.zeros((), dtype=torch.float64)).to(torch.float32)


class ViTPoseBackbone:
    """``state_dict``: the reference's (any superset of the backbone's keys).  ``resolution`` is (W, H), both multiples of 16."""

    def __init__(self, state_dict, in_ch, resolution, prefix='model', max_batch=8, device='cuda:0'):
        self.W, self.H = int(resolution[0]), int(resolution[1])
        self.IN_CH, self.max_batch = int(in_ch), int(max_batch)
        if self.W < 16 or self.H < 16 or self.W % 16 or self.H % 16:
            raise ValueError('resolution %dx%d: width and height must be positive multiples of 16' % (self.W, self.H))
        self.hp, self.wp = self.H // 16, self.W // 16
        self.tokens = self.hp * self.wp
        self._shapes = [(prefix + '.backbone.' + k, s) for k, s in backbone_shapes(self.IN_CH, self.tokens)]
        for k, s in self._shapes:
            if k not in state_dict:
                raise ValueError('state_dict has no %s' % k)
            if tuple(state_dict[k].shape) != s:
                raise ValueError('%s: expected shape %s, got %s' % (k, s, tuple(state_dict[k].shape)))
        _lib.require_gpu()
        self.device = torch.device(device)
        self._lib = _lib.load()
        self.params = {k: torch.as_tensor(state_dict[k]).to(torch.float32).detach().to(self.device).clone().contiguous() for k, _ in self._shapes}
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_vitpose_grad_create(self.IN_CH, self.hp, self.wp, self.max_batch, ctypes.byref(self._handle))
        _lib.check(rc)
        self._ran = None          # the batch of the last forward

    def __del__(self):
        h, self._handle = getattr(self, '_handle', None), None
        if h:
            self._lib.ttup_vitpose_grad_destroy(h)

    def workspace_bytes(self):
        return self._lib.ttup_vitpose_grad_workspace_bytes(self.IN_CH, self.hp, self.wp, self.max_batch)

    def state_dict(self):
        """The backbone's keys as the reference's ``load_state_dict`` takes them (clones, on the device)."""
        return {k: v.clone() for k, v in self.params.items()}

    def _param_ptrs(self):
        return _Ptrs((ctypes.c_void_p * TENSORS)(*[self.params[k].data_ptr() for k, _ in self._shapes]))

    def forward(self, x, drop_scale=None):
        """x (B, in_ch, H, W) float, B <= max_batch; drop_scale None or (12, 2, B) -> feat (B * tokens, 384) float32, last_norm's output."""
        if not torch.is_tensor(x) or x.dim() != 4 or tuple(x.shape[1:]) != (self.IN_CH, self.H, self.W) or not 1 <= x.shape[0] <= self.max_batch:
            raise ValueError('expected input (1..%d,%d,%d,%d), got %s' % (self.max_batch, self.IN_CH, self.H, self.W, tuple(x.shape) if torch.is_tensor(x) else type(x)))
        batch = x.shape[0]
        x = x.to(self.device, torch.float32).contiguous()
        if drop_scale is not None:
            drop_scale = torch.as_tensor(drop_scale)
            if tuple(drop_scale.shape) != (DEPTH, 2, batch):
                raise ValueError('drop_scale must be (12, 2, %d), got %s' % (batch, tuple(drop_scale.shape)))
            drop_scale = drop_scale.to(self.device, torch.float32).contiguous()
        feat = torch.empty((batch * self.tokens, DIM), dtype=torch.float32, device=self.device)
        p = self._param_ptrs()
        self._ran = None
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_vitpose_grad_forward(self._handle, _lib.ptr(x), batch, ctypes.byref(p), _lib.ptr(drop_scale),
                                                     0 if drop_scale is None else drop_scale.numel(), _lib.ptr(feat), _lib.stream_ptr())
        _lib.check(rc)
        self._ran = batch
        return feat

    def backward(self, dfeat):
        """dfeat (B * tokens, 384) of the last forward -> {reference key: gradient} of the 149 tensors (views of one flat buffer, in
        the reference's order).  The gradient into the images is not computed."""
        if self._ran is None:
            raise ValueError('backward without a preceding forward')
        batch = self._ran
        if not torch.is_tensor(dfeat) or tuple(dfeat.shape) != (batch * self.tokens, DIM):
            raise ValueError('expected dfeat (%d,%d) as the forward returned, got %s'
                             % (batch * self.tokens, DIM, tuple(dfeat.shape) if torch.is_tensor(dfeat) else type(dfeat)))
        dfeat = dfeat.to(self.device, torch.float32).contiguous()
        counts = [int(torch.Size(s).numel()) for _, s in self._shapes]
        flat = torch.empty((sum(counts),), dtype=torch.float32, device=self.device)
        out, off = {}, 0
        for (k, s), n in zip(self._shapes, counts):
            out[k] = flat[off:off + n].view(s)
            off += n
        p = self._param_ptrs()
        g = _Ptrs((ctypes.c_void_p * TENSORS)(*[out[k].data_ptr() for k, _ in self._shapes]))
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_vitpose_grad_backward(self._handle, _lib.ptr(dfeat), batch, ctypes.byref(p), ctypes.byref(g), _lib.stream_ptr())
        _lib.check(rc)
        return out

    def read_tap(self, name, block=0):
        """What the last forward kept of block `block`: 'x' (0..12: the stream entering the block; 12: what last_norm reads), 'x_mid',
        'att' (rows, 384), 'qkv' (rows, 1152), 'lse' (rows, 12), 'pre' (rows, 1536); and 'dqkv' (rows, 1152) of block 0 after a backward."""
        if name not in TAPS:
            raise ValueError('unknown tap %r (one of %s)' % (name, ', '.join(sorted(TAPS))))
        if self._ran is None:
            raise ValueError('read_tap without a preceding forward')
        out = torch.empty((self._ran * self.tokens, TAPS[name][0]), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_vitpose_grad_read_tap(self._handle, name.encode(), int(block), _lib.ptr(out), out.numel() * 4)
        _lib.check(rc)
        return out
