"""ViTPose's keypoint head (TopdownHeatmapSimpleHead) in training mode on the device, and its backward (csrc/vitpose_head_grad.hip,
DESIGN.md section 29): features in; heatmaps, the eight parameter gradients and the gradient into the features out.

The parameters live in ``.params`` as device tensors under the reference's keys and in the reference's layouts (an optimizer can own
them); the library packs what its kernels read on every ``forward``.  ``forward(train=True)`` normalises with the batch's statistics
over the whole batch and updates ``running_mean`` / ``running_var`` / ``num_batches_tracked`` in place, as ``model.train()`` does;
``train=False`` reads the running statistics.  ``backward`` goes through BN in the mode of the last forward.
"""
import ctypes

import torch

from . import _lib

DIM, DEC = 384, 256
TAPS = {'z1': 1, 'a1': 1, 'z2': 2, 'a2': 2, 'mean1': 0, 'var1': 0, 'mean2': 0, 'var2': 0}          # level: (B, 2^l hp, 2^l wp, 256) NHWC; 0: (256,)


class _Params(ctypes.Structure):          # ttup_vitpose_head_params
    _fields_ = [(n, ctypes.c_void_p) for n in (
        'deconv1_weight', 'bn1_weight', 'bn1_bias', 'bn1_running_mean', 'bn1_running_var', 'bn1_num_batches_tracked',
        'deconv2_weight', 'bn2_weight', 'bn2_bias', 'bn2_running_mean', 'bn2_running_var', 'bn2_num_batches_tracked',
        'final_weight', 'final_bias')]


GRAD_FIELDS = ('deconv1_weight', 'bn1_weight', 'bn1_bias', 'deconv2_weight', 'bn2_weight', 'bn2_bias', 'final_weight', 'final_bias')


class _Grads(ctypes.Structure):           # ttup_vitpose_head_grads
    _fields_ = [(n, ctypes.c_void_p) for n in GRAD_FIELDS + ('feat',)]


def head_keys(prefix='model'):
    """field of the C structs -> the reference's state_dict key"""
    h = prefix + '.keypoint_head.'
    keys = {'final_weight': h + 'final_layer.weight', 'final_bias': h + 'final_layer.bias'}
    for n, i in ((1, 0), (2, 3)):
        keys['deconv%d_weight' % n] = h + 'deconv_layers.%d.weight' % i
        for f, k in (('weight', 'weight'), ('bias', 'bias'), ('running_mean', 'running_mean'), ('running_var', 'running_var'),
                     ('num_batches_tracked', 'num_batches_tracked')):
            keys['bn%d_%s' % (n, f)] = h + 'deconv_layers.%d.%s' % (i + 1, k)
    return keys


def head_shapes(out_ch):
    s = {'final_weight': (out_ch, DEC, 1, 1), 'final_bias': (out_ch,), 'deconv1_weight': (DIM, DEC, 4, 4), 'deconv2_weight': (DEC, DEC, 4, 4)}
    for n in (1, 2):
        for f in ('weight', 'bias', 'running_mean', 'running_var'):
            s['bn%d_%s' % (n, f)] = (DEC,)
        s['bn%d_num_batches_tracked' % n] = ()
    return s


class ViTPoseHead:
    """``state_dict``: the reference's (any superset of the head's keys; ``num_batches_tracked`` may be missing and then starts at 0).
    ``max_rows``: the most tokens (batch * hp * wp) a forward may bring."""

    def __init__(self, state_dict, out_ch, prefix='model', max_rows=8 * 40 * 72, device='cuda:0'):
        self.OUT_CH, self.max_rows = int(out_ch), int(max_rows)
        self._keys = head_keys(prefix)
        shapes = head_shapes(self.OUT_CH)
        if not 1 <= self.OUT_CH <= 16:
            raise ValueError('out_ch %d outside 1..16' % self.OUT_CH)
        for f, k in self._keys.items():
            if k not in state_dict and not f.endswith('num_batches_tracked'):
                raise ValueError('state_dict has no %s' % k)
            if k in state_dict and tuple(state_dict[k].shape) != shapes[f]:
                raise ValueError('%s: expected shape %s, got %s' % (k, shapes[f], tuple(state_dict[k].shape)))
        _lib.require_gpu()
        self.device = torch.device(device)
        self._lib = _lib.load()
        self.params = {}
        for f, k in self._keys.items():
            if f.endswith('num_batches_tracked'):
                v = torch.as_tensor(state_dict.get(k, 0)).to(torch.int64).reshape(())
            else:
                v = torch.as_tensor(state_dict[k]).to(torch.float32)
            self.params[k] = v.detach().to(self.device).clone().contiguous()
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_vitpose_head_create(self.OUT_CH, self.max_rows, ctypes.byref(self._handle))
        _lib.check(rc)
        self._ran = None          # (batch, hp, wp, feat's shape) of the last forward

    def __del__(self):
        h, self._handle = getattr(self, '_handle', None), None
        if h:
            self._lib.ttup_vitpose_head_destroy(h)

    def workspace_bytes(self):
        return self._lib.ttup_vitpose_head_workspace_bytes(self.OUT_CH, self.max_rows)

    def state_dict(self):
        """The head's keys as the reference's ``load_state_dict`` takes them (clones, on the device)."""
        return {k: v.clone() for k, v in self.params.items()}

    def forward(self, feat, grid, train=True):
        """feat: (B*hp*wp, 384) token-major, as ``ViTPoseNet.features`` returns it, or (B, 384, hp, wp) -> heat (B, out_ch, 4hp, 4wp)."""
        hp, wp = int(grid[0]), int(grid[1])
        if hp < 1 or wp < 1:
            raise ValueError('grid %dx%d must be positive' % (hp, wp))
        if not torch.is_tensor(feat) or feat.dim() not in (2, 4):
            raise ValueError('feat must be a (B*hp*wp,384) or (B,384,hp,wp) tensor')
        shape = tuple(feat.shape)
        if feat.dim() == 4:
            if shape[1:] != (DIM, hp, wp) or shape[0] < 1:
                raise ValueError('expected features (B,%d,%d,%d), got %s' % (DIM, hp, wp, shape))
            feat = feat.permute(0, 2, 3, 1).reshape(-1, DIM)
        elif shape[1] != DIM or shape[0] < 1 or shape[0] % (hp * wp):
            raise ValueError('expected features (B*%d,%d), got %s' % (hp * wp, DIM, shape))
        feat = feat.to(self.device, torch.float32).contiguous()
        batch = feat.shape[0] // (hp * wp)
        if feat.shape[0] > self.max_rows:
            raise ValueError('%d rows, the head was sized for %d' % (feat.shape[0], self.max_rows))
        heat = torch.empty((batch, self.OUT_CH, 4 * hp, 4 * wp), dtype=torch.float32, device=self.device)
        p = _Params(**{f: self.params[k].data_ptr() for f, k in self._keys.items()})
        self._ran = None
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_vitpose_head_forward(self._handle, _lib.ptr(feat), batch, hp, wp, ctypes.byref(p), int(bool(train)), _lib.ptr(heat),
                                                     _lib.stream_ptr())
        _lib.check(rc)
        self._ran = (batch, hp, wp, shape)
        return heat

    def backward(self, dheat):
        """dheat (B, out_ch, 4hp, 4wp) of the last forward -> ({reference key: gradient}, dfeat shaped like that forward's feat)."""
        if self._ran is None:
            raise ValueError('backward without a preceding forward')
        batch, hp, wp, shape = self._ran
        if not torch.is_tensor(dheat) or tuple(dheat.shape) != (batch, self.OUT_CH, 4 * hp, 4 * wp):
            raise ValueError('expected dheat (%d,%d,%d,%d) as the forward returned, got %s'
                             % (batch, self.OUT_CH, 4 * hp, 4 * wp, tuple(dheat.shape) if torch.is_tensor(dheat) else type(dheat)))
        dheat = dheat.to(self.device, torch.float32).contiguous()
        shapes = head_shapes(self.OUT_CH)
        out = {f: torch.empty(shapes[f], dtype=torch.float32, device=self.device) for f in GRAD_FIELDS}
        dfeat = torch.empty((batch * hp * wp, DIM), dtype=torch.float32, device=self.device)
        g = _Grads(feat=dfeat.data_ptr(), **{f: t.data_ptr() for f, t in out.items()})
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_vitpose_head_backward(self._handle, _lib.ptr(dheat), batch, hp, wp, ctypes.byref(g), _lib.stream_ptr())
        _lib.check(rc)
        if len(shape) == 4:
            dfeat = dfeat.view(batch, hp, wp, DIM).permute(0, 3, 1, 2).contiguous()
        return {self._keys[f]: t for f, t in out.items()}, dfeat

    def read_tap(self, name):
        """What the last forward kept: 'z1', 'a1' (B, 2hp, 2wp, 256) and 'z2', 'a2' (B, 4hp, 4wp, 256) NHWC; 'mean1', 'var1', 'mean2',
        'var2' (256,): the statistics the BN used."""
        if name not in TAPS:
            raise ValueError('unknown tap %r (one of %s)' % (name, ', '.join(sorted(TAPS))))
        if self._ran is None:
            raise ValueError('read_tap without a preceding forward')
        batch, hp, wp, _ = self._ran
        lvl = TAPS[name]
        shape = (batch, hp << lvl, wp << lvl, DEC) if lvl else (DEC,)
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_vitpose_head_read_tap(self._handle, name.encode(), _lib.ptr(out), out.numel() * 4)
        _lib.check(rc)
        return out
