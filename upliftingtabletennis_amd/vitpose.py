"""ViTPose-small detector behind ``self.model(x)`` for model_name 'vitpose' (balldetection/models/vitpose.py,
tabledetection/models/vitpose.py; factories balldetection/train.py:263-265, tabledetection/train.py:218-220).

The forward runs in libttup.so (csrc/vitpose.hip), in fp32 arithmetic by default or, with ``dtype='bf16'``, on the bf16 matrix pipe
under the rounding contract of DESIGN.md section 24 (an uncertified detector for the hub's aux slot); this class only owns the handle
and the torch-side buffers.
``forward(x) -> (heatmaps (B, C_out, H/4, W/4) float32, None)``, as the reference wrapper returns ``(seg_out, None)``.
``forward_frames(frames_u8)`` takes the uint8 frames themselves (the hub's single upload) and gives the same peaks bit for bit.
"""
import ctypes

import torch

from . import _lib, weights

RESOLUTIONS = {'vitpose': weights.VITPOSE_RESOLUTION}      # (width, height): balldetection/config.py:82, tabledetection/config.py:76
DTYPES = {'f32': 0, 'bf16': 1}                             # ttup_vitpose_create_dtype
STAGES = 14                                                # run_stage: 0 patch embedding, 1..12 the blocks, 13 the head
# read_tap: tap -> (columns per token, stored as bf16 on a bf16 handle); 'heat' is (batch, out_ch, H/4, W/4) float32.  The library's
# own table is csrc/vitpose_plan.h's TAPS; tests/test_vitpose_plan_host.py holds the two together.
TAPS = {'x': (384, False), 'x_attn': (384, False), 'qkv': (1152, True), 'att': (384, True), 'hid': (1536, True), 'ln': (384, True),
        'd1': (4 * 256, True), 'd2': (16 * 256, True), 'heat': (None, False)}


class ViTPoseNet:
    """``in_ch`` 9 (ball: three frames) or 3 (table); ``out_ch`` 1 (ball) or 13 (table keypoints).  ``resolution`` is (W, H)."""

    def __init__(self, state_dict, in_ch=9, out_ch=1, resolution=weights.VITPOSE_RESOLUTION, max_batch=32, micro_batch=0,
                 device='cuda:0', dtype='f32'):
        if dtype not in DTYPES:
            raise ValueError("dtype must be 'f32' or 'bf16', got %r" % (dtype,))
        _lib.require_gpu()
        self.device = torch.device(device)
        self.W, self.H = int(resolution[0]), int(resolution[1])
        self.IN_CH, self.OUT_CH = int(in_ch), int(out_ch)
        self.max_batch = int(max_batch)
        self.dtype = dtype
        self._lib = _lib.load()
        blob = weights.pack_vitpose_blob(state_dict, in_ch=self.IN_CH, out_ch=self.OUT_CH)
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_vitpose_create_dtype(blob, len(blob), self.H, self.W, self.max_batch, int(micro_batch), self.IN_CH, self.OUT_CH,
                                                     DTYPES[dtype], ctypes.byref(self._handle))
        _lib.check(rc)
        self.micro_batch = self._lib.ttup_vitpose_micro_batch(self._handle)

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def __del__(self):
        h, self._handle = getattr(self, '_handle', None), None
        if h:
            self._lib.ttup_vitpose_destroy(h)

    def forward(self, x, want_heatmap=True, want_peaks=False):
        """x (B, in_ch, H, W) float -> (heat or None, None), or with want_peaks (heat or None, argmax (B*C_out,) int64 flat index
        into each (H/4, W/4) map, windows (B*C_out, 9) float32 zero-padded 3x3 around it)."""
        if x.dim() != 4 or x.shape[1] != self.IN_CH or x.shape[2] != self.H or x.shape[3] != self.W:
            raise ValueError('expected input (B,%d,%d,%d), got %s' % (self.IN_CH, self.H, self.W, tuple(x.shape)))
        x = x.to(self.device, torch.float32).contiguous()
        b, k, h, w = x.shape[0], self.OUT_CH, self.H // 4, self.W // 4
        heats, idxs, wins = [], [], []
        for b0 in range(0, b, self.max_batch):
            xb = x[b0:b0 + self.max_batch]
            nb = xb.shape[0]
            heat = torch.empty((nb, k, h, w), dtype=torch.float32, device=self.device) if want_heatmap else None
            idx = torch.empty((nb * k,), dtype=torch.int64, device=self.device) if want_peaks else None
            win = torch.empty((nb * k, 9), dtype=torch.float32, device=self.device) if want_peaks else None
            with torch.cuda.device(self.device):
                rc = self._lib.ttup_vitpose_forward(self._handle, _lib.ptr(xb), nb, _lib.ptr(heat), _lib.ptr(idx), _lib.ptr(win), _lib.stream_ptr())
            _lib.check(rc)
            heats.append(heat); idxs.append(idx); wins.append(win)
        heat = (torch.cat(heats) if heats else torch.empty((0, k, h, w), dtype=torch.float32, device=self.device)) if want_heatmap else None
        if want_peaks:
            if not idxs:
                return heat, torch.empty((0,), dtype=torch.int64, device=self.device), torch.empty((0, 9), dtype=torch.float32, device=self.device)
            return heat, torch.cat(idxs), torch.cat(wins)
        return heat, None

    def forward_frames(self, frames_u8, want_heatmap=False):
        """(N, h, w, 3) uint8 BGR device frames (any h, w; a slice of a larger tensor is fine) -> (heat or None, argmax (S*C_out,) int64,
        windows (S*C_out, 9) float32) of the S = N - 2 triples (in_ch 9) or N frames (in_ch 3): the values `forward` gives on
        wasb.preprocess_triples / preprocess_frames of the same frames, with every frame pre-processed once.  Split at max_batch
        samples (consecutive calls share in_ch / 3 - 1 frames)."""
        if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
            raise ValueError('frames must be a uint8 (N,h,w,3) tensor')
        nf = self.IN_CH // 3
        if self.IN_CH != 3 * nf:
            raise ValueError('a %d-channel handle does not take BGR frames' % self.IN_CH)
        frames_u8 = frames_u8.to(self.device).contiguous()
        n, fh, fw = frames_u8.shape[0], frames_u8.shape[1], frames_u8.shape[2]
        if n < nf:
            raise ValueError('%d frames: a %d-channel sample needs at least %d' % (n, self.IN_CH, nf))
        s, k = n - nf + 1, self.OUT_CH
        heat = torch.empty((s, k, self.H // 4, self.W // 4), dtype=torch.float32, device=self.device) if want_heatmap else None
        idx = torch.empty((s * k,), dtype=torch.int64, device=self.device)
        win = torch.empty((s * k, 9), dtype=torch.float32, device=self.device)
        for b0 in range(0, s, self.max_batch):
            nb = min(self.max_batch, s - b0)
            with torch.cuda.device(self.device):
                rc = self._lib.ttup_vitpose_forward_frames(self._handle, _lib.ptr(frames_u8[b0:b0 + nb + nf - 1]), nb + nf - 1, fh, fw,
                                                           _lib.ptr(heat[b0:b0 + nb]) if want_heatmap else None, _lib.ptr(idx[b0 * k:]),
                                                           _lib.ptr(win[b0 * k:]), _lib.stream_ptr())
            _lib.check(rc)
        return heat, idx, win

    def features(self, x):
        """x (B, in_ch, H, W) float -> (B * tokens, 384) float32: the backbone alone, last_norm's output -- what the keypoint head's
        deconvolutions read (`vitpose_head.ViTPoseHead.forward`), bit-equal to the 'ln' tap.  Runs in micro-batches; an f32 handle only."""
        if self.dtype != 'f32':
            raise ValueError("features needs an f32 handle: a %s handle keeps last_norm's output in %s" % (self.dtype, self.dtype))
        if x.dim() != 4 or x.shape[1] != self.IN_CH or x.shape[2] != self.H or x.shape[3] != self.W:
            raise ValueError('expected input (B,%d,%d,%d), got %s' % (self.IN_CH, self.H, self.W, tuple(x.shape)))
        x = x.to(self.device, torch.float32).contiguous()
        out = torch.empty((x.shape[0] * (self.H // 16) * (self.W // 16), 384), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_vitpose_features(self._handle, _lib.ptr(x), x.shape[0], _lib.ptr(out), _lib.stream_ptr())
        _lib.check(rc)
        return out

    def run_stage(self, stage, x):
        """The testing seam: one stage alone.  Stage 0: the patch embedding of x (B, in_ch, H, W); 1..12: that block on the float32
        residual stream x (B * tokens, 384); 13: the head on a residual stream.  B is at most the micro-batch; `read_tap` then
        returns what the stage left in the handle's buffers."""
        tokens = (self.H // 16) * (self.W // 16)
        x = x.to(self.device, torch.float32).contiguous()
        if stage == 0:
            if x.dim() != 4 or tuple(x.shape[1:]) != (self.IN_CH, self.H, self.W):
                raise ValueError('expected input (B,%d,%d,%d), got %s' % (self.IN_CH, self.H, self.W, tuple(x.shape)))
            batch = x.shape[0]
        else:
            if x.dim() != 2 or x.shape[1] != 384 or x.shape[0] % tokens:
                raise ValueError('expected a residual stream (B*%d,384), got %s' % (tokens, tuple(x.shape)))
            batch = x.shape[0] // tokens
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_vitpose_run_stage(self._handle, int(stage), _lib.ptr(x), batch, _lib.stream_ptr())
        _lib.check(rc)
        self._stage_batch = batch

    def read_tap(self, tap):
        """A tap of the last `run_stage` as a device tensor: (B * tokens, columns) -- float32, or the raw bf16 bits as int16 viewed as
        torch.bfloat16 where a bf16 handle stores bf16 -- and 'heat' as (B, out_ch, H/4, W/4) float32.  'd1' and 'd2' are NHWC: 4 and
        16 pixels of 256 channels per token."""
        if tap not in TAPS:
            raise ValueError('unknown tap %r (one of %s)' % (tap, ', '.join(sorted(TAPS))))
        batch = getattr(self, '_stage_batch', 0)
        tokens = (self.H // 16) * (self.W // 16)
        cols, narrow = TAPS[tap]
        shape = (batch, self.OUT_CH, self.H // 4, self.W // 4) if tap == 'heat' else (batch * tokens, cols)
        out = torch.empty(shape, dtype=torch.bfloat16 if narrow and self.dtype == 'bf16' else torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_vitpose_read_tap(self._handle, tap.encode(), _lib.ptr(out), out.numel() * out.element_size())
        _lib.check(rc)
        return out

    __call__ = forward
