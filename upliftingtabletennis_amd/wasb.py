"""a2: drop-in for the reference's ``WASBNet`` module behind ``self.model(x)`` (interface.py:115,
inference/utils.py:57): ``model(x) -> (heatmap (B,1,H,W) float32, None)`` with x (B,9,H,W) float32.

Reference: balldetection/models/wasb.py:510-608 (WASBNet), factory balldetection/train.py:249-271,
loader inference/inference_balldetection.py:40-61.  The forward runs in libttup.so (csrc/wasb_net.hip,
csrc/conv.hip); this class only owns the handle and the torch-side buffers.
"""
import ctypes
import dataclasses

import numpy as np
import torch

from . import _lib, weights
from .detect_eval import ball_val_metrics, heatmap_loss, heatmap_loss_grad, heatmap_loss_grad_device, table_val_metrics  # noqa: F401  (how good the detectors' heatmaps and positions are)

RESOLUTIONS = {'wasb': (1280, 704)}     # balldetection/config.py:84-85 (width, height)


class WASBNet:
    """Callable like the reference nn.Module.  ``resolution`` is (W, H) as in the reference."""
    IN_CH, HEAD_OUT, OUT_CH = 9, 3, 1

    def __init__(self, state_dict, resolution=(1280, 704), in_frames=3, max_batch=64, dtype='bf16', device='cuda:0', lanes=0):
        _lib.require_gpu()
        if in_frames * 3 != self.IN_CH:
            raise ValueError('only in_frames=%d (%d input channels) is built' % (self.IN_CH // 3, self.IN_CH))
        self.device = torch.device(device)
        self.W, self.H = int(resolution[0]), int(resolution[1])
        self.max_batch = int(max_batch)
        self.dtype = dtype
        self._lib = _lib.load()
        self._state_dict = state_dict            # kept for the other handles of the certified argmax (twins, strips, re-runs)
        self._f32_twin = self._bf16_twin = self._strip_twins = self._recert = None
        self.certified = False
        self.eps = None
        self.exact_windows = False
        self.audit_state = dict(audited_frames=0, max_err_seen=0.0, widened=0)          # (calibration + audits: `note_error`)
        blob = weights.pack_wasb_blob(state_dict, in_ch=self.IN_CH, head_out=self.HEAD_OUT)
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_wasb_create_ex(blob, len(blob), self.H, self.W, self.max_batch,
                                               _lib.DTYPE_F32 if dtype == 'f32' else _lib.DTYPE_BF16, 0, int(lanes), ctypes.byref(self._handle))
        _lib.check(rc)

    # nn.Module surface used by the reference call sites
    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def __del__(self):
        h, self._handle = getattr(self, '_handle', None), None
        if h:
            self._lib.ttup_wasb_destroy(h)

    def forward(self, x, want_heatmap=True, want_peaks=False):
        if x.dim() != 4 or x.shape[1] != self.IN_CH or x.shape[2] != self.H or x.shape[3] != self.W:
            raise ValueError('expected input (B,%d,%d,%d), got %s' % (self.IN_CH, self.H, self.W, tuple(x.shape)))
        x = x.to(self.device, torch.float32).contiguous()
        b = x.shape[0]
        if b == 0:          # empty batch: empty results, like the reference nn.Module
            heat = torch.empty((0, self.OUT_CH, self.H, self.W), dtype=torch.float32, device=self.device) if want_heatmap else None
            if want_peaks:
                return heat, torch.empty((0,), dtype=torch.int64, device=self.device), torch.empty((0, 9), dtype=torch.float32, device=self.device)
            return heat, None
        outs = []
        for b0 in range(0, b, self.max_batch):
            xb = x[b0:b0 + self.max_batch]
            nb = xb.shape[0]
            k = self.OUT_CH
            heat = torch.empty((nb, k, self.H, self.W), dtype=torch.float32, device=self.device) if want_heatmap else None
            idx = torch.empty((nb * k,), dtype=torch.int64, device=self.device) if want_peaks else None
            win = torch.empty((nb * k, 9), dtype=torch.float32, device=self.device) if want_peaks else None
            with torch.cuda.device(self.device):
                rc = self._lib.ttup_wasb_forward(self._handle, _lib.ptr(xb), nb, _lib.ptr(heat), _lib.ptr(idx), _lib.ptr(win), _lib.stream_ptr())
            _lib.check(rc)
            outs.append((heat, idx, win))
        heat = torch.cat([o[0] for o in outs]) if want_heatmap else None
        if want_peaks:
            return heat, torch.cat([o[1] for o in outs]), torch.cat([o[2] for o in outs])
        return heat, None

    __call__ = forward

    def forward_frames(self, frames_u8, want_heatmap=False):
        """Fast path: (N,h,w,3) uint8 device tensor -> peaks of the N-2 triples (pre-processing fused in).
        Returns (heat or None, argmax (N-2,) int64, windows (N-2,9) float32)."""
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
            raise ValueError('frames must be uint8 (N,h,w,3)')
        frames_u8 = frames_u8.to(self.device).contiguous()
        n = frames_u8.shape[0]
        nb = n - (self.IN_CH // 3 - 1)
        if nb > self.max_batch:
            raise ValueError('%d samples exceed max_batch %d' % (nb, self.max_batch))
        k = self.OUT_CH
        heat = torch.empty((nb, k, self.H, self.W), dtype=torch.float32, device=self.device) if want_heatmap else None
        idx = torch.empty((nb * k,), dtype=torch.int64, device=self.device)
        win = torch.empty((nb * k, 9), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_wasb_forward_frames(self._handle, _lib.ptr(frames_u8), n, frames_u8.shape[1], frames_u8.shape[2],
                                                    _lib.ptr(heat), _lib.ptr(idx), _lib.ptr(win), _lib.stream_ptr())
        _lib.check(rc)
        return heat, idx, win

    # ---- certified argmax (csrc/certify.hip, csrc/certify_plan.h): the fp32 path's argmax indices from the bf16 path, GIVEN an error bound eps
    # The guarantee is conditional: an index is the fp32 argmax whenever |bf16 heatmap - fp32 heatmap| <= eps on that frame.  eps is
    # an empirical bound, measured and then audited for as long as the handle runs: `EpsAudit` (below) drives these primitives.
    SAFETY = 1.5           # an observed error within this factor of eps triggers a widening (and a re-run of the affected work)
    HEADROOM = 1.5         # eps is set to this factor times the largest error seen (= SAFETY: every new maximum widens eps -- which is cheap:
                           # only the heatmaps whose guard band is not empty are run again, `recertify_subset`)

    def set_certify(self, eps_abs, crop=0, max_crops_per_map=0, exact_windows=None):
        """eps_abs bounds |bf16 heatmap - fp32 heatmap|; < 0 switches the certification off.  exact_windows=True: every heatmap
        (not only the near-ties) gets an fp32 crop, so every 3x3 window holds fp32 values (parity mode, one fp32 crop per frame)."""
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ttup_wasb_set_certify(self._handle, float(eps_abs), int(crop), int(max_crops_per_map)))
        self.certified = eps_abs >= 0
        self.eps = float(eps_abs)
        if exact_windows is not None:
            self.exact_windows = bool(exact_windows)
        if self.certified:
            _lib.check(self._lib.ttup_wasb_certify_exact_windows(self._handle, 1 if self.exact_windows else 0))
            if self.exact_windows:
                self.certify_budget(2 * self.max_batch)

    def certify_audit_crops(self, every, phase=0):
        """Audit crops of the forwards that follow: of the frames f with (f + phase) % every == 0, one single-candidate heatmap gets an
        fp32 crop as well, which reports |bf16 - fp32| at the winner (`certify_info`, folded into eps by `EpsAudit.settle`).  every = 0: off (default)."""
        _lib.check(self._lib.ttup_wasb_certify_audit_crops(self._handle, int(every), int(phase)))

    def _make(self, resolution=None, max_batch=1, dtype='bf16'):
        """Another handle of this detector type with the same weights."""
        return type(self)(self._state_dict, resolution=resolution or (self.W, self.H), max_batch=max_batch, dtype=dtype, device=self.device)

    def _twin(self):
        if self._f32_twin is None:
            self._f32_twin = self._make(dtype='f32')
        return self._f32_twin

    @property
    def NF(self):
        """Frames per sample: 3 (ball detector, triples) or 1 (table detector)."""
        return self.IN_CH // 3

    def _pre(self, frames_u8):
        """The network input of the samples of a uint8 clip: (N - NF + 1, IN_CH, H, W) float32."""
        return (preprocess_triples if self.NF == 3 else preprocess_frames)(frames_u8, (self.W, self.H))

    def _heat(self, x):
        """(B, OUT_CH, H, W) heatmaps of a float input, whatever `forward` of the subclass returns."""
        return WASBNet.forward(self, x, want_heatmap=True)[0]

    def _audit_twin(self):
        """A one-sample bf16 handle with the same weights: the audit re-computes the production path's heatmap of a frame on its own
        buffers (the kernels are per-tile deterministic: same values as the batched handle, asserted in the tests), so it never
        touches the production handle's lanes or its per-call certification state."""
        if self._bf16_twin is None:
            self._bf16_twin = self._make(dtype='bf16')
        return self._bf16_twin

    SUBSET_MAX_SHARE = 0.25      # recertify_subset: above this share of guarded heatmaps the caller re-runs the whole call
    AUDIT_STRIP = 320      # columns of the image strip an audit re-computes (full height); calibration uses whole frames

    AUDIT_MARGIN = 72      # = the receptive-field radius: columns this close to an artificial strip border are left out of the measure

    def heatmap_error(self, frames_u8, t, x0=None, out=None, accumulate=False):
        """max |bf16 heatmap - fp32 heatmap| of sample t of the uint8 clip, on the current stream -> 0-dim device tensor.
        x0=None: the whole frame (calibration).  x0 = a column (multiple of 8): only the strip [x0, x0 + AUDIT_STRIP) of the
        pre-processed sample is run through a bf16 and an fp32 handle of that size -- any sub-image is a fair sample of the
        bf16-vs-fp32 error on this kind of content, and a quarter-width strip costs a quarter of the fp32 time.  The strip's own
        zero padding is not the frame's: the columns within AUDIT_MARGIN (the receptive-field radius) of a strip border that is not
        an image border are left out of the maximum (round-3 advisor).  `out`: a (1,) device tensor for the result; with
        accumulate=True its current value is kept as a running maximum.  Library kernels only (no torch element-wise work beside the CNN, csrc/common.h)."""
        fr = frames_u8[t:t + self.NF]
        if x0 is None or self.W <= self.AUDIT_STRIP:
            hb, _, _ = self._audit_twin().forward_frames(fr, want_heatmap=True)
            hf = self._twin()._heat(self._pre(fr))
            return max_abs_diff(hb[0], hf[0], out=out, accumulate=accumulate)
        S = self.AUDIT_STRIP
        xs = slice_columns(self._pre(fr), x0, S)
        if self._strip_twins is None:
            res = (S, self.H)
            self._strip_twins = (self._make(res, dtype='bf16'), self._make(res, dtype='f32'))
        tw = self._strip_twins
        c0 = 0 if x0 == 0 else self.AUDIT_MARGIN
        c1 = S if x0 + S >= self.W else S - self.AUDIT_MARGIN
        return max_abs_diff(tw[0]._heat(xs)[0], tw[1]._heat(xs)[0], cols=(c0, c1), out=out, accumulate=accumulate)

    def calibrate(self, frames_u8=None, n=8, exact_windows=None, x=None):
        """First estimate of eps: HEADROOM x the largest bf16-vs-fp32 heatmap error on `n` samples spread over the uint8 (N,h,w,3) clip
        `frames_u8`, or on the first `n` samples of the float input `x` (against this handle's own heatmaps).  The samples count as
        audited.  Enables the certified argmax and returns eps; `EpsAudit` keeps it honest from then on."""
        if x is not None:
            picks = range(min(n, x.shape[0]))
            hb = self._heat(x[:len(picks)])
            twin = self._twin()
            err = max(float(max_abs_diff(hb[k], twin._heat(x[k:k + 1])[0]).item()) for k in picks)
        else:
            frames_u8 = frames_u8.to(self.device)
            nt = frames_u8.shape[0] - (self.NF - 1)
            n = max(1, min(n, nt))
            picks = sorted(set(int(round(k * (nt - 1) / max(1, n - 1))) for k in range(n))) if n > 1 else [0]
            err = max(float(self.heatmap_error(frames_u8, t).item()) for t in picks)
        self.set_certify(self.HEADROOM * err, exact_windows=exact_windows)
        self.note_error(err, len(picks))
        return self.eps

    def note_error(self, err, n_frames=0):
        """Fold an observed |bf16 - fp32| error (and the number of samples it covers) into `audit_state`.  Returns err."""
        self.audit_state['audited_frames'] += n_frames
        self.audit_state['max_err_seen'] = max(self.audit_state['max_err_seen'], err)
        return err

    def eps_violated(self, err):
        """True when an observed error is within the safety factor of eps: eps must be widened and the work re-certified."""
        return self.certified and err * self.SAFETY > self.eps * (1 + 1e-6)

    def widen_eps(self, err):
        """eps <- HEADROOM * err (never smaller); affects the forward calls issued from now on."""
        new = max(self.eps, self.HEADROOM * err)
        if new > self.eps:
            self.set_certify(new)
            self.audit_state['widened'] += 1
        return self.eps

    def certify_budget(self, max_crops):
        """Crops the following forward calls may use (saves empty fp32 passes when the typical count is known)."""
        _lib.check(self._lib.ttup_wasb_certify_budget(self._handle, int(max_crops)))

    GUARD = 1.25           # csrc/wasb_net.h CertState::GUARD: widening eps by up to this factor keeps heatmaps with an empty guard band valid

    def certify_status(self, batch, raw=False):
        """Per-heatmap status of the last forward: 0 single candidate, 1 resolved on fp32 crops, 2 not certified.
        raw=True keeps bit 2 (value 4): the guard band below the candidate band is NOT empty, i.e. the heatmap has to be run again
        when eps is widened (heatmaps without it keep their result under any eps up to GUARD times the one they ran with)."""
        st = torch.empty((batch,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            fn = self._lib.ttup_wasb_certify_flags if raw else self._lib.ttup_wasb_certify_status
            _lib.check(fn(self._handle, batch, _lib.ptr(st), _lib.stream_ptr()))
        return st

    def certify_margins(self, batch):
        """fp32 top-2 margin among the candidates of each heatmap of the last forward (+inf: single candidate / not resolved)."""
        m = torch.empty((batch,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ttup_wasb_certify_margins(self._handle, batch, _lib.ptr(m), _lib.stream_ptr()))
        return m

    def certify_info(self):
        """(2,) int32 device tensor of the last forward, in stream order: [crops it asked for, bits of the largest |bf16 - fp32|
        seen at any candidate so far].  `decode_info` turns a host copy into (n_crops, max_candidate_err)."""
        info = torch.empty((2,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ttup_wasb_certify_info(self._handle, _lib.ptr(info), _lib.stream_ptr()))
        return info

    @staticmethod
    def decode_info(info):
        """`certify_info` (device or host) -> (n_crops, max_candidate_err)."""
        a = np.asarray(_host(info), dtype=np.int32)
        return int(a[0]), float(a[1:2].view(np.float32)[0])

    def certify_stats(self, reset=False):
        out = np.zeros(len(_lib.CERT_STATS), np.int64)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ttup_wasb_certify_stats(self._handle, out.ctypes.data_as(ctypes.c_void_p), 1 if reset else 0))
        stats = {k: int(v) for k, v in zip(_lib.CERT_STATS, out)}
        stats['max_candidate_err'] = float(out[_lib.CERT_STATS.index('max_candidate_err'):][:1].astype(np.uint32).view(np.float32)[0])          # a float's bits
        return stats

    def fix_uncertified(self, idx, win, frames_u8=None, x=None, status=None):
        """Heatmaps the certified argmax flagged 2 (candidate / crop budget exceeded) are re-run on the full-frame fp32 path, so that
        every returned index is the fp32 argmax.  Give the call's input -- the uint8 clip (`forward_frames`) or the float tensor
        (`forward`) -- and the call's OWN status (`certify_status` taken right after it, host or device); without it the handle's
        last call is assumed.  idx / win / status hold OUT_CH entries per sample (13 keypoint heatmaps per frame for the table
        detector).  Synchronises; returns the number of samples re-run."""
        K = self.OUT_CH
        if idx.shape[0] > self.max_batch * K:
            raise ValueError('fix_uncertified covers one forward call of at most max_batch=%d samples' % self.max_batch)
        if status is None:
            status = self.certify_status(idx.shape[0])
        st = _host(status) & _lib.CERT_STATUS_MASK
        bad = np.nonzero(st == _lib.CERT_NOT_CERTIFIED)[0]
        samples = np.unique(bad // K)
        if samples.size:
            twin = self._twin()
            for t in samples:
                t = int(t)
                xt = x[t:t + 1] if x is not None else self._pre(frames_u8[t:t + self.NF].to(self.device))
                _, i1, w1 = WASBNet.forward(twin, xt, want_heatmap=False, want_peaks=True)
                for m in bad[bad // K == t]:
                    idx[int(m)] = i1[int(m) - t * K]
                    win[int(m)] = w1[int(m) - t * K]
        return int(samples.size)

    def recertify_subset(self, idx, win, status_raw, eps_used, frames_u8):
        """eps has been widened since the call that produced (idx, win, status_raw) from the uint8 clip `frames_u8`.  Heatmaps whose
        guard band was empty keep their certified result (same candidate set under any eps up to GUARD * eps_used); the others are
        run again one sample at a time under the current eps and repaired on the fp32 handle if they overflow the budget; their entries
        of `status_raw` (a host array) are REPLACED by the re-run's own status -- 0 = single candidate (bf16 window), 1 = settled on fp32
        values (crops, or the full-frame repair) -- so the status keeps saying which windows hold fp32 values.  Returns the indices
        re-run, or None when eps grew past the guard factor (the caller then re-runs the whole call; also when more than
        SUBSET_MAX_SHARE of the heatmaps are guarded)."""
        if self.eps > eps_used * self.GUARD * (1 - 1e-6):
            return None
        st = _host(status_raw)
        todo = np.nonzero((st & _lib.CERT_GUARD) != 0)[0]
        if todo.size == 0:
            return todo
        if todo.size > self.SUBSET_MAX_SHARE * st.size:
            return None          # most of the call is guarded (near-ties everywhere): one batched re-run beats many single ones
        # a one-sample certified handle of its own (same weights, same per-tile arithmetic as the production handle: its bf16
        # heatmaps are bit-identical, tests/test_certify_audit_gpu.py): the re-runs never touch the production handle's lanes or its
        # per-call certification slots, which a clip in flight may still be using
        if self._recert is None:
            self._recert = self._make(dtype='bf16')
            self._recert._f32_twin = self._twin()
        h = self._recert
        if not h.certified or h.eps != self.eps or h.exact_windows != self.exact_windows:
            h.set_certify(self.eps, exact_windows=self.exact_windows)
            # a one-sample handle defaults to ONE crop per call; a re-run frame may plan up to 8 per heatmap / 16 per frame, and what
            # does not fit the budget goes to the full-frame fp32 repair (3.6 ms instead of 0.1 ms per crop; round-4 advisor)
            h.certify_budget(min(16, 8 * self.OUT_CH))
        K = self.OUT_CH
        for t in np.unique(todo // K):
            t = int(t)
            fr = frames_u8[t:t + self.NF]
            _, i1, w1 = h.forward_frames(fr, want_heatmap=False)
            s1 = h.certify_status(K).cpu().numpy() & _lib.CERT_STATUS_MASK
            h.fix_uncertified(i1, w1, frames_u8=fr, status=s1)
            for m in todo[todo // K == t]:
                idx[int(m)] = i1[int(m) - t * K]
                win[int(m)] = w1[int(m) - t * K]
                if isinstance(status_raw, np.ndarray):
                    status_raw[int(m)] = _lib.CERT_SINGLE if s1[int(m) - t * K] == _lib.CERT_SINGLE else _lib.CERT_RESOLVED
        return todo

    def internal_streams(self):
        """The handle's own HIP streams as torch ExternalStreams: lanes first, then the certified argmax's fp32 stream."""
        out = (ctypes.c_void_p * 8)()
        n = ctypes.c_int(0)
        _lib.check(self._lib.ttup_wasb_streams(self._handle, out, 8, ctypes.byref(n)))
        return [torch.cuda.ExternalStream(int(out[k]), device=self.device) for k in range(n.value)]

    def set_priority(self, high=True):
        """Run this handle's kernels ahead of (high) / behind other handles sharing the GPU."""
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ttup_wasb_set_priority(self._handle, 1 if high else 0))

    def read_tap(self, name, batch=1):
        c, h, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(self._lib.ttup_wasb_read_tap(self._handle, name.encode(), batch, None, ctypes.byref(c), ctypes.byref(h), ctypes.byref(w), None))
        out = torch.empty((batch, c.value, h.value, w.value), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ttup_wasb_read_tap(self._handle, name.encode(), batch, _lib.ptr(out), ctypes.byref(c), ctypes.byref(h), ctypes.byref(w), _lib.stream_ptr()))
        return out


def _host(a):
    """A status / info array on the host: device tensors are copied, host tensors and arrays are viewed."""
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


@dataclasses.dataclass
class CertCall:
    """One forward call of the certified argmax (`EpsAudit.enqueue`) on the input range f0:f1 (frames of a uint8 clip, or samples of a
    float input), its peaks (updated in place by `settle`), raw status flags and info (device tensors, host arrays once settled; None
    when the handle is not certified), the eps it ran under and, for a float input, its heatmaps."""
    f0: int
    f1: int
    idx: torch.Tensor
    win: torch.Tensor
    status: object = None
    info: object = None
    eps_used: float = None
    heat: torch.Tensor = None


class EpsAudit:
    """The host protocol of the certified argmax for one bf16 handle, which keeps its empirical eps honest after `WASBNet.calibrate`:
      1. `enqueue`: a forward call, its status flags and info copied right behind it (the handle's per-call slot flips with its next call).
      2. `picks` / `audit`: one sample per `rate()` samples re-run in both precisions -- `every_fast` until eps has stood for
         `settle_clips` settles in a row, then `every`.  Every fp32 crop of a call reports the error at its candidates for free.
      3. `settle`: fold those errors into eps (the handle's `audit_state`), widen it when one comes within SAFETY of it, re-run the
         guarded heatmaps of calls certified under a smaller eps (`recertify_subset`) -- the whole call past the guard factor, or on
         any widening for a float input -- and repair heatmaps over the crop budget on the fp32 twin (`fix_uncertified`)."""

    def __init__(self, net, every=256, every_fast=None, settle_clips=0, seed=0):
        self.net = net
        self.every = int(every)
        self.every_fast = self.every if every_fast is None else int(every_fast)
        self.settle_clips = int(settle_clips)
        self.seen = 0                  # samples counted by `picks`
        self.quiet = 0                 # settles in a row without a widening
        self.widen_sources = {'strip': 0, 'candidates': 0}
        self.recertified_calls = 0     # whole calls run again
        self.recertified_heatmaps = 0  # guarded heatmaps run again
        self.fp32_reruns = 0           # samples repaired on the full-frame fp32 path
        self.rng = np.random.default_rng(seed)              # which samples are audited
        self.strip_rng = np.random.default_rng(12345)       # where an audit's strip lies
        self.audit_stream = None
        self._since = 0

    @property
    def eps(self):
        """The bound the handle certifies under; None until calibrated."""
        return self.net.eps if self.net.certified else None

    def rate(self):
        """Samples per audited sample right now (0: no audits)."""
        if self.every <= 0:
            return 0
        return self.every_fast if self.quiet < self.settle_clips else self.every

    def picks(self, n):
        """Count the n samples of a call's input; returns those of them that the audit re-runs: one per `rate()` samples."""
        self.seen += max(0, int(n))
        every = self.rate()
        if every <= 0 or n <= 0:
            return []
        self._since += n
        out = []
        while self._since >= every:
            self._since -= every
            out.append(int(self.rng.integers(n)))
        return out

    def audit(self, picks, frames_u8=None, x=None, heat=None):
        """Enqueue the audit of the samples `picks` -> a ticket for `settle` (None without picks).  A uint8 clip: each sample's heatmap
        re-computed on the one-sample bf16 audit twin and the fp32 twin over a quarter-width strip at a random column, on a side stream
        behind everything the current stream has enqueued (enqueue it ahead of the call).  A float input: the call's own heatmaps
        `heat` against the fp32 twin, on the current stream."""
        if not picks:
            return None
        net = self.net
        if x is not None:
            err = torch.empty((1,), dtype=torch.float32, device=net.device)
            for k, t in enumerate(picks):
                max_abs_diff(heat[t], net._twin()._heat(x[t:t + 1])[0], out=err, accumulate=k > 0)
            return self._ticket(err, len(picks))
        if self.audit_stream is None:
            self.audit_stream = torch.cuda.Stream(net.device)
        st = self.audit_stream
        st.wait_stream(torch.cuda.current_stream(net.device))
        with torch.cuda.stream(st):
            err = torch.empty((1,), dtype=torch.float32, device=net.device)
            for k, t in enumerate(picks):          # the running maximum lives in `err` (the library's kernel folds each sample in)
                x0 = 8 * int(self.strip_rng.integers(0, max(1, (net.W - net.AUDIT_STRIP) // 8 + 1)))
                net.heatmap_error(frames_u8, int(t), x0, out=err, accumulate=k > 0)
            ticket = self._ticket(err, len(picks))
        frames_u8.record_stream(st)
        return ticket

    @staticmethod
    def _ticket(err, n):
        """max |bf16 - fp32| of n audited samples, copied to pinned host memory behind the audit on the current stream."""
        host = torch.empty((1,), dtype=torch.float32, pin_memory=True)
        host.copy_(err, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return {'host': host, 'event': ev, 'n': n}

    def enqueue(self, frames_u8=None, f0=0, f1=None, x=None):
        """Enqueue one forward call on the current stream -> CertCall: the samples of the uint8 clip frames_u8[f0:f1] (no heatmaps), or
        of the float input x (with heatmaps).  Status flags and info are copied right behind it (not on an uncertified handle)."""
        net, eps = self.net, self.eps
        if x is None:
            heat, idx, win = net.forward_frames(frames_u8[f0:f1], want_heatmap=False)
        else:
            heat, idx, win = WASBNet.forward(net, x, want_heatmap=True, want_peaks=True)
        if not net.certified:
            return CertCall(f0, f1, idx, win, heat=heat)
        return CertCall(f0, f1, idx, win, net.certify_status(idx.shape[0], raw=True), net.certify_info(), eps, heat)

    def run(self, frames_u8=None, x=None, counted=False):
        """One call start to finish (blocking): audit, enqueue, settle -> its CertCall.  `settle` runs the whole call again through this
        method with counted=True: its samples are not counted, and no audit drawn, a second time."""
        n = x.shape[0] if x is not None else frames_u8.shape[0] - (self.net.NF - 1)
        picks = [] if counted else self.picks(n)
        audit = self.audit(picks, frames_u8) if x is None else None
        call = self.enqueue(frames_u8, x=x)
        if x is not None:
            audit = self.audit(picks, x=x, heat=call.heat)
        self.settle([call], frames_u8, x=x, audit=audit, rerun=lambda c: self.run(frames_u8, x, counted=True))
        return call

    def settle(self, calls, frames_u8=None, x=None, audit=None, rerun=None):
        """The host half of enqueued calls on one input (the uint8 clip `frames_u8`, or one call on the float input `x`), once their
        status and info are on the host or their stream has drained; `audit`: a ticket of `audit`.  In this order: fold the calls'
        candidate errors and the audit into eps; widen it if one comes within SAFETY of it; re-certify each call whose eps_used is now
        stale -- or, if eps grew past the guard factor, replace its peaks and status by those of `rerun(call)`, a new certified call on
        the same input; repair its status-2 heatmaps on the fp32 twin.  Returns the positions of the calls whose idx / win changed."""
        changed = set()
        if not calls:
            return changed
        net = self.net
        cand = net.note_error(max(net.decode_info(c.info)[1] for c in calls))
        strip = 0.0
        if audit is not None:
            audit['event'].synchronize()
            strip = net.note_error(float(audit['host'][0]), audit['n'])
        err = max(cand, strip)
        widened = net.eps_violated(err)
        if widened:
            net.widen_eps(err)
            self.widen_sources['strip' if strip > cand else 'candidates'] += 1
        self.quiet = 0 if widened else self.quiet + 1
        for k, c in enumerate(calls):
            c.status = _host(c.status)
            fr = frames_u8[c.f0:c.f1] if frames_u8 is not None else None
            if c.eps_used < net.eps:
                todo = net.recertify_subset(c.idx, c.win, c.status, c.eps_used, fr) if x is None else None
                if todo is None:
                    self.recertified_calls += 1
                    new = rerun(c)
                    c.idx, c.win, c.status, c.heat = new.idx, new.win, new.status, new.heat
                    changed.add(k)
                    continue
                self.recertified_heatmaps += int(todo.size)
                if todo.size:
                    changed.add(k)          # (c.status[todo] holds the re-runs' own status now: 0 or 1)
            if ((c.status & _lib.CERT_STATUS_MASK) == _lib.CERT_NOT_CERTIFIED).any():
                self.fp32_reruns += net.fix_uncertified(c.idx, c.win, frames_u8=fr, x=x, status=c.status)
                changed.add(k)
        return changed


class MyHRNet(WASBNet):
    """Table-keypoint detector: reference tabledetection/models/hrnet.py:510-589 -- the same HRNet with a
    3-channel single-frame input and 13 heatmap channels; ``model(x) -> heat (B,13,H,W)`` (a tensor, not a tuple)."""
    IN_CH, HEAD_OUT, OUT_CH = 3, 13, 13

    def __init__(self, state_dict, resolution=(1280, 704), max_batch=16, dtype='bf16', device='cuda:0', lanes=0):
        super().__init__(state_dict, resolution=resolution, in_frames=1, max_batch=max_batch, dtype=dtype, device=device, lanes=lanes)
        self.number_output_channels = 13

    def forward(self, x, want_peaks=False):
        out = super().forward(x, want_heatmap=True, want_peaks=want_peaks)
        return out if want_peaks else out[0]

    __call__ = forward


def get_table_model(model_name, resolution, pretraining=False, state_dict=None, **kw):
    """Mirror of tabledetection/train.py:205-226 for the in-tree HRNet."""
    if model_name != 'hrnet':
        raise ValueError('Model %s not implemented (only the in-tree HRNet table detector is built)' % model_name)
    if state_dict is None:
        raise ValueError('a state_dict is required (no weights can be downloaded offline)')
    return MyHRNet(state_dict, resolution=resolution, **kw)


def preprocess_frames(frames_u8, dst_wh):
    """Single-frame pre-processing on the GPU: (N,h,w,3) uint8 -> (N,3,H,W) float32 (interface.py:160-165)."""
    _lib.require_gpu()
    lib = _lib.load()
    frames_u8 = frames_u8.contiguous()
    n, h, w, _ = frames_u8.shape
    out = torch.empty((n, 3, dst_wh[1], dst_wh[0]), dtype=torch.float32, device=frames_u8.device)
    with torch.cuda.device(frames_u8.device):
        _lib.check(lib.ttup_preprocess_frames(_lib.ptr(frames_u8), n, h, w, dst_wh[1], dst_wh[0], _lib.ptr(out), _lib.stream_ptr()))
    return out


def get_model(model_name, in_frames, resolution, pretraining=False, state_dict=None, **kw):
    """Mirror of balldetection/train.py:249-271 for the in-tree CNN."""
    if model_name != 'wasb':
        raise ValueError('Model %s not implemented (only the in-tree WASB/HRNet detector is built; see DESIGN.md)' % model_name)
    if state_dict is None:
        raise ValueError('a state_dict is required (no weights can be downloaded offline)')
    return WASBNet(state_dict, resolution=resolution, in_frames=in_frames, **kw)


def preprocess_triples(frames_u8, dst_wh):
    """a1 on the GPU: (N,h,w,3) uint8 -> (N-2,9,H,W) float32, the tensor interface.py:104-112 builds."""
    _lib.require_gpu()
    lib = _lib.load()
    frames_u8 = frames_u8.contiguous()
    n, h, w, _ = frames_u8.shape
    out = torch.empty((n - 2, 9, dst_wh[1], dst_wh[0]), dtype=torch.float32, device=frames_u8.device)
    with torch.cuda.device(frames_u8.device):
        _lib.check(lib.ttup_preprocess_triples(_lib.ptr(frames_u8), n, h, w, dst_wh[1], dst_wh[0], _lib.ptr(out), _lib.stream_ptr()))
    return out


def max_abs_diff(a, b, cols=None, out=None, accumulate=False):
    """max |a - b| of two float32 device tensors of equal shape on the current stream -> 0-dim device tensor (ttup_max_abs_diff:
    the audit's error measure without torch's element-wise kernels, which must not run beside the CNN -- csrc/common.h).
    cols=(c0, c1): only the columns [c0, c1) of the last dimension.  out: a (1,) float32 device tensor for the result; with
    accumulate=True its current value is kept as a running maximum."""
    _lib.require_gpu()
    lib = _lib.load()
    a, b = a.contiguous(), b.contiguous()
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.shape != b.shape:
        raise ValueError('max_abs_diff: two float32 tensors of equal shape expected')
    res = out if out is not None else torch.empty((1,), dtype=torch.float32, device=a.device)
    acc = 1 if (accumulate and out is not None) else 0
    if a.numel() == 0:
        if not acc:
            res.zero_()
        return res[0]
    with torch.cuda.device(a.device):
        if cols is None:
            _lib.check(lib.ttup_max_abs_diff_cols(_lib.ptr(a), _lib.ptr(b), 1, a.numel(), 0, a.numel(), _lib.ptr(res), acc, _lib.stream_ptr()))
        else:
            width = a.shape[-1]
            _lib.check(lib.ttup_max_abs_diff_cols(_lib.ptr(a), _lib.ptr(b), a.numel() // width, width, int(cols[0]), int(cols[1]), _lib.ptr(res),
                                                  acc, _lib.stream_ptr()))
    return res[0]


def slice_columns(x, x0, w):
    """x[..., x0:x0 + w] of a contiguous float32 device tensor as a new contiguous tensor, by the library's copy kernel."""
    _lib.require_gpu()
    lib = _lib.load()
    x = x.contiguous()
    out = torch.empty(x.shape[:-1] + (w,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.ttup_slice_columns(_lib.ptr(x), x.numel() // x.shape[-1], x.shape[-1], int(x0), int(w), _lib.ptr(out), _lib.stream_ptr()))
    return out


def time_replay(net, batch=None, reps=10):
    """Milliseconds per pass of the CNN graph over one micro-batch: `reps` passes launched back to back on the current stream between
    ONE pair of HIP events inside the library (ttup_wasb_time_replay) -- no event between the ops, unlike time_ops(in_graph=True),
    whose per-op intervals each carry an event record."""
    import numpy as _np
    lib = net._lib
    micro = lib.ttup_wasb_micro_batch(net._handle)
    batch = micro if batch is None else min(batch, micro)
    ms = _np.zeros(1, _np.float32)
    with torch.cuda.device(net.device):
        _lib.check(lib.ttup_wasb_time_replay(net._handle, batch, int(reps), ms.ctypes.data_as(ctypes.c_void_p), _lib.stream_ptr()))
    return float(ms[0])


_OP_KINDS = {0: 'conv', 1: 'upsum', 2: 'bneck_trans', 3: 'bb_chain', 4: 'stem', 5: 'upsum_head'}


def time_ops(net, batch=None, reps=5, in_graph=True):
    """Per-op timing of the CNN graph (HIP events inside the library, on the current stream).
    in_graph=True: the whole graph in launch order with an event between consecutive ops (what the forward pass sees);
    False: every op on its own, back to back.  Returns a list of dicts {kernel, kind, cin, cout, k, stride, h, w, ms, flops}
    for one micro-batch; flops = algorithmic 2*MACs of the op (0 for the element-wise sums)."""
    import numpy as _np
    lib = net._lib
    micro = lib.ttup_wasb_micro_batch(net._handle)
    batch = micro if batch is None else min(batch, micro)
    ms = _np.zeros(256, _np.float32)
    info = _np.zeros((256, 8), _np.int32)
    names = _np.zeros((256, 64), _np.uint8)
    n = ctypes.c_int()
    with torch.cuda.device(net.device):
        if in_graph:
            _lib.check(lib.ttup_wasb_time_graph(net._handle, batch, reps, 256, ms.ctypes.data_as(ctypes.c_void_p), info.ctypes.data_as(ctypes.c_void_p),
                                                names.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n), _lib.stream_ptr()))
        else:
            _lib.check(lib.ttup_wasb_time_ops(net._handle, batch, reps, 256, ms.ctypes.data_as(ctypes.c_void_p),
                                              info.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n), _lib.stream_ptr()))
    ops = []
    for i in range(n.value):
        kind, cin, cout, k, stride, h, w, cpad = [int(v) for v in info[i]]
        flops = 2.0 * batch * h * w * cout * cin * k * k if kind in (0, 2, 3, 4) else 0.0
        ops.append(dict(index=i, kernel=bytes(names[i]).split(b'\0')[0].decode() or _OP_KINDS[kind], kind=_OP_KINDS[kind], cin=cin, cout=cout, k=k,
                        stride=stride, h=h, w=w, cin_padded=cpad, ms=float(ms[i]), flops=flops, batch=batch))
    return ops
