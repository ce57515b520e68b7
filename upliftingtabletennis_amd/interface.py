"""Drop-in boundary: the classes of the reference's ``interface.py`` (:83-312) for the ball-detection ->
refine -> uplift path, same constructor arguments, method names, argument meaning, return types and errors.

Differences forced by the environment (documented in DESIGN.md):
  * no network: weights come from ``TTUP_WEIGHTS`` (a directory laid out like the reference's weight zip:
    inference_balldetection/<name>/model.pt, inference_uplifting/ours/model.pt) or from the folder the reference
    unpacks that zip into under the torch hub directory; when neither exists the constructors raise the reference's
    RuntimeError unless ``TTUP_SYNTHETIC_WEIGHTS=1`` asks for the seeded generators in ``weights.py`` (with a warning);
  * the in-tree WASB/HRNet and ViTPose-small ('vitpose') detectors are built; 'segformerpp_*' needs the un-vendored
    KieDani/SegformerPlusPlus hub repo and raises NotImplementedError;
  * table detection uses the in-tree HRNet ('hrnet'); the pipeline's primaries are WASB / HRNet (the reference's SegFormer++
    primaries are unavailable), and its aux slots hold ViTPose-small (`TableTennisPipeline(ball_aux='vitpose',
    table_aux='vitpose')`) or, by default, the primary itself -- which then stands in for both sides of the agreement filter.
Quirks kept on purpose: BGR frames are fed to the detector as they come (interface.py:96,104-110); the
*table* variant of the refine is used on the hub surface (interface.py:116); visibility is always 1.
"""
import os
import time

import numpy as np
import torch

from . import _lib, calib, detect_eval, glue, inference, refine, uplift, vitpose, vitpose_backbone, vitpose_head, wasb, weights
from .detect_eval import ball_val_metrics, heatmap_loss, heatmap_loss_grad, heatmap_loss_grad_device, table_val_metrics  # noqa: F401  (the evaluation functions, beside the detectors they measure)

HEIGHT, WIDTH = 1080, 1920
KEYPOINT_VISIBLE = 1


def _weights_dir():
    """Where reference-format checkpoints are looked for: $TTUP_WEIGHTS, else the folder the reference itself unpacks its
    weight archive into (interface.py:34-73: <torch hub dir>/checkpoints/tt_uplifting_extracted/weights)."""
    d = os.environ.get('TTUP_WEIGHTS', '')
    if d:
        return d
    hub = os.path.join(torch.hub.get_dir(), 'checkpoints', 'tt_uplifting_extracted', 'weights')
    return hub if os.path.isdir(hub) else ''


def _seed():
    return int(os.environ.get('TTUP_SEED', '0'))


def _find_checkpoint(task, name, what):
    """-> (state_dict, additional_info) of <weights dir>/<task>/<name>/model.pt, or None when there is no such file and
    TTUP_SYNTHETIC_WEIGHTS=1 explicitly asks for seeded random weights (benchmarks / smoke tests: the outputs are then meaningless
    as detections; said in a warning).  Otherwise no checkpoint is an error: the reference downloads one or raises RuntimeError
    (interface.py:61,71); there is no network here, so the same RuntimeError is raised."""
    d = _weights_dir()
    path = os.path.join(d, task, name, 'model.pt')
    if d and os.path.exists(path):
        return weights.load_checkpoint_state_dict(path)
    if os.environ.get('TTUP_SYNTHETIC_WEIGHTS') != '1':
        raise RuntimeError('Failed to download weights: %s not found and there is no network; point TTUP_WEIGHTS at a folder laid '
                           'out like the reference weight archive, or set TTUP_SYNTHETIC_WEIGHTS=1 for seeded random weights' % (path if d else what))
    import warnings
    warnings.warn('upliftingtabletennis_amd: %s runs on SEEDED RANDOM weights (TTUP_SYNTHETIC_WEIGHTS=1); its outputs '
                  'are not detections' % what, RuntimeWarning, stacklevel=3)
    return None


def _load_ball_checkpoint(model_name):
    """-> (state_dict, resolution (W,H), in_frames).  Reference: inference_balldetection.load_model :40-61."""
    res = vitpose.RESOLUTIONS['vitpose'] if model_name == 'vitpose' else wasb.RESOLUTIONS['wasb']
    found = _find_checkpoint('inference_balldetection', model_name, "BallDetector('%s')" % model_name)
    if found is not None:
        sd, info = found
        return sd, tuple(info.get('image_resolution', res)), int(info.get('in_frames', 3))
    if model_name == 'vitpose':
        return weights.random_vitpose_state_dict(_seed(), in_ch=9, out_ch=1, resolution=res), res, 3
    return weights.random_wasb_state_dict(_seed(), planted=True), res, 3


def _load_table_checkpoint(model_name):
    """-> (state_dict, resolution (W,H)).  Reference: inference_tabledetection.load_model :40-57."""
    res = vitpose.RESOLUTIONS['vitpose'] if model_name == 'vitpose' else (1280, 704)
    found = _find_checkpoint('inference_tabledetection', model_name, "TableDetector('%s')" % model_name)
    if found is not None:
        return found[0], tuple(found[1].get('image_resolution', res))
    if model_name == 'vitpose':
        return weights.random_vitpose_state_dict(_seed() + 1, in_ch=3, out_ch=13, resolution=res), res
    # seeded stand-in: a planted path to every keypoint head, so the heatmaps are PEAKED like a trained detector's (one dominant
    # maximum per keypoint map; on pure noise weights every map is a field of near-ties and the certified argmax degrades to the
    # full-frame fp32 path -- TTUP_TABLE_NOISE_WEIGHTS=1 selects that regime)
    noise = os.environ.get('TTUP_TABLE_NOISE_WEIGHTS') == '1'
    return weights.random_wasb_state_dict(_seed() + 1, planted=not noise, in_ch=3, head_out=13, plant_all_heads=not noise), res


def _load_uplift_checkpoint():
    """-> (state_dict, size, transform_mode).  Reference: inference_uplifting.load_model :33-58."""
    found = _find_checkpoint('inference_uplifting', 'ours', 'UpliftingModel()')
    if found is None:
        return weights.random_uplift_state_dict(_seed(), 'large'), 'large', 'global'
    sd, info = found
    if info.get('name', 'connectstage') != 'connectstage' or info.get('tabletoken_mode', 'dynamic') != 'dynamic':
        raise ValueError('only connectstage/dynamic uplift checkpoints are supported')
    if info.get('time_rotation', 'new') != 'new':       # the reference hands this to get_model (inference_uplifting.py:49-52)
        raise ValueError("only time_rotation='new' uplift checkpoints are supported (got %r)" % info.get('time_rotation'))
    return sd, info.get('size', 'large'), info.get('transform_mode', 'global')


class _HubDetector:
    """What the four detectors share: the constructor tail, the frame upload, the peak refine and `cert`, the certified argmax of a
    bf16 handle -- a wasb.EpsAudit, where the protocol lives: eps measured on the first input, one sample per 256 audited after it;
    None when certification is off, the handle is fp32 or the detector is a ViTPose (either dtype) -- with the detector calls that go through it.  `calibrate`,
    `enqueue`, `audit`, `settle` and `refine_peaks` are what the pipeline's overlapped clip path drives a detector by; each does the
    right thing with and without `cert`."""
    NO_CERTIFY_ENV = ('TTUP_NO_CERTIFY',)
    HEAT_DIV = 1            # the heatmaps are model_resolution / HEAT_DIV
    CLIP_AUX = False        # whether the clip path can run this detector as an aux detector, beside the primaries and with nothing to settle
    CERTIFIES = True        # whether a bf16 handle of this detector gets the certified argmax

    def _init_hub(self, model, res, max_batch):
        self.device = torch.device('cuda')
        self.resolution = (WIDTH, HEIGHT)
        self.KEYPOINT_VISIBLE = KEYPOINT_VISIBLE
        self.model, self.model_resolution, self.max_batch = model, res, max_batch
        off = not self.CERTIFIES or model.dtype != 'bf16' or any(os.environ.get(k) == '1' for k in self.NO_CERTIFY_ENV)
        self.cert = None if off else wasb.EpsAudit(model, every=0 if os.environ.get('TTUP_NO_AUDIT') == '1' else 256, seed=0)

    def _head_pass_check(self):
        """`head_loss_and_grad` exists for the ViTPose detectors alone (their head is the one whose backward is built)"""
        raise NotImplementedError('head_loss_and_grad: only the ViTPose detectors have a head backward (DESIGN.md section 29)')

    @property
    def AUDIT_EVERY(self):
        """Samples per audited sample."""
        return self.cert.every

    @AUDIT_EVERY.setter
    def AUDIT_EVERY(self, every):
        self.cert.every = self.cert.every_fast = int(every)

    @property
    def heat_hw(self):
        w, h = self.model_resolution
        return h // self.HEAT_DIV, w // self.HEAT_DIV

    def _upload(self, images):
        """A list of BGR uint8 HWC frames (a triple, a batch, a stretch of a clip) -> one (N,h,w,3) uint8 device tensor."""
        return torch.from_numpy(np.stack([np.asarray(i) for i in images])).to(self.device)

    def refine_peaks(self, idx, win):
        """Peaks -> (len(idx), 3) float64 device positions [x, y, visibility] in 1920x1080 px: 3x3 Gaussian refine around the argmax,
        table variant (interface.py:113-116), scaled by the heatmap size."""
        h, w = self.heat_hw
        return refine.refine_windows_device(idx.reshape(-1), win.reshape(-1, 9), h, w, self.resolution[0], self.resolution[1], _lib.REFINE_TABLE)

    def refine_peaks_as(self, idx, win, variant):
        """`refine_peaks` with the fit of `variant` (_lib.REFINE_BALL: what the ball val() refines with, helper_balldetection.py:29-110)."""
        h, w = self.heat_hw
        return refine.refine_windows_device(idx.reshape(-1), win.reshape(-1, 9), h, w, self.resolution[0], self.resolution[1], variant)

    def calibrate(self, frames_u8=None, x=None):
        """First eps, on the first input this detector sees (a uint8 clip or a float input); a no-op after it and when uncertified."""
        if self.cert is not None and not self.model.certified:
            self.model.calibrate(frames_u8, n=4 if x is None else 2, exact_windows=os.environ.get('TTUP_EXACT_WINDOWS') == '1', x=x)

    def _certified_forward(self, x):
        """(heat, idx, win) of the float input x (the `self.model(x)` seam of `predict`): the certified argmax -- the fp32 index the
        reference's torch.argmax returns -- or, with certification off, the handle's own."""
        self.calibrate(x=x)
        if self.cert is None:
            return wasb.WASBNet.forward(self.model, x, want_heatmap=True, want_peaks=True)
        c = self.cert.run(x=x)
        return c.heat, c.idx, c.win

    def _certified_peaks(self, fr):
        """(idx, win) of the samples of the uint8 device clip `fr` (one forward call), certified like `_certified_forward`."""
        if self.cert is None:
            return self.model.forward_frames(fr)[1:]
        c = self.cert.run(fr)
        return c.idx, c.win

    def enqueue(self, frames_u8, f0, f1):
        """One call on frames_u8[f0:f1], enqueued on the current stream -> wasb.CertCall (without status and info when uncertified)."""
        if self.cert is not None:
            return self.cert.enqueue(frames_u8, f0, f1)
        return wasb.CertCall(f0, f1, *self.model.forward_frames(frames_u8[f0:f1])[1:])

    def audit(self, frames_u8, n, after):
        """Count the n samples of the clip frames_u8 and enqueue the eps audit of those drawn among them: on the fp32 twin, on its own
        stream next to the detector calls, once the current stream has seen the event `after` (the clip's last upload).  -> a ticket
        for `settle`; None when nothing was drawn or the detector is uncertified."""
        picks = self.cert.picks(n) if self.cert is not None else []
        if not picks:
            return None
        torch.cuda.current_stream(self.device).wait_event(after)
        return self.cert.audit(picks, frames_u8)

    def settle(self, calls, frames_u8, audit):
        """The host half of enqueued calls once their stream has drained (`EpsAudit.settle`; a call run again whole is a new, counted
        call: `EpsAudit.run`) -> the positions of the calls whose peaks changed: none when uncertified."""
        if self.cert is None:
            return set()
        return self.cert.settle(calls, frames_u8, audit=audit, rerun=lambda c: self.cert.run(frames_u8[c.f0:c.f1]))

    # `val`, `heatmap_loss_grad` and `head_loss_and_grad` of both detectors, over the two hooks BallDetector and TableDetector provide:
    #   _net_input(images)            the network input of a run of images (ball: triples; table: frames)
    #   _targets(n, *annotations)     the annotations of n images -> (centres (n,C,2) float64, has_target (n,C) int32)

    def _chunks(self, images, centres, has):
        """The forward in chunks of `max_batch` -> per chunk (`_certified_forward` of its input, its centres, its has_target)."""
        for b0 in range(0, len(images), self.max_batch):
            b1 = min(len(images), b0 + self.max_batch)
            yield self._certified_forward(self._net_input(images[b0:b1])), centres[b0:b1], has[b0:b1]

    def _val(self, images, annotations, sigma, weighted, variant, tolerances, batch_size, finish, metrics):
        """`val`: per chunk the peaks refined with `variant` and the loss sums, both kept on the device; then `metrics(positions)` ->
        device (sums, counts), one read-back, and `finish` for the ratios."""
        centres, has = self._targets(len(images), *annotations)
        pos, sums = [], []
        for (heat, idx, win), c, t in self._chunks(images, centres, has):
            pos.append(self.refine_peaks_as(idx, win, variant))
            sums.append(detect_eval.heatmap_loss_device(heat, c, t, sigma, weighted, (HEIGHT, WIDTH)))
        if not pos:
            raise ValueError('need at least one sample')
        loss_sums = torch.cat(sums)
        msums, counts = metrics(torch.cat(pos))
        msums, counts, loss_sums = detect_eval.read_back(msums, counts, loss_sums)
        out = finish(msums, counts, [float(t) for t in tolerances])
        out.update(loss=detect_eval.loss_from_sums(loss_sums, (HEIGHT, WIDTH), batch_size), loss_sums=loss_sums)
        return out

    def _heatmap_loss_grad(self, images, annotations, sigma, size, weighted):
        """`heatmap_loss_grad`: per chunk the loss sums and the gradient, with the whole batch's scale."""
        n = len(images)
        centres, has = self._targets(n, *annotations)
        scale = 1.0 / (max(n, 1) * has.shape[1] * int(size[0]) * int(size[1]))
        sums, grads = [], []
        for (heat, _, _), c, t in self._chunks(images, centres, has):
            s, g = detect_eval.heatmap_loss_grad_device(heat, c, t, sigma, weighted, size, scale)
            sums.append(s)
            grads.append(g)
        if not sums:
            raise ValueError('need at least one sample')
        return detect_eval.loss_from_sums(torch.cat(sums).cpu().numpy(), size), torch.cat(grads)

    def _full_pass_check(self):
        """`loss_and_grad` exists for the ViTPose detectors alone (theirs is the network whose backward is built)"""
        raise NotImplementedError('loss_and_grad: only the ViTPose detectors have a backward (DESIGN.md section 30)')

    def _loss_and_grad(self, images, annotations, sigma, size, weighted, train, drop_scale):
        """`loss_and_grad`: the whole batch in one call (one BatchNorm over it)."""
        self._full_pass_check()
        n = len(images)
        centres, has = self._targets(n, *annotations)
        if not n:
            raise ValueError('need at least one sample')
        return self._full_pass(self._net_input(images), centres, has, sigma, size, weighted, 1.0 / (n * has.shape[1] * int(size[0]) * int(size[1])), train, drop_scale)

    def _head_loss_and_grad(self, images, annotations, sigma, size, weighted, train):
        """`head_loss_and_grad`: the whole batch in one call (one BatchNorm over it)."""
        self._head_pass_check()
        n = len(images)
        centres, has = self._targets(n, *annotations)
        if not n:
            raise ValueError('need at least one sample')
        return self._head_pass(self._net_input(images), centres, has, sigma, size, weighted, 1.0 / (n * has.shape[1] * int(size[0]) * int(size[1])), train)


class BallDetector(_HubDetector):
    def __new__(cls, model_name='segformerpp_b2', *a, **k):
        return super().__new__(ViTPoseBallDetector if cls is BallDetector and model_name == 'vitpose' else cls)

    def __init__(self, model_name='segformerpp_b2', max_batch=32, dtype='bf16', lanes=0):
        if 'segformerpp' in model_name:
            raise NotImplementedError("detector '%s' depends on code that is not vendored in the reference "
                                      "(KieDani/SegformerPlusPlus); only 'wasb' and 'vitpose' are built" % model_name)
        _lib.require_gpu()
        sd, res, in_frames = _load_ball_checkpoint(model_name)
        self._init_hub(wasb.get_model(model_name, in_frames=in_frames, resolution=res, pretraining=False, state_dict=sd,
                                      max_batch=max_batch, dtype=dtype, lanes=lanes), res, max_batch)

    def predict(self, images):
        """images: list (length B) of [prev, curr, next] BGR uint8 HWC arrays.
        Returns (pred_pos (B,3) float64 [x, y, confidence] in 1920x1080 px, preds (B,1,H,W) float32; ViTPose: (B,1,H/4,W/4))."""
        pred_pos, preds = [], []
        w, h = self.model_resolution
        for b0 in range(0, len(images), self.max_batch):
            xs = [wasb.preprocess_triples(self._upload(imgs), (w, h)) for imgs in images[b0:b0 + self.max_batch]]
            # peaks from the certified argmax (the fp32 index the reference's torch.argmax returns), table-variant fit (interface.py:116)
            heat, idx, win = self._certified_forward(torch.cat(xs))
            pred_pos.append(self.refine_peaks(idx, win).cpu().numpy())
            preds.append(heat.cpu().numpy())
        if not pred_pos:
            return np.zeros((0, 3)), np.zeros((0, 1) + self.heat_hw, np.float32)
        return np.concatenate(pred_pos, axis=0), np.concatenate(preds, axis=0)

    def _net_input(self, images):
        return torch.cat([wasb.preprocess_triples(self._upload(imgs), self.model_resolution) for imgs in images])

    def _targets(self, n, ball_coords, vis):
        centres = np.asarray(ball_coords, np.float64).reshape(n, 1, 2)
        return centres, (np.asarray(vis).reshape(n) != detect_eval.BALL_INVISIBLE).astype(np.int32).reshape(n, 1)

    def val(self, images, ball_coords, min_coords, max_coords, vis, sigma=6, refine='ball', tolerances=(2, 5, 10), batch_size=None):
        """The reference's ball val() (balldetection/train.py:144-245) on this detector.  images: list (length B) of [prev, curr, next]
        BGR uint8 HWC arrays, as `predict` takes them; ball_coords / min_coords / max_coords (B,2) annotations in 1920x1080 px (the
        ball and the two ends of its motion-blur streak); vis (B,) with BALL_VISIBLE = 1.
        -> {'loss', 'pck@2', 'pck@5', 'pck@10', 'avg_dist', 'dist_streak', the counts of detect_eval.ball_val_metrics, 'loss_sums' (B,1)}.

        The forward runs in chunks of `max_batch`; the peaks are refined on the device (refine='ball' as val() does, 'table' as
        inference_balldetection.py:94), positions and per-sample loss sums stay there, one metrics launch finishes, and the one
        read-back of the result is the only synchronisation.  The loss is val()'s unweighted nn.MSELoss at 1080x1920 against a
        Gaussian of `sigma` px around ball_coords (zeros where vis is BALL_INVISIBLE, as the TTHQ loader builds them); batch_size:
        the loader's batch size, whose per-batch means val() averages (None: one batch)."""
        variant = detect_eval.refine_variant(refine)
        return self._val(images, (ball_coords, vis), sigma, False, variant, tolerances, batch_size, detect_eval.finish_ball,
                         lambda pos: detect_eval.ball_metrics_device(pos, ball_coords, min_coords, max_coords, np.asarray(vis).reshape(len(images)), tolerances))

    def heatmap_loss_grad(self, images, ball_coords, vis, sigma=6, size=(HEIGHT, WIDTH), weighted=True):
        """The reference's ball training loss (balldetection/train.py:112-113: weighted_mse_loss after F.interpolate to `size`;
        weighted=False: nn.MSELoss) on this detector, and its gradient into the detector's heatmaps -- the seed of a backward pass.
        images, ball_coords, vis as `val` takes them.  -> (loss: the element mean over the whole batch, grad (B,1,H,W) float32
        device tensor, shaped like the heatmaps: d loss / d heatmap).  The forward runs in the chunks `val` runs; no heatmap goes
        to the host."""
        return self._heatmap_loss_grad(images, (ball_coords, vis), sigma, size, weighted)

    def head_loss_and_grad(self, images, ball_coords, vis, sigma=6, size=(HEIGHT, WIDTH), weighted=True, train=True):
        """`heatmap_loss_grad` carried on through the keypoint head: the backbone's features, the head's
        training-mode forward with the whole batch in one BatchNorm (train=False: the running statistics), the loss's gradient
        into the heatmaps and the head's backward.  -> (loss, {reference key: gradient} of the head's eight parameters, dfeat
        (B * tokens, 384): the gradient into last_norm's output).  Works on a copy of the detector's head parameters: the
        detector itself is unchanged.  ViTPose / f32 only."""
        return self._head_loss_and_grad(images, (ball_coords, vis), sigma, size, weighted, train)

    def loss_and_grad(self, images, ball_coords, vis, sigma=6, size=(HEIGHT, WIDTH), weighted=True, train=True, drop_scale=None):
        """The ball training loss and the gradient of every parameter of the detector: the backbone's
        training forward (drop_scale (12, 2, B): the stochastic-depth factor of every residual branch and sample, as
        `vitpose_backbone.sample_drop_scale` draws them; None: all ones), the head's training-mode forward with the whole batch
        in one BatchNorm (train=False: the running statistics), the loss's gradient into the heatmaps, the head's backward and
        the backbone's.  -> (loss, {reference key: gradient} of the 157 parameters: 149 backbone + 8 head).  Works on a copy of
        the detector's parameters: the detector itself is unchanged.  ViTPose / f32 only."""
        return self._loss_and_grad(images, (ball_coords, vis), sigma, size, weighted, train, drop_scale)

    def predict_clip(self, images):
        """Fast path for consecutive frames (what TableTennisPipeline.predict feeds the detector, interface.py:276-279):
        images = list of N BGR uint8 HWC frames -> pred_pos (N-2, 3), the same values `predict` returns for the triples
        (images[i-1], images[i], images[i+1]).  Every frame is uploaded once and pre-processing, CNN, argmax and window
        extraction run fused on the device; no heatmap is written."""
        n = len(images)
        if n < 3:
            return np.zeros((0, 3))
        out = []
        step = self.max_batch                      # triples per call; consecutive calls overlap by two frames
        for t0 in range(0, n - 2, step):
            fr = self._upload(images[t0:t0 + step + 2])
            self.calibrate(fr)
            out.append(self.refine_peaks(*self._certified_peaks(fr)).cpu().numpy())
        return np.concatenate(out, axis=0)

    def filter_trajectory(self, ball_positions, ball_positions_aux, fps):
        return glue.filter_trajectory_ball(ball_positions, ball_positions_aux, fps)


class TableDetector(_HubDetector):
    NO_CERTIFY_ENV = ('TTUP_NO_CERTIFY', 'TTUP_NO_TABLE_CERTIFY')

    def __new__(cls, model_name='segformerpp_b2', *a, **k):
        return super().__new__(ViTPoseTableDetector if cls is TableDetector and model_name == 'vitpose' else cls)

    def __init__(self, model_name='segformerpp_b2', max_batch=8, dtype='bf16', lanes=0):
        if 'segformerpp' in model_name:
            raise NotImplementedError("detector '%s' depends on code that is not vendored in the reference; only 'hrnet' and 'vitpose' are built" % model_name)
        _lib.require_gpu()
        sd, res = _load_table_checkpoint(model_name)
        self._init_hub(wasb.get_table_model(model_name, resolution=res, pretraining=False, state_dict=sd, max_batch=max_batch, dtype=dtype, lanes=lanes),
                       res, max_batch)

    def predict(self, images):
        """images: list (length B) of BGR uint8 HWC frames.
        Returns (pred_pos (B,13,3) float64 [x, y, visibility] in 1920x1080 px, preds (B,1,13,H,W) float32 -- the reference
        stacks one (1,13,H,W) tensor per frame with np.array, interface.py:165-167; ViTPose: (B,1,13,H/4,W/4))."""
        pred_pos, preds = [], []
        for b0 in range(0, len(images), self.max_batch):
            fr = self._upload(images[b0:b0 + self.max_batch])
            # per-channel peaks from the certified argmax: the reference takes them from fp32 heatmaps (interface.py:148-172 ->
            # tabledetection/helper_tabledetection.py:50-156)
            heat, idx, win = self._certified_forward(wasb.preprocess_frames(fr, self.model_resolution))
            pred_pos.append(self.refine_peaks(idx, win).cpu().numpy().reshape(-1, 13, 3))
            preds.append(heat.cpu().numpy()[:, None])
        if not pred_pos:
            return np.zeros((0, 13, 3)), np.zeros((0, 1, 13) + self.heat_hw, np.float32)
        return np.concatenate(pred_pos, axis=0), np.concatenate(preds, axis=0)

    def _net_input(self, images):
        return wasb.preprocess_frames(self._upload(images), self.model_resolution)

    def _targets(self, n, table_coords):
        coords = np.asarray(table_coords, np.float64).reshape(n, 13, 3)
        return np.ascontiguousarray(coords[:, :, :2]), (coords[:, :, 2] == KEYPOINT_VISIBLE).astype(np.int32)

    def val(self, images, table_coords, sigma=6, tolerances=(2, 5, 10), batch_size=None):
        """The reference's table val() (tabledetection/train.py:131-201) on this detector.  images: list (length B) of BGR uint8 HWC
        frames; table_coords (B,13,3) [x, y, visibility] annotations in 1920x1080 px (the loader's integer pixel positions).
        -> {'loss', 'pck@2', 'pck@5', 'pck@10', 'avg_dist', 'ratio_detected', the counts of detect_eval.table_val_metrics,
        'loss_sums' (B,13)}.  Runs like `BallDetector.val`; the loss is val()'s weighted_mse_loss, against zeros for a keypoint
        whose visibility is not KEYPOINT_VISIBLE."""
        return self._val(images, (table_coords,), sigma, True, _lib.REFINE_TABLE, tolerances, batch_size, detect_eval.finish_table,
                         lambda pos: detect_eval.table_metrics_device(pos.reshape(-1, 13, 3), np.asarray(table_coords, np.float64).reshape(len(images), 13, 3), tolerances))

    def heatmap_loss_grad(self, images, table_coords, sigma=6, size=(HEIGHT, WIDTH), weighted=True):
        """The reference's table training loss (tabledetection/train.py:106-107) on this detector and its gradient into the
        detector's heatmaps; images and table_coords as `val` takes them.  -> (loss, grad (B,13,H,W) float32 device tensor).  Runs
        like `BallDetector.heatmap_loss_grad`; the target of a keypoint whose visibility is not KEYPOINT_VISIBLE is zeros."""
        return self._heatmap_loss_grad(images, (table_coords,), sigma, size, weighted)

    def head_loss_and_grad(self, images, table_coords, sigma=6, size=(HEIGHT, WIDTH), weighted=True, train=True):
        """`heatmap_loss_grad` carried on through the keypoint head, like `BallDetector.head_loss_and_grad`.  -> (loss, grads,
        dfeat).  ViTPose / f32 only."""
        return self._head_loss_and_grad(images, (table_coords,), sigma, size, weighted, train)

    def loss_and_grad(self, images, table_coords, sigma=6, size=(HEIGHT, WIDTH), weighted=True, train=True, drop_scale=None):
        """The table training loss and the gradient of every parameter of the detector, like `BallDetector.loss_and_grad`.
        -> (loss, grads).  ViTPose / f32 only."""
        return self._loss_and_grad(images, (table_coords,), sigma, size, weighted, train, drop_scale)

    def predict_keypoints(self, images):
        """`predict` without the heatmaps: (B,13,3) keypoints only.  Pre-processing, CNN, per-channel argmax and windows run
        fused on the device; nothing but the 39 numbers per frame comes back to the host."""
        out = []
        for b0 in range(0, len(images), self.max_batch):
            fr = self._upload(images[b0:b0 + self.max_batch])
            self.calibrate(fr)
            out.append(self.refine_peaks(*self._certified_peaks(fr)).cpu().numpy().reshape(-1, 13, 3))
        return np.concatenate(out, axis=0) if out else np.zeros((0, 13, 3))

    def calibrate_camera(self, keypoints):
        """interface.py:174-175: (13,3) keypoints -> (Mint, Mext); host numpy/SciPy like the reference (calib.py)."""
        return calib.calibrate_camera(keypoints)

    def filter_trajectory(self, table_keypoints, table_keypoints_aux):
        return glue.filter_trajectory_table(table_keypoints, table_keypoints_aux)


class _ViTPoseHooks:
    """What a ViTPose detector changes in its base: it is uncertified -- a ViT's receptive field is global, so the certified argmax's
    fp32 crops do not apply: `cert` is None and nothing is calibrated, for the fp32 path (csrc/vitpose.hip, `dtype='f32'`, the
    default: peaks from fp32 heatmaps like the reference's) and for the bf16 path (`dtype='bf16'`, DESIGN.md section 24: meant for
    the aux slot, whose only job is to agree with the primary within the agreement filters' pixel radii) alike -- its heatmaps are
    a quarter of the model resolution, and its clip call (`ViTPoseNet.forward_frames`) takes a frame range of any length."""
    HEAT_DIV = 4
    CLIP_AUX = True
    CERTIFIES = False

    def _certified_forward(self, x):
        return self.model.forward(x, want_heatmap=True, want_peaks=True)

    def _keep_head(self, state_dict):
        """The head's parameters in the reference's layout, for `head_loss_and_grad` (the handle itself holds them BN-folded)"""
        self._head_state = {k: np.array(weights._np(v)) for k, v in state_dict.items() if '.keypoint_head.' in k}
        self._backbone_state = {k: np.array(weights._np(v)) for k, v in state_dict.items() if '.backbone.' in k}          # for `loss_and_grad`

    def _head_pass_check(self):
        if self.model.dtype != 'f32':
            raise ValueError("head_loss_and_grad needs dtype='f32': a %s handle keeps last_norm's output in %s" % (self.model.dtype, self.model.dtype))

    def _head_pass(self, x, centres, has, sigma, size, weighted, scale, train):
        """features -> the head's training forward (one BN over the whole batch) -> the loss's gradient -> the head's backward, on a
        head of its own per call: a copy of the parameters and a workspace sized for this batch, freed with it"""
        net = self.model
        feat = net.features(x)
        head = vitpose_head.ViTPoseHead(self._head_state, net.OUT_CH, max_rows=feat.shape[0], device=net.device)
        heat = head.forward(feat, (net.H // 16, net.W // 16), train=train)
        sums, grad = detect_eval.heatmap_loss_grad_device(heat, centres, has, sigma, weighted, size, scale)
        grads, dfeat = head.backward(grad)
        return detect_eval.loss_from_sums(sums.cpu().numpy(), size), grads, dfeat

    def _full_pass_check(self):
        if self.model.dtype != 'f32':
            raise ValueError("loss_and_grad needs dtype='f32': the training pass is fp32 (a %s handle)" % self.model.dtype)

    def _full_pass(self, x, centres, has, sigma, size, weighted, scale, train, drop_scale):
        """the backbone's training forward -> the head's (one BN over the whole batch) -> the loss's gradient -> the head's backward ->
        the backbone's, on a backbone and a head of their own per call: copies of the parameters and workspaces sized for this
        batch, freed with them"""
        net = self.model
        backbone = vitpose_backbone.ViTPoseBackbone(self._backbone_state, net.IN_CH, (net.W, net.H), max_batch=x.shape[0], device=net.device)
        feat = backbone.forward(x, drop_scale)
        head = vitpose_head.ViTPoseHead(self._head_state, net.OUT_CH, max_rows=feat.shape[0], device=net.device)
        heat = head.forward(feat, (net.H // 16, net.W // 16), train=train)
        sums, grad = detect_eval.heatmap_loss_grad_device(heat, centres, has, sigma, weighted, size, scale)
        grads, dfeat = head.backward(grad)
        grads.update(backbone.backward(dfeat))
        return detect_eval.loss_from_sums(sums.cpu().numpy(), size), grads


class ViTPoseBallDetector(_ViTPoseHooks, BallDetector):
    """BallDetector('vitpose'): the reference's ViTPose-small ball detector (balldetection/models/vitpose.py, in_frames 3,
    1152x640, heatmaps at a quarter of that)."""

    def __init__(self, model_name='vitpose', max_batch=32, dtype='f32', lanes=0):
        _lib.require_gpu()
        sd, res, in_frames = _load_ball_checkpoint(model_name)
        self._init_hub(vitpose.ViTPoseNet(sd, in_ch=3 * in_frames, out_ch=1, resolution=res, max_batch=max_batch, dtype=dtype), res, max_batch)
        self._keep_head(sd)


class ViTPoseTableDetector(_ViTPoseHooks, TableDetector):
    """TableDetector('vitpose'): the reference's ViTPose-small table-keypoint detector (tabledetection/models/vitpose.py, 13
    heatmaps at a quarter of 1152x640)."""

    def __init__(self, model_name='vitpose', max_batch=8, dtype='f32', lanes=0):
        _lib.require_gpu()
        sd, res = _load_table_checkpoint(model_name)
        self._init_hub(vitpose.ViTPoseNet(sd, in_ch=3, out_ch=13, resolution=res, max_batch=max_batch, dtype=dtype), res, max_batch)
        self._keep_head(sd)


class UpliftingModel:
    def __init__(self, max_len=128, model_path=None):
        """model_path: an uplift checkpoint of any variant the reference's ``load_model`` opens (inference.load_uplifting_model);
        None: the hub's `ours` slot, which holds the shipped connectstage/dynamic/new configuration."""
        _lib.require_gpu()
        self.device = torch.device('cuda')
        if model_path is not None:
            self.model, _, self.transform_mode = inference.load_uplifting_model(model_path, max_batch=64, max_len=max_len)
            return
        sd, size, self.transform_mode = _load_uplift_checkpoint()
        self.model = uplift.get_model('connectstage', size, 'dynamic', 'new', state_dict=sd, max_batch=64, max_len=max_len)

    def transform(self, data):
        """NormalizeImgCoords (uplifting/transformations.py:252-266): divide by the uplift resolution 2560x1440."""
        r_img, table_img = data['r_img'], data['table_img']
        r_img = r_img / np.array([2560, 1440])
        table_img[..., :2] = table_img[..., :2] / np.array([2560, 1440])
        data['r_img'], data['table_img'] = r_img, table_img
        return data

    def predict(self, ball_coords, table_coords, times):
        data = self.transform({'r_img': ball_coords, 'table_img': table_coords})
        ball_coords, table_coords = data['r_img'], data['table_img']
        mask = np.zeros((ball_coords.shape[0] + 1,), dtype=np.float32)
        mask[:-1] = 1.0
        return self.predict_without_normalization(ball_coords, table_coords, torch.tensor(mask).to(self.device), times)

    def predict_without_normalization(self, ball_coords, table_coords, mask, times):
        host = all(isinstance(a, np.ndarray) or (torch.is_tensor(a) and a.device.type == 'cpu') for a in (ball_coords, table_coords, mask, times))
        if host and np.asarray(ball_coords).ndim == 2:
            # one rally from host arrays (what the pipeline hands over): padded on the host, ONE upload, the number of valid steps from the
            # host mask -- instead of four uploads, four pad kernels and a device-side mask.sum().item() (three host round trips less)
            b_, t_, m_, tm_ = [np.asarray(a, dtype=np.float32) for a in (ball_coords, table_coords, mask, times)]
            n = m_.shape[-1]
            buf = torch.zeros((4 * n + 39,), dtype=torch.float32).pin_memory()
            hb = buf.numpy()
            hb[:2 * b_.shape[0]] = b_.reshape(-1); hb[2 * n:2 * n + 39] = t_.reshape(-1)
            hb[2 * n + 39:3 * n + 39] = m_.reshape(-1); hb[3 * n + 39:3 * n + 39 + tm_.shape[0]] = tm_.reshape(-1)
            # the reference's mask check (uplifting/model.py:541-546) on the host copy: no device round trip for it
            if not (m_.size and float(m_.min()) == 0.0 and float(m_.max()) == 1.0):
                raise ValueError('wrong format for masks. Should be 0, 1 or -1e9, 0.')
            dev = buf.to(self.device, non_blocking=True)
            pred_rotation, pred_position = self.model(dev[:2 * n].view(1, n, 2), dev[2 * n:2 * n + 39].view(1, 13, 3), dev[2 * n + 39:3 * n + 39].view(1, n),
                                                      dev[3 * n + 39:].view(1, n), check_mask=False)
            mask = m_          # the number of valid steps comes from the host copy
        else:
            ball_coords, table_coords, mask, times = [torch.as_tensor(a).to(self.device, torch.float32) for a in (ball_coords, table_coords, mask, times)]
            if ball_coords.dim() == 2:      # (N,2) -> pad to the mask length like the reference's callers do
                n = mask.shape[-1]
                b = torch.zeros((1, n, 2), device=self.device); b[0, :ball_coords.shape[0]] = ball_coords
                t = torch.zeros((1, n), device=self.device); t[0, :times.shape[0]] = times
                ball_coords, times, mask, table_coords = b, t, mask.reshape(1, n), table_coords.reshape(1, 13, 3)
            pred_rotation, pred_position = self.model(ball_coords, table_coords, mask, times)
        pred_rotation_local = uplift.transform_rotationaxes(pred_rotation, pred_position.clone()) if self.transform_mode == 'global' else pred_rotation
        t_prime = int(mask.sum())          # (a device mask: one read-back)
        return pred_rotation_local.squeeze(0), pred_position[:, :t_prime, :].cpu().numpy().squeeze(0)


def _aux_class(name, vit_cls, what):
    """The detector class an aux slot name selects: None (share the primary), 'vitpose', or the un-vendored 'segformerpp_*'."""
    if name is None or name == 'vitpose':
        return None if name is None else vit_cls
    if isinstance(name, str) and 'segformerpp' in name:
        raise NotImplementedError("%s '%s' depends on code that is not vendored in the reference; only 'vitpose' (or None) is built" % (what, name))
    raise ValueError("%s must be None or 'vitpose', got %r" % (what, name))


def clip_schedule(n, chunk, chunk_long, first, max_batch):
    """The overlapped clip path's schedule for n frames -> (bounds, ball, aux).  bounds: the chunk boundaries -- a short first chunk
    (`first` frames) gets the GPU going while the host still stages the bulk of the clip; after it, chunks of `chunk` frames, or of
    `chunk_long` for clips of at least four chunks.  Chunk k, bounds[k]:bounds[k+1], is one upload, one table-detector call and the
    ball-detector calls ball[k] = [(f0, f1), ...], frame ranges of at most `max_batch` triples each, on the triples whose three
    frames are resident by then (triple t needs frames t..t+2: everything up to c1-3 can go once c1 frames are up).  aux[k]: the
    one frame range an aux ball detector takes for the same triples, None where ball[k] is empty."""
    C = chunk if n < 4 * chunk else chunk_long
    F0 = min(first, C, n)
    bounds = sorted(set([0, F0] + list(range(F0 + C, n, C)) + ([n] if n > F0 else [])))
    ball, aux, t = [], [], 0               # t: first triple not yet submitted
    for c1 in bounds[1:]:
        calls = []
        while t < c1 - 2:
            nt = min(max_batch, c1 - 2 - t)
            calls.append((t, t + nt + 2))
            t += nt
        ball.append(calls)
        aux.append((calls[0][0], c1) if calls else None)
    return bounds, ball, aux


def _to_pinned(t):
    """A pinned host copy of the device tensor t, enqueued on the current stream (the caller records the event to wait for)."""
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    return host


class _ClipRun:
    """One call of `TableTennisPipeline._clip_detections`: the clip on the device, the detector calls enqueued on it and their outputs.
    ViTPose aux detectors (`CLIP_AUX`) run on a third stream from the same upload."""

    def __init__(self, pipe, images, want_table):
        self.t00, self.trace = time.perf_counter(), pipe._trace          # tools/hub_trace.py: host time stamps (ms since the call) of the stages
        self.pipe, self.images, self.n, self.want_table = pipe, images, len(images), want_table
        self.bd, self.td = pipe.ball_detector, pipe.table_detector
        self.ba = pipe.ball_detector_aux if pipe.ball_detector_aux.CLIP_AUX else None
        self.ta = pipe.table_detector_aux if want_table and pipe.table_detector_aux.CLIP_AUX else None
        self.has_aux = self.ba is not None or self.ta is not None
        self.frames, self.st, self.cur = pipe._clip_resources(images, self.has_aux)
        self.ball_calls, self.table_calls, self.table_out, self.ball_aux_out, self.table_aux_out = [], [], [], [], []
        self.ev = self.ball_audit = self.kp_aux_host = self.ev_kp_aux = None

    def mark(self, name):
        if self.trace is not None:
            self.trace.append((name, (time.perf_counter() - self.t00) * 1e3))

    def upload(self, ci, c0, c1):
        """Stage frames c0:c1 (chunk ci) in pinned memory and copy them to the device; `ev` is the end of that copy.  The first chunk
        also calibrates the certified detectors (eps: once per detector)."""
        pipe, k = self.pipe, ci % 2
        if pipe._pin_free[k] is not None:
            pipe._pin_free[k].synchronize()          # the copy that last read this staging buffer is done
        pipe._stage(self.images, c0, c1, pipe._pinned[k])
        self.mark('staged chunk %d' % ci)
        with torch.cuda.stream(self.st['copy']):
            self.frames[c0:c1].copy_(pipe._pinned[k][:c1 - c0], non_blocking=True)
            self.ev = torch.cuda.Event(); self.ev.record()
        pipe._pin_free[k] = self.ev
        if ci == 0:
            self.cur.wait_event(self.ev)
            if c1 >= 3:
                self.bd.calibrate(self.frames[:c1])
            if self.want_table:
                self.td.calibrate(self.frames[:c1])

    def enqueue(self, c0, c1, ball_ranges, aux_range):
        """The detector work on an uploaded chunk: table, ball, aux in that order, each on its own stream behind the upload."""
        frames, st, ev = self.frames, self.st, self.ev
        if self.want_table:
            with torch.cuda.stream(st['table']):
                st['table'].wait_event(ev)
                # the keypoints are refined at once from what the call returned -- settled in `finish_table`, after the stream has
                # drained, and refined again only where a re-certification or repair changed them
                call = self.td.enqueue(frames, c0, c1)
                self.table_calls.append(call)
                self.table_out.append(self.td.refine_peaks(call.idx, call.win))
        for f0, f1 in ball_ranges:
            with torch.cuda.stream(st['ball']):
                st['ball'].wait_event(ev)
                self.ball_calls.append(self.bd.enqueue(frames, f0, f1))
        if self.has_aux:
            with torch.cuda.stream(st['aux']):
                st['aux'].wait_event(ev)
                if self.ta is not None:
                    call = self.ta.enqueue(frames, c0, c1)
                    self.table_aux_out.append(self.ta.refine_peaks(call.idx, call.win))
                    if c1 == self.n:           # the aux keypoints go to the host ahead of the last ball pass: the keypoint filter overlaps it
                        self.kp_aux_host = _to_pinned(torch.cat(self.table_aux_out).reshape(-1, 13, 3))
                        self.ev_kp_aux = torch.cuda.Event(); self.ev_kp_aux.record()
                if self.ba is not None and aux_range is not None:
                    call = self.ba.enqueue(frames, *aux_range)
                    self.ball_aux_out.append(self.ba.refine_peaks(call.idx, call.win))

    def all_enqueued(self):
        """After the last chunk: the clip tensor is held until the streams are through with it, and the ball detector's eps audit (a
        random triple of the clip) is drawn and enqueued."""
        self.mark('all calls enqueued')
        self.frames.record_stream(self.st['ball']); self.frames.record_stream(self.st['table'])
        if self.has_aux:
            self.frames.record_stream(self.st['aux'])
        self.ball_audit = self.bd.audit(self.frames, self.n - 2, self.ev)

    def finish_table(self, table_consumer, return_aux):
        """-> (keypoints or what `table_consumer` makes of them, raw aux keypoints).  The table detector (high-priority streams)
        finishes first: its keypoints come back and the host-side consumer (the DBSCAN filter) runs while the ball detector is still
        busy on the GPU."""
        td, st, calls, frames = self.td, self.st, self.table_calls, self.frames
        audit = td.audit(frames, self.n, self.ev)
        certified = calls[0].status is not None
        with torch.cuda.stream(st['table']):
            kp_host = _to_pinned(torch.cat(self.table_out).reshape(-1, 13, 3))
            if certified:          # the calls' status flags and crop / error info in one copy each
                st_host = _to_pinned(torch.cat([c.status for c in calls]))
                in_host = _to_pinned(torch.stack([c.info for c in calls]))
            ev_t = torch.cuda.Event(); ev_t.record()
        ev_t.synchronize()
        self.mark('table stream drained')
        kp_np = kp_host.numpy()
        if certified:
            o = 0
            for k, c in enumerate(calls):
                nmap = c.idx.shape[0]
                c.status, c.info = st_host.numpy()[o:o + nmap], in_host.numpy()[k]
                o += nmap
            self.cur.wait_stream(st['table'])
        for k in sorted(td.settle(calls, frames, audit)):          # rare: re-certified / repaired calls are refined again
            c = calls[k]
            kp_np[c.f0:c.f1] = td.refine_peaks(c.idx, c.win).cpu().numpy().reshape(-1, 13, 3)
        self.mark('table calls settled')
        if self.ta is not None:
            self.ev_kp_aux.synchronize()
            self.mark('aux table keypoints on the host')
            kp_aux = self.kp_aux_host.numpy().copy()
            kp = table_consumer(kp_np, kp_aux) if table_consumer is not None else kp_np.copy()
        else:
            kp_aux = kp_np.copy() if return_aux else None
            kp = table_consumer(kp_np) if table_consumer is not None else kp_np.copy()
        self.mark('keypoint filter done')
        return kp, kp_aux

    def finish_ball(self, return_aux):
        """-> (positions, raw aux positions if asked for: the primary's where the primary fills the aux slot).  The caller's stream joins every
        stream here, and the host blocks on it in the downloads."""
        for s in self.st.values():
            self.cur.wait_stream(s)
        self.bd.settle(self.ball_calls, self.frames, self.ball_audit)
        out = [self.bd.refine_peaks(c.idx, c.win) for c in self.ball_calls]
        pos = torch.cat(out).cpu().numpy() if out else np.zeros((0, 3))
        self.mark('ball calls settled, positions on the host')
        if self.ba is None or not return_aux:
            return pos, pos
        return pos, torch.cat(self.ball_aux_out).cpu().numpy() if self.ball_aux_out else np.zeros((0, 3))


class TableTennisPipeline:
    def __init__(self, max_batch=32, ball_aux=None, table_aux=None, aux_dtype='f32'):
        """ball_aux / table_aux: the second detector of each agreement filter (interface.py:254-289 runs two per frame).  None: the
        primary stands in for both sides (the filters then keep every detection the primary makes); 'vitpose': ViTPose-small, fed
        from the same single upload of the clip.  The primaries stay WASB / HRNet, and the filters keep the primaries' positions.
        aux_dtype: 'f32' or 'bf16', the arithmetic of the ViTPose aux detectors (vitpose.ViTPoseNet)."""
        if aux_dtype not in vitpose.DTYPES:
            raise ValueError("aux_dtype must be 'f32' or 'bf16', got %r" % (aux_dtype,))
        ball_cls = _aux_class(ball_aux, ViTPoseBallDetector, 'ball_aux')
        table_cls = _aux_class(table_aux, ViTPoseTableDetector, 'table_aux')
        _lib.require_gpu()
        self.device = torch.device('cuda')
        self.CHUNK = int(os.environ.get('TTUP_HUB_CHUNK', self.CHUNK))
        self.FIRST = int(os.environ.get('TTUP_HUB_FIRST', self.FIRST))
        self.CHUNK_LONG = max(self.CHUNK, int(os.environ.get('TTUP_HUB_CHUNK_LONG', self.CHUNK_LONG)))
        # one lane per detector: the two handles already run side by side on their own streams; with two lanes each, four CNN streams
        # (plus copy, audit and refine work) collide on the runtime's four hardware queues, and a high-priority table kernel queued
        # behind a ball kernel is no longer ahead of it (measured on a 48-frame clip: 748-757 -> 804-820 frames/s; table lanes alone:
        # 808-811; GPU_MAX_HW_QUEUES=8 with one lane each: 843)
        lanes = int(os.environ.get('TTUP_HUB_LANES', '1'))
        self.ball_detector = BallDetector(model_name='wasb', max_batch=max(max_batch, self.CHUNK_LONG), lanes=lanes)
        self.table_detector = TableDetector(model_name='hrnet', max_batch=max(16, self.CHUNK_LONG), lanes=lanes)
        # the reference's primary SegFormer++ detectors are not available offline: without an aux detector the primary fills both slots
        self.ball_detector_aux = ball_cls('vitpose', max_batch=max(max_batch, self.CHUNK_LONG), dtype=aux_dtype) if ball_cls else self.ball_detector
        self.table_detector_aux = table_cls('vitpose', max_batch=max(16, self.CHUNK_LONG), dtype=aux_dtype) if table_cls else self.table_detector
        # the overlapped clip path runs both detectors side by side: the table detector goes first on the GPU, so that its
        # host-side consumer (the DBSCAN keypoint filter) overlaps with the rest of the ball detector
        self.table_detector.model.set_priority(True)
        self.uplifting_model = UpliftingModel()
        self.KEYPOINT_VISIBLE = KEYPOINT_VISIBLE
        # the overlapped clip path's streams, pinned staging buffers (created on first use) and staging threads; _trace: a list to
        # collect host time stamps of its stages in (tools/hub_trace.py)
        self._streams = self._pinned = self._pin_free = self._stage_pool = self._trace = None

    def predict(self, images, fps):
        """images: list of BGR frames of one rally; fps: frame rate (interface.py:265-289).
        Returns (pred_spin torch (3,), pred_pos_3d numpy (T',3))."""
        return self._predict(images, fps, None)

    def predict_with_table(self, images, fps, table_keypoints):
        """`predict` with known table keypoints ((13,3) [x,y,vis] in 1920x1080 px), skipping table detection -- an addition
        for fixed-camera streams; the reference surface is `predict`."""
        return self._predict(images, fps, table_keypoints)

    CHUNK = 24          # frames per upload / detector call of the overlapped clip path (measured: 16 -> 68 ms, 24 -> 60 ms, 48 -> 63 ms per 48-frame clip)
    CHUNK_LONG = 64     # ... of clips of at least four chunks, after their first chunk: a detector call drains at its end, so long clips take fewer, larger calls (256 frames: 868 -> see DESIGN.md 11)
    FIRST = 24          # frames of the first chunk (a short first chunk -- 8 frames -- was measured 5 ms SLOWER per clip: its one-micro-batch calls run at half the batched rate)

    def _clip_detections(self, images, want_table, table_consumer=None, return_aux=False):
        """Ball positions (N-2,3) and table keypoints ((N,13,3), or what `table_consumer` makes of them) of one clip with everything overlapped: the frames are staged in
        pinned memory and uploaded ONCE in chunks on a copy stream; while chunk k+1 is staged and copied, the table detector
        runs on chunk k on its own stream and the ball detector on the triples whose three frames are already resident on a
        third; the host blocks only at the end.  Same values as `predict_clip` / `predict_keypoints` (same kernels per frame).
        ViTPose aux detectors run on a third stream from the same upload; `table_consumer` then gets (keypoints, aux keypoints).
        return_aux: (pos, kp, pos_aux, kp_aux), the aux values raw (the primary's where the primary fills the aux slot)."""
        run = _ClipRun(self, images, want_table)
        bounds, ball, aux = clip_schedule(run.n, self.CHUNK, self.CHUNK_LONG, self.FIRST, self.ball_detector.max_batch)
        for ci, (c0, c1) in enumerate(zip(bounds[:-1], bounds[1:])):
            run.upload(ci, c0, c1)
            run.enqueue(c0, c1, ball[ci], aux[ci])
        run.all_enqueued()
        kp, kp_aux = run.finish_table(table_consumer, return_aux) if want_table else (None, None)
        pos, pos_aux = run.finish_ball(return_aux)
        return (pos, kp, pos_aux, kp_aux) if return_aux else (pos, kp)

    def _clip_resources(self, images, aux):
        """-> (the clip's device tensor, the streams, the caller's stream, which the streams start behind).  Streams and pinned staging
        buffers are created on first use and kept."""
        dev = self.device
        h0, w0 = np.asarray(images[0]).shape[:2]
        frames = torch.empty((len(images), h0, w0, 3), dtype=torch.uint8, device=dev)
        if self._streams is None:
            self._streams = {k: torch.cuda.Stream(dev) for k in ('ball', 'table')}
            self._streams['copy'] = self._streams['table']          # uploads ride on the table stream (chunk k+1 behind the table pass of chunk k): one stream fewer
        st = self._streams
        if self._pinned is None or self._pinned[0].shape[1:] != (h0, w0, 3):          # CHUNK_LONG rows: the largest chunk
            self._pinned = [torch.empty((self.CHUNK_LONG, h0, w0, 3), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self._pin_free = [None, None]
        if aux and 'aux' not in st:
            st['aux'] = torch.cuda.Stream(dev)          # the ViTPose passes (the long pole): the HRNet streams run beside them
        cur = torch.cuda.current_stream(dev)
        for s in st.values():
            s.wait_stream(cur)
        return frames, st, cur

    STAGE_THREADS = 4

    def _stage(self, images, c0, c1, pin):
        """Copy frames c0..c1 of the caller's list into the pinned staging buffer.  The copies are plain memcpys of 2.8 MB each
        (numpy releases the GIL for them), so a few threads bring a 16-frame chunk from 4.5 ms down to about 1.5 ms -- the first
        chunk's staging is the one stretch of a clip during which the GPU has nothing to do."""
        dst = pin.numpy()
        nthr = 1 if os.environ.get('TTUP_HUB_STAGE_THREADS') == '1' else self.STAGE_THREADS
        if nthr <= 1 or c1 - c0 < 4:
            for k in range(c0, c1):
                np.copyto(dst[k - c0], images[k])
            return
        if self._stage_pool is None:
            import concurrent.futures
            self._stage_pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.STAGE_THREADS)
        list(self._stage_pool.map(lambda k: np.copyto(dst[k - c0], images[k]), range(c0, c1)))

    def _predict(self, images, fps, table_keypoints):
        # the overlapped clip path feeds an aux detector only when it can run beside the primaries (or is the primary itself)
        overlapped = ((self.ball_detector_aux is self.ball_detector or self.ball_detector_aux.CLIP_AUX)
                      and (self.table_detector_aux is self.table_detector or self.table_detector_aux.CLIP_AUX)
                      and len(images) >= 3
                      and self.table_detector.max_batch >= self.CHUNK_LONG and self.ball_detector.max_batch >= self.CHUNK_LONG
                      and os.environ.get('TTUP_HUB_SERIAL') != '1')
        if overlapped:
            ball_positions, kp, ball_positions_aux, _ = self._clip_detections(
                images, want_table=table_keypoints is None, return_aux=True,
                table_consumer=lambda k, k_aux=None: self.table_detector_aux.filter_trajectory(k, k if k_aux is None else k_aux))
            if table_keypoints is None:
                table_keypoints = kp
        else:
            if table_keypoints is None:        # 2. table detection (interface.py:281-283)
                kp = self.table_detector.predict_keypoints(images)
                kp_aux = kp if self.table_detector_aux is self.table_detector else self.table_detector_aux.predict_keypoints(images)
                table_keypoints = self.table_detector_aux.filter_trajectory(kp, kp_aux)
            # the reference builds (prev, curr, next) triples and pushes each through the detector (interface.py:276-279);
            # the triples are consecutive frames, so the clip path computes the same positions with every frame uploaded once
            ball_positions = self.ball_detector.predict_clip(images)
            ball_positions_aux = ball_positions if self.ball_detector_aux is self.ball_detector else self.ball_detector_aux.predict_clip(images)
        filtered, _, times_ball = self.ball_detector.filter_trajectory(ball_positions, ball_positions_aux, fps)
        ball_coords, table_coords, times, mask = glue._uplifting_transform(filtered, np.asarray(table_keypoints, dtype=np.float64), times_ball)
        return self.uplifting_model.predict_without_normalization(ball_coords, table_coords, mask, times)

    def calibrate_camera(self, keypoints):
        """interface.py:291-299: (13,3) table keypoints [x, y, visibility] in pixels -> Mint (3,4), Mext (4,4)."""
        return calib.calibrate_camera(keypoints)

    def reproject(self, positions_3d, Mint, Mext):
        """interface.py:301-312: (N,3) world positions -> (N,2) pixel positions."""
        return calib.reproject(positions_3d, Mint, Mext)
