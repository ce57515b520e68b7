"""Evaluation of the ball and table detectors on the device (csrc/detect_eval.hip): what the reference's val()
(balldetection/train.py:144-245, tabledetection/train.py:131-201) and its evaluation scripts (inference/inference_balldetection.py:64-113
and the table twin) compute from predicted heatmaps and positions -- the heatmap loss at the evaluation resolution, PCK at fixed
pixel tolerances, the average distance, the distance to the motion-blur streak and the ratio of detected keypoints.

fp32 heatmaps and positions, fp64 arithmetic and sums, a fixed summation tree: two calls return the same bits.  The `*_device`
functions enqueue on the current stream and return device tensors; the public functions read them back once and finish the ratios
on the host, with the reference's sentinels: PCK -1 and distances 10000 when no detection is valid, NaN where it divides 0 by 0.
`BallDetector.val` / `TableDetector.val` (interface.py) run a detector through them.  DESIGN.md section 27.

`heatmap_loss_grad` adds the gradient of that loss into the predicted heatmaps -- what the reference's loss.backward() leaves in the
network's output (balldetection/train.py:112-119, tabledetection/train.py:106-108) -- from the same call as the sums; the detectors'
`heatmap_loss_grad` methods run a detector through it.  DESIGN.md section 28."""
import ctypes

import numpy as np
import torch

from . import _lib

HEIGHT, WIDTH = 1080, 1920          # helper_balldetection.py:12: the evaluation resolution
BALL_VISIBLE, BALL_INVISIBLE = 1, 0
KEYPOINT_VISIBLE = 1
MAX_TOLERANCES = 8                  # TTUP_DETECT_MAX_TOLERANCES
NO_DETECTION_PCK, NO_DETECTION_DISTANCE = -1, 10000          # what the reference returns when no detection is valid


def _tolerances(tolerances):
    tol = [float(t) for t in tolerances]
    if not 1 <= len(tol) <= MAX_TOLERANCES:
        raise ValueError('need 1 to %d tolerances, got %d' % (MAX_TOLERANCES, len(tol)))
    return tol, (ctypes.c_double * len(tol))(*tol)


def pck_key(tolerance):
    return 'pck@%g' % tolerance


def refine_variant(refine):
    """'ball' (what the ball val() refines with) or 'table' (inference_balldetection.py:94) -> the _lib.REFINE_* constant."""
    if refine not in ('ball', 'table'):
        raise ValueError("refine must be 'ball' or 'table', got %r" % (refine,))
    return _lib.REFINE_BALL if refine == 'ball' else _lib.REFINE_TABLE


def _device_of(*tensors):
    for t in tensors:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device('cuda')


def _to(a, dev, dtype):
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(dev, dtype).contiguous()


def _workspace(nbytes, dev):
    return torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=dev)


def _heatmap_loss_call(pred, centres, has_target, sigma, weighted, size, scale=None, want_grad=False):
    """What `heatmap_loss_device` and `heatmap_loss_grad_device` (want_grad) share: the operands on pred's device, the shape checks,
    the workspace and the call -> (sums (N, C) float64, grad (N, C, h, w) float32 or None)."""
    _lib.require_gpu()
    lib = _lib.load()
    dev = _device_of(pred)
    pred = _to(pred, dev, torch.float32)
    if pred.dim() != 4:
        raise ValueError('pred must have shape (N, C, h, w), got %s' % (tuple(pred.shape),))
    n, c, h, w = pred.shape
    centres = _to(centres, dev, torch.float64)
    has_target = _to(has_target, dev, torch.int32)
    if tuple(centres.shape) != (n, c, 2) or tuple(has_target.shape) != (n, c):
        raise ValueError('centres must have shape (N, C, 2) and has_target (N, C) for pred %s, got %s and %s'
                         % (tuple(pred.shape), tuple(centres.shape), tuple(has_target.shape)))
    out_h, out_w = int(size[0]), int(size[1])
    if want_grad and scale is None:
        scale = 1.0 / (n * c * out_h * out_w)
    sums = torch.empty((n, c), dtype=torch.float64, device=dev)
    grad = torch.empty((n, c, h, w), dtype=torch.float32, device=dev) if want_grad else None
    head = (_lib.ptr(pred), _lib.ptr(centres), _lib.ptr(has_target), n, c, h, w, float(sigma), out_h, out_w, 1 if weighted else 0)
    with torch.cuda.device(dev):
        if want_grad:
            nbytes = int(lib.ttup_detect_loss_grad_workspace_bytes(n * c, h, w, out_h, out_w))
            ws = _workspace(nbytes, dev)
            _lib.check(lib.ttup_detect_heatmap_loss_grad(*head, float(scale), _lib.ptr(ws), nbytes, _lib.ptr(sums), _lib.ptr(grad), _lib.stream_ptr()))
        else:
            nbytes = int(lib.ttup_detect_loss_workspace_bytes(n * c, out_h, out_w))
            ws = _workspace(nbytes, dev)
            _lib.check(lib.ttup_detect_heatmap_loss(*head, _lib.ptr(ws), nbytes, _lib.ptr(sums), _lib.stream_ptr()))
    return sums, grad


def heatmap_loss_device(pred, centres, has_target, sigma=6, weighted=False, size=(HEIGHT, WIDTH)):
    """-> (N, C) float64 device tensor: per (sample, channel) the sum over the size[0] x size[1] output pixels of
    w (up(pred) - target)^2 (see `heatmap_loss`).  Enqueued on the current stream; nothing synchronises."""
    return _heatmap_loss_call(pred, centres, has_target, sigma, weighted, size)[0]


def loss_from_sums(sums, size=(HEIGHT, WIDTH), batch_size=None):
    """The reference's validation loss from the per-(sample, channel) sums: `loss += loss_fn(...).item() / len(valloader)` over
    batches of `batch_size` samples (the last one may be smaller; None: one batch), each batch's loss its element mean."""
    sums = np.asarray(sums, np.float64)
    n, c = sums.shape
    bs = n if batch_size is None else int(batch_size)
    if bs <= 0:
        raise ValueError('batch_size must be positive, got %r' % (batch_size,))
    starts = range(0, n, bs)
    loss = 0.0
    for b0 in starts:
        b = sums[b0:b0 + bs]
        loss += float(b.sum() / (b.shape[0] * c * int(size[0]) * int(size[1]))) / len(starts)
    return loss


def heatmap_loss(pred, centres, has_target, sigma=6, weighted=False, size=(HEIGHT, WIDTH), batch_size=None):
    """The reference's heatmap loss without its two full-resolution tensors.  pred (N, C, h, w) float32, any h, w >= 1 (w <= 7680);
    centres (N, C, 2) float64 [x, y] in output pixels; has_target (N, C).

    up = torch's F.interpolate(pred, size, mode='bilinear'); target = float32(exp(-((x - cx)^2 + (y - cy)^2) / (2 sigma^2))), zeros
    where has_target is 0 (an invisible ball or keypoint); w = 100 where `weighted` and target > 0.1, else 1 -- `weighted_mse_loss`,
    the training loss of both detectors and the table val() loss; weighted=False is the ball val()'s nn.MSELoss.
    -> {'sums': float64 (N, C), the per-(sample, channel) sums over the output pixels, 'loss': `loss_from_sums` of them}."""
    sums = heatmap_loss_device(pred, centres, has_target, sigma, weighted, size).cpu().numpy()
    return {'sums': sums, 'loss': loss_from_sums(sums, size, batch_size)}


def heatmap_loss_grad_device(pred, centres, has_target, sigma=6, weighted=True, size=(HEIGHT, WIDTH), scale=None):
    """-> (sums (N, C) float64, grad (N, C, h, w) float32), device tensors: `heatmap_loss_device`'s sums, bit for bit, and the gradient
    of scale * sums.sum() with respect to pred (csrc/detect_eval.hip grad_kernel).  scale=None: 1 / (N C size[0]
    size[1]), the element mean -- the reference's loss.backward() into the network's output.  Enqueued on the current stream;
    nothing synchronises."""
    return _heatmap_loss_call(pred, centres, has_target, sigma, weighted, size, scale, want_grad=True)


def heatmap_loss_grad(pred, centres, has_target, sigma=6, weighted=True, size=(HEIGHT, WIDTH), scale=None):
    """The detectors' training loss (`weighted_mse_loss` after F.interpolate; weighted=False: nn.MSELoss) and its gradient into pred,
    without a full-resolution tensor.  Arguments as `heatmap_loss`.  -> (loss: the batch's element mean, what
    `heatmap_loss(..., batch_size=None)['loss']` returns; grad (N, C, h, w) float32 device tensor: the gradient of scale * the summed
    squared error, scale=None: of that mean)."""
    sums, grad = heatmap_loss_grad_device(pred, centres, has_target, sigma, weighted, size, scale)
    return loss_from_sums(sums.cpu().numpy(), size), grad


def _metrics_call(entry, tolerances, n_items, operands, dev):
    """What the two metrics wrappers share: the results, the workspace for n_items items and the call `entry(*operands, tolerances,
    workspace, results, stream)` -> (sums float64 (2,), counts int64 (4 + len(tolerances),)) on `dev`."""
    tol, ctol = tolerances
    sums = torch.empty((2,), dtype=torch.float64, device=dev)
    counts = torch.empty((4 + len(tol),), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        nbytes = int(_lib.load().ttup_detect_metrics_workspace_bytes(n_items))
        ws = _workspace(nbytes, dev)
        _lib.check(entry(*operands, ctol, len(tol), _lib.ptr(ws), nbytes, _lib.ptr(sums), _lib.ptr(counts), _lib.stream_ptr()))
    return sums, counts


def ball_metrics_device(pred_pos, gt_pos, gt_min, gt_max, vis, tolerances=(2, 5, 10)):
    """-> (sums float64 (2,), counts int64 (4 + len(tolerances),)) on the device, as ttup_detect_ball_metrics lays them out."""
    tolerances = _tolerances(tolerances)
    _lib.require_gpu()
    lib = _lib.load()
    dev = _device_of(pred_pos, gt_pos)
    # the reference evaluates np.array(pred_pos, dtype=np.float32) against float32 annotations (train.py:210-213)
    pred, gt, lo, hi = (_to(a, dev, torch.float32) for a in (pred_pos, gt_pos, gt_min, gt_max))
    vis = _to(vis, dev, torch.int32).reshape(-1)
    n = pred.shape[0]
    if pred.dim() != 2 or pred.shape[1] != 3 or any(tuple(a.shape) != (n, 2) for a in (gt, lo, hi)) or tuple(vis.shape) != (n,):
        raise ValueError('pred_pos must have shape (N, 3), gt_pos / gt_min / gt_max (N, 2) and vis (N,)')
    return _metrics_call(lib.ttup_detect_ball_metrics, tolerances, n, (_lib.ptr(pred), _lib.ptr(gt), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(vis), n), dev)


def table_metrics_device(pred_pos, gt_pos, tolerances=(2, 5, 10)):
    """-> (sums float64 (2,), counts int64 (4 + len(tolerances),)) on the device, as ttup_detect_table_metrics lays them out."""
    tolerances = _tolerances(tolerances)
    _lib.require_gpu()
    lib = _lib.load()
    dev = _device_of(pred_pos, gt_pos)
    pred, gt = _to(pred_pos, dev, torch.float32), _to(gt_pos, dev, torch.float32)
    if pred.dim() != 3 or pred.shape[2] != 3 or pred.shape != gt.shape:
        raise ValueError('pred_pos and gt_pos must both have shape (N, K, 3), got %s and %s' % (tuple(pred.shape), tuple(gt.shape)))
    n, k, _ = pred.shape
    return _metrics_call(lib.ttup_detect_table_metrics, tolerances, n * k, (_lib.ptr(pred), _lib.ptr(gt), n, k), dev)


def _ratio(num, den):
    """num / den as numpy divides: NaN for 0 / 0, without the warning."""
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.float64(num) / np.float64(den))


def finish_ball(sums, counts, tolerances):
    """Host half of `ball_val_metrics`: the ratios and sentinels from the device's sums and counts (host arrays)."""
    visible, flagged, detected = (int(c) for c in counts[:3])
    out = {}
    for k, t in enumerate(tolerances):
        out[pck_key(t)] = _ratio(int(counts[3 + k]), flagged) if flagged else NO_DETECTION_PCK
        out['correct@%g' % t] = int(counts[3 + k])
    out['avg_dist'] = _ratio(sums[0], detected) if detected else NO_DETECTION_DISTANCE
    out['dist_streak'] = _ratio(sums[1], detected) if detected else NO_DETECTION_DISTANCE
    out.update(number=int(counts[-1]), visible=visible, valid=flagged, detected=detected)
    return out


def finish_table(sums, counts, tolerances):
    """Host half of `table_val_metrics`."""
    valid, both, total = int(counts[0]), int(counts[1]), int(counts[-1])
    out = {}
    for k, t in enumerate(tolerances):
        out[pck_key(t)] = _ratio(int(counts[3 + k]), both) if valid else NO_DETECTION_PCK
        out['correct@%g' % t] = int(counts[3 + k])
    out['avg_dist'] = _ratio(sums[0], both) if valid else NO_DETECTION_DISTANCE
    out['ratio_detected'] = _ratio(valid, total)
    out.update(number=total, valid=valid, valid_visible=both)
    return out


def ball_val_metrics(pred_pos, gt_pos, gt_min, gt_max, vis, tolerances=(2, 5, 10)):
    """The ball val()'s metrics (balldetection/train.py:207-220) over N samples in one launch.  pred_pos (N, 3) [x, y, visibility]
    in evaluation pixels, gt_pos / gt_min / gt_max (N, 2), vis (N,); evaluated over the samples with vis == BALL_VISIBLE.
    -> {'pck@<t>' per tolerance, 'avg_dist', 'dist_streak', and the counts 'number' (N), 'visible', 'valid' (prediction visibility
    == 1: PCK's denominator), 'detected' (x, y > -100: the distances' denominator), 'correct@<t>'}.

    PCK measures the distance to the nearer of the segments gt_min -> gt and gt -> gt_max (calculate_pck_fixed_tolerance); the
    inference scripts' call with the degenerate streak (gt, gt, gt) and PCK@20 go through the same function.  Kept from the
    reference: `dist_streak` is distance_to_streak called as train.py:220 calls it, (pred, gt, gt_min, gt_max) into the signature
    (pred, r_min, r_b, r_max) -- the segments gt -> gt_min and gt_min -> gt_max; PCK is -1 and both distances are 10000 when their
    denominator is empty.  Not kept: an undetected sample is selected out of the distance sums rather than multiplied by 0."""
    tol, _ = _tolerances(tolerances)
    sums, counts = ball_metrics_device(pred_pos, gt_pos, gt_min, gt_max, vis, tol)
    return finish_ball(sums.cpu().numpy(), counts.cpu().numpy(), tol)


def table_val_metrics(pred_pos, gt_pos, tolerances=(2, 5, 10)):
    """The table val()'s metrics (tabledetection/train.py:180-187) in one launch.  pred_pos, gt_pos (N, K, 3) [x, y, visibility].
    -> {'pck@<t>' per tolerance and 'avg_dist' over the keypoints that are valid (prediction visibility == 1) and visible (gt
    visibility == 1), 'ratio_detected' (valid / all), and the counts 'number' (N K), 'valid', 'valid_visible', 'correct@<t>'}.
    As the reference: PCK -1 and avg_dist 10000 when no keypoint is valid; NaN (0 / 0) when some are valid and none of them visible."""
    tol, _ = _tolerances(tolerances)
    sums, counts = table_metrics_device(pred_pos, gt_pos, tol)
    return finish_table(sums.cpu().numpy(), counts.cpu().numpy(), tol)


def read_back(*tensors):
    """Device tensors (float64 / int64, counts far below 2^53) -> host float64 arrays of their shapes, in ONE copy."""
    flat = torch.cat([t.reshape(-1).to(torch.float64) for t in tensors]).cpu().numpy()
    out, at = [], 0
    for t in tensors:
        out.append(flat[at:at + t.numel()].reshape(tuple(t.shape)))
        at += t.numel()
    return out
