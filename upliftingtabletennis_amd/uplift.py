"""a6/a7: drop-in for the uplift network behind ``self.model(ball, table, mask, times) -> (rot, pos)``
(interface.py:235, inference/utils.py:254) and for ``transform_rotationaxes`` (uplifting/helper.py:394-420).
Reference models: everything uplifting/model.py:574-603 ``get_model`` builds -- SingleStageModel (:393-499) and MultiStageModel
(:502-571, 'multistage' / 'connectstage') with their table-token modes and both RoPE time conventions."""
import ctypes

import numpy as np
import torch

from . import _lib, arch, weights


class Gradients(dict):
    """Parameter name -> gradient view; `.flat` is the one device tensor they all view, `.rot` / `.pos` the forward outputs."""


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


class MultiStageModel:
    """One native handle for any variant (the class keeps the name of the shipped default's reference class)."""

    def __init__(self, state_dict, size='large', max_batch=64, max_len=128, device='cuda:0', name='connectstage', mode='dynamic', time_rotation='new'):
        arch.check_uplift_variant(name, size, mode, time_rotation)
        _lib.require_gpu()
        self.device = torch.device(device)
        self.size = size
        self.dim, self.depth, self.heads = arch.UPLIFT_SIZES[size]
        self.max_batch, self.max_len = int(max_batch), int(max_len)
        self.name, self.mode, self.time_rotation = name, mode, time_rotation
        self._lib = _lib.load()
        blob = weights.pack_uplift_blob(state_dict, size, name, mode, time_rotation)
        self._handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ttup_uplift_create(blob, len(blob), self.max_batch, self.max_len, ctypes.byref(self._handle)))

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def __del__(self):
        h, self._handle = getattr(self, '_handle', None), None
        if h:
            self._lib.ttup_uplift_destroy(h)

    def forward(self, ball_pos, table_pos, mask, times, check_mask=True):
        """ball (B,T,2), table (B,13,3), mask (B,T) in {0,1} with at least one 0, times (B,T) -> rot (B,3), pos (B,T,3).
        Raises ValueError for a mask that is not {0,1} with both values present (model.py:541-546), and -- before anything is
        launched -- for a T beyond max_len or beyond what the attention kernels serve (T + 1 <= 512 at `large`, 962 / 496 / 334 at
        `small` / `base` / `huge`)."""
        args = [t.to(self.device, torch.float32).contiguous() for t in (ball_pos, table_pos, mask, times)]
        ball, table, mask, times = args
        b, t, _ = ball.shape
        if table.shape != (b, 13, 3) or mask.shape != (b, t) or times.shape != (b, t):
            raise ValueError('inconsistent input shapes')
        if b == 0 or t == 0:      # the reference fails on mask.min() of an empty tensor (model.py:541)
            raise ValueError('empty batch: the uplift model needs at least one trajectory with one time step')
        rot = torch.empty((b, 3), dtype=torch.float32, device=self.device)
        pos = torch.empty((b, t, 3), dtype=torch.float32, device=self.device)
        self._forward_into(ball, table, mask, times, rot, pos, check_mask)
        return rot, pos

    __call__ = forward

    def _forward_into(self, ball, table, mask, times, rot, pos, check_mask):
        """The native forward on prepared device tensors, into caller-owned contiguous rot (b,3) / pos (b,t,3)."""
        b, t, _ = ball.shape
        with torch.cuda.device(self.device):
            rc = self._lib.ttup_uplift_forward(self._handle, _lib.ptr(ball), _lib.ptr(table), _lib.ptr(mask), _lib.ptr(times), b, t,
                                               _lib.ptr(rot), _lib.ptr(pos), 1 if check_mask else 0, _lib.stream_ptr())
        _lib.check(rc)

    def _predict(self, ball_pos, table_pos, mask, times, batch_size, check_mask):
        """`forward` in chunks of batch_size (default max_batch) into one prediction buffer -> ball, mask (device, fp32), rot, pos."""
        ball, table, mask, times = [t.to(self.device, torch.float32).contiguous() for t in (ball_pos, table_pos, mask, times)]
        if ball.dim() != 3:
            raise ValueError('inconsistent input shapes')
        n, t, _ = ball.shape
        if table.shape != (n, 13, 3) or mask.shape != (n, t) or times.shape != (n, t):
            raise ValueError('inconsistent input shapes')
        if n == 0 or t == 0:
            raise ValueError('empty batch: the uplift model needs at least one trajectory with one time step')
        step = self.max_batch if batch_size is None else int(batch_size)
        if not 1 <= step <= self.max_batch:
            raise ValueError('batch_size must be in [1, max_batch = %d], got %d' % (self.max_batch, step))
        rot = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        pos = torch.empty((n, t, 3), dtype=torch.float32, device=self.device)
        for i in range(0, n, step):
            j = min(n, i + step)
            self._forward_into(ball[i:j], table[i:j], mask[i:j], times[i:j], rot[i:j], pos[i:j], check_mask)
        return ball, mask, rot, pos

    def val(self, r_img, table_img, mask, times, r_world, rotation, transform_mode='global', batch_size=None, check_mask=True):
        """The reference's val() (uplifting/train.py:141-225) for one camera over a whole set: `forward` in chunks of batch_size
        (default max_batch) into one prediction buffer, then ONE metrics launch over all N samples -> the dict of `val_metrics`.
        The reference's return value is d['metric'].  Arguments: the fields of a reference batch (train.py:162) or of
        dataset.SampleBatch, by name.  Every variant get_model builds is served (only `forward` is called).
        With check_mask=False nothing synchronises with the host until the result is read (the mask check of `forward` reads one
        word back per chunk).  Bits depend on batch_size: the forward picks its kernels by batch size."""
        if transform_mode not in ('global', 'local'):
            raise ValueError("transform_mode should be 'global' or 'local'")
        _, mask_d, rot, pos = self._predict(r_img, table_img, mask, times, batch_size, check_mask)
        return val_metrics(rot, pos, r_world, rotation, mask_d, transform_mode)

    def val_real(self, r_img, table_img, mask, times, Mint, Mext, spin_class, transform_mode='global', batch_size=None, check_mask=True):
        """The reference's val_real() (uplifting/train.py:228-299) over a whole set, as `val` runs it -> the dict of
        `val_real_metrics`.  The reference's return pair is (d['metric_2D_normed'], d['macro_f1']).  Arguments: the fields of a
        RealInferenceDataset batch (train.py:247), by name; r_img normalised as the model takes it."""
        if transform_mode not in ('global', 'local'):
            raise ValueError("transform_mode should be 'global' or 'local'")
        ball_d, mask_d, rot, pos = self._predict(r_img, table_img, mask, times, batch_size, check_mask)
        return val_real_metrics(rot, pos, ball_d, mask_d, Mint, Mext, spin_class, transform_mode)

    def grad_layout(self):
        """[(parameter name, shape, offset, used)] and the length of the flat gradient buffer `loss_and_grad` fills
        (arch.uplift_grad_layout; checked against the library's own ttup_uplift_grad_layout)."""
        arch.check_uplift_grad_variant(self.name, self.mode)
        layout, n = arch.uplift_grad_layout(self.size)
        nf, nt = ctypes.c_longlong(0), ctypes.c_int(0)
        offs, used = (ctypes.c_longlong * len(layout))(), (ctypes.c_int * len(layout))()
        _lib.check(self._lib.ttup_uplift_grad_layout(self._handle, ctypes.byref(nf), ctypes.byref(nt), offs, used, len(layout)))
        if (nf.value, nt.value, list(offs), [bool(u) for u in used]) != (n, len(layout), [e[2] for e in layout], [e[3] for e in layout]):
            raise RuntimeError('the library lays the gradient buffer out differently from arch.uplift_grad_layout')
        return layout, n

    def loss_and_grad(self, ball_pos, table_pos, mask, times, r_world, rotation, transform_mode='global', check_mask=True):
        """The reference's training loss (uplifting/train.py:121-127) and `loss.backward()` for one batch.
        ball (B,T,2), table (B,13,3), mask (B,T) in {0,1}, times (B,T), r_world (B,T,3), rotation (B,3) -- the rows `r_img, table_img,
        mask, r_world, rotation, times` of a reference batch (train.py:116) or of dataset.TableTennisDataset.batch, passed by name.
        transform_mode 'local' first takes the target spin through transform_rotationaxes(rotation, r_world) (train.py:123-124).
        -> (loss_rot, loss_pos, grads): two 0-d device tensors and a dict from the reference's parameter names to views into one flat
        device tensor (`grads.flat`; `grad_layout()` has the offsets).  `grads.rot` / `grads.pos` are the forward outputs.
        Raises ValueError for any variant but connectstage/dynamic before the library is asked, and -- as `forward` does, and as the
        reference's training step does through model.forward (model.py:541-546) -- for a mask that is not {0,1} with both values
        present.  That check reads one word back and synchronises the stream once; check_mask=False skips both."""
        arch.check_uplift_grad_variant(self.name, self.mode)
        if transform_mode not in ('global', 'local'):
            raise ValueError("transform_mode should be 'global' or 'local'")
        args = [t.to(self.device, torch.float32).contiguous() for t in (ball_pos, table_pos, mask, times, r_world, rotation)]
        ball, table, mask, times, r_world, rotation = args
        b, t, _ = ball.shape
        if table.shape != (b, 13, 3) or mask.shape != (b, t) or times.shape != (b, t) or r_world.shape != (b, t, 3) or rotation.shape != (b, 3):
            raise ValueError('inconsistent input shapes')
        if b == 0 or t == 0:
            raise ValueError('empty batch: the uplift model needs at least one trajectory with one time step')
        layout, n = self.grad_layout()
        with torch.cuda.device(self.device):
            nbytes = int(self._lib.ttup_uplift_grad_workspace_bytes(self._handle, b, t))
            ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=self.device)
            flat = torch.empty((n,), dtype=torch.float32, device=self.device)
            loss = torch.empty((2,), dtype=torch.float32, device=self.device)
            rot = torch.empty((b, 3), dtype=torch.float32, device=self.device)
            pos = torch.empty((b, t, 3), dtype=torch.float32, device=self.device)
            rc = self._lib.ttup_uplift_loss_grad(self._handle, _lib.ptr(ball), _lib.ptr(table), _lib.ptr(mask), _lib.ptr(times), _lib.ptr(r_world),
                                                 _lib.ptr(rotation), b, t, (1 if transform_mode == 'local' else 0) | (2 if check_mask else 0), _lib.ptr(ws), nbytes,
                                                 _lib.ptr(flat), _lib.ptr(loss), _lib.ptr(rot), _lib.ptr(pos), _lib.stream_ptr())
        _lib.check(rc)
        grads = Gradients((k, flat[off:off + _numel(shape)].view(shape)) for k, shape, off, _ in layout)
        grads.flat, grads.rot, grads.pos = flat, rot, pos
        return loss[0], loss[1], grads

    def graph_info(self):
        """{'graphs', 'off', 'replays', 'stage_launches'}: the small-batch path (hipGraph replay of a captured forward; all layers
        of a stage in one stage_x3_kernel launch, csrc/uplift_stage.h)."""
        out = (ctypes.c_int * 3)()
        _lib.check(self._lib.ttup_uplift_graph_info(self._handle, out))
        st = ctypes.c_longlong(0)
        _lib.check(self._lib.ttup_uplift_stage_info(self._handle, ctypes.byref(st)))
        return {'graphs': int(out[0]), 'off': bool(out[1]), 'replays': int(out[2]), 'stage_launches': int(st.value)}


class UpliftTrainer:
    """The reference's training step (uplifting/train.py:113-132) on the device: `loss_and_grad`, then gradient clipping, torch.optim.Adam
    and the EMA of the weights in one native step (csrc/uplift_opt.hip).  Defaults: uplifting/config.py and train.py:73, :129.

    It owns a private MultiStageModel whose plain fp32 weights the step updates in place; that model's packed forward weights go
    stale with the first step, so it is never handed out: `model()` builds a fresh inference model from the current weights
    (parameters -> host -> weights.pack_uplift_blob -> ttup_uplift_create, the route every model takes).  `ema_state_dict` starts the
    EMA from other weights than `state_dict` (resume); by default it is a copy, as train.py:58.
    Only connectstage/dynamic is trained (arch.UPLIFT_GRAD_VARIANT): `name` / `mode` exist so that another variant is refused with
    a ValueError before the native library is touched, as loss_and_grad refuses it.
    Evaluation is MultiStageModel.val / .val_real on `model()`, checkpoint selection is CheckpointSelector.  Not here: the epoch loop."""

    def __init__(self, state_dict, size='large', time_rotation='new', lr=1e-4, betas=(0.9, 0.999), eps=1e-8, ema_decay=0.999, max_grad_norm=5.0,
                 transform_mode='global', max_batch=64, max_len=128, device='cuda:0', ema_state_dict=None, name='connectstage', mode='dynamic'):
        arch.check_uplift_variant(name, size, mode, time_rotation)
        arch.check_uplift_grad_variant(name, mode)
        if transform_mode not in ('global', 'local'):
            raise ValueError("transform_mode should be 'global' or 'local'")
        self.size, self.time_rotation, self.transform_mode = size, time_rotation, transform_mode
        self.hyper = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), ema_decay=float(ema_decay), max_grad_norm=float(max_grad_norm))
        self._model = MultiStageModel(state_dict, size=size, max_batch=max_batch, max_len=max_len, device=device, time_rotation=time_rotation)
        self.device, self._lib = self._model.device, self._model._lib
        self._layout, self._n = self._model.grad_layout()
        # what no step changes: the embed.* tensors (held, never read: no gradient, so Adam skips them) and the inv_freq buffers
        self._fixed = {k: torch.as_tensor(weights._np(state_dict[k])).clone() for k, _ in arch.uplift_schema(size)
                       if k.endswith('.inv_freq') or k.startswith('embed.')}
        self._opt = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ttup_uplift_opt_create(self._model._handle, self.hyper['lr'], *self.hyper['betas'], self.hyper['eps'], self.hyper['ema_decay'],
                                                        self.hyper['max_grad_norm'], ctypes.byref(self._opt)))
        if ema_state_dict is not None:
            self._load(_lib.OPT_EMA, ema_state_dict)

    def __del__(self):
        h, self._opt = getattr(self, '_opt', None), None
        if h:
            self._lib.ttup_uplift_opt_destroy(h)          # before the model's handle, which it points to
        self._model = None

    def step(self, ball_pos, table_pos, mask, times, r_world, rotation, check_mask=True):
        """One training step on a batch (arguments as MultiStageModel.loss_and_grad) -> (loss_rot, loss_pos, grad_norm): 0-d device
        tensors, the losses of the weights BEFORE the step and the gradient's total norm before clipping.  Everything runs on the
        current stream; with check_mask=False nothing synchronises with the host."""
        loss_rot, loss_pos, grads = self._model.loss_and_grad(ball_pos, table_pos, mask, times, r_world, rotation, self.transform_mode, check_mask)
        norm = torch.empty((1,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ttup_uplift_opt_step(self._opt, _lib.ptr(grads.flat), _lib.ptr(norm), _lib.stream_ptr()))
        return loss_rot, loss_pos, norm[0]

    @property
    def steps(self):
        n = ctypes.c_longlong(0)
        _lib.check(self._lib.ttup_uplift_opt_get_step(self._opt, ctypes.byref(n)))
        return int(n.value)

    def _read(self, which):
        """One of the four device buffers in gradient-layout order -> {parameter name: CPU tensor} (embed.* slots: zeros)."""
        flat = torch.empty((self._n,), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ttup_uplift_opt_read(self._opt, which, _lib.ptr(flat), _lib.stream_ptr()))
        flat = flat.cpu()
        return {k: flat[off:off + _numel(shape)].view(shape).clone() for k, shape, off, _ in self._layout}

    def _load(self, which, tensors):
        flat = torch.zeros((self._n,), dtype=torch.float32)
        for k, shape, off, used in self._layout:
            if used:
                t = torch.as_tensor(weights._np(tensors[k]), dtype=torch.float32)
                if tuple(t.shape) != tuple(shape):
                    raise ValueError('%s: expected shape %s, got %s' % (k, tuple(shape), tuple(t.shape)))
                flat[off:off + _numel(shape)] = t.reshape(-1)
        flat = flat.to(self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.ttup_uplift_opt_load(self._opt, which, _lib.ptr(flat), _lib.stream_ptr()))
            torch.cuda.current_stream().synchronize()          # `flat` dies with this call

    def state_dict(self, ema=False):
        """The reference's names -> CPU tensors, in its order: loadable strict=True by get_model('connectstage', size, 'dynamic', .).
        embed.* and the inv_freq buffers are the initial dict's, for the EMA too (the reference's update_ema moves them
        by rounding alone)."""
        got = self._read(_lib.OPT_EMA if ema else _lib.OPT_PARAM)
        return {k: (self._fixed[k].clone() if k in self._fixed else got[k]) for k, _ in arch.uplift_schema(self.size)}

    def model(self, ema=True, **kw):
        """A fresh MultiStageModel for inference on the current (EMA) weights, packed on the host like any other model."""
        kw = dict(dict(max_batch=self._model.max_batch, max_len=self._model.max_len, device=self.device), **kw)
        return MultiStageModel(self.state_dict(ema), size=self.size, time_rotation=self.time_rotation, **kw)

    def optimizer_state(self):
        """{'step', 'exp_avg': {name: tensor}, 'exp_avg_sq': {name: tensor}} of the parameters Adam holds state for (not embed.*)."""
        used = [k for k, _, _, u in self._layout if u]
        m, v = self._read(_lib.OPT_M), self._read(_lib.OPT_V)
        return {'step': self.steps, 'exp_avg': {k: m[k] for k in used}, 'exp_avg_sq': {k: v[k] for k in used}}

    def load_optimizer_state(self, state):
        self._load(_lib.OPT_M, state['exp_avg'])
        self._load(_lib.OPT_V, state['exp_avg_sq'])
        _lib.check(self._lib.ttup_uplift_opt_set_step(self._opt, int(state['step'])))

    def save(self, path, ema=True, epoch=0):
        """Write the reference's checkpoint format (uplifting/helper.py:371-391 save_model): what inference.load_uplifting_model and
        interface.UpliftingModel(model_path=...) open, and the reference's own inference_uplifting.load_model."""
        h = self.hyper
        info = {'epoch': int(epoch), 'lr': h['lr'], 'name': 'connectstage', 'size': self.size, 'ema_decay': h['ema_decay'], 'tabletoken_mode': 'dynamic',
                'time_rotation': self.time_rotation, 'transform_mode': self.transform_mode}
        ident = 'lr:%.2e_name:connectstage_mode:dynamic_size:%s_tr:%s_trans:%s' % (h['lr'], self.size, self.time_rotation, self.transform_mode)
        torch.save({'model_state_dict': self.state_dict(ema), 'identifier': ident, 'additional_info': info}, path)


def get_model(name='connectstage', size='large', mode='dynamic', time_rotation='new', state_dict=None, **kw):
    """Mirror of uplifting/model.py:574-603: every (name, size, mode, time_rotation) the reference builds, and its AssertionError /
    ValueError for the rest -- raised before the native library is touched."""
    arch.check_uplift_variant(name, size, mode, time_rotation)
    if state_dict is None:
        raise ValueError('a state_dict is required (no weights can be downloaded offline)')
    return MultiStageModel(state_dict, size=size, name=name, mode=mode, time_rotation=time_rotation, **kw)


def transform_rotationaxes(rotation, r_gt):
    """uplifting/helper.py:394-420: spin from the global frame into the ball-local frame.  (B,3),(B,T,3) or (3,),(T,3)."""
    _lib.require_gpu()
    lib = _lib.load()
    single = rotation.dim() == 1
    if r_gt.dim() not in (2, 3):
        raise ValueError('Shape not supported.')
    rot = (rotation[None] if single else rotation).to(torch.float32).contiguous()
    pos = (r_gt[None] if single else r_gt).to(torch.float32).contiguous()
    if not rot.is_cuda:
        rot, pos = rot.cuda(), pos.cuda()
    out = torch.empty_like(rot)
    with torch.cuda.device(rot.device):
        _lib.check(lib.ttup_transform_rotationaxes(_lib.ptr(rot), _lib.ptr(pos), rot.shape[0], pos.shape[1], _lib.ptr(out), _lib.stream_ptr()))
    return out[0] if single else out


# ---------------------------------------------------------------------------------------------------- evaluation
WIDTH, HEIGHT = 2560, 1440            # uplifting/helper.py:26 -- the image val_real measures in, not glue.py's 1920 x 1080
TOPSPIN_CLASS, BACKSPIN_CLASS = 1, 2  # uplifting/data.py
_VAL_SUMS = ('metric', 'metric_x', 'metric_y', 'metric_z', 'metric_abs', 'metric_angle', 'metric_position')


def _eval_inputs(tensors, device=None):
    """fp32, contiguous, on one HIP device (that of the first tensor that already lives on one)."""
    ts = [torch.as_tensor(t) for t in tensors]
    if device is None:
        device = next((t.device for t in ts if t.is_cuda), torch.device('cuda', torch.cuda.current_device()))
    return [t.to(device, torch.float32).contiguous() for t in ts], device


def _eval_mode(transform_mode):
    if transform_mode not in ('global', 'local'):
        raise ValueError("transform_mode should be 'global' or 'local'")
    return 1 if transform_mode == 'global' else 0


def val_metrics(pred_rotation, pred_position, r_world, rotation, mask, transform_mode='global'):
    """The metrics of the reference's val() (uplifting/train.py:166-195) over N samples in one launch (csrc/uplift_eval.hip).
    pred_rotation (N,3), pred_position (N,T,3), r_world (N,T,3), rotation (N,3), mask (N,T) in {0,1}; T >= 2.  The target spin goes
    through transform_rotationaxes(rotation, r_world); with transform_mode 'global' the predicted spin does too.
    -> {'metric', 'metric_x', 'metric_y', 'metric_z', 'metric_abs', 'metric_angle', 'metric_position', 'mse': float (sums over the
    samples divided by N, as the reference), 'accuracy': float64 (3), 'TP', 'TN', 'FP', 'FN': int64 (3), 'number': N}.
    fp32 inputs, fp64 arithmetic and sums, a fixed summation tree: two calls return the same bits.  Reading the result is the one
    host synchronisation.

    Kept from the reference: TP / TN / FP / FN are helper.binary_metrics called as train.py:181 calls it, with the prediction in
    the `rot_gt` slot: FP counts prediction < 0 with target > 0, FN prediction > 0 with target < 0 (swapped relative to the names).
    A sample whose first two r_world positions coincide in x and y has a NaN local frame (0 / 0): `metric`, `metric_x`, `metric_y`,
    `metric_abs`, `metric_angle` and `mse` become NaN, `metric_z` (e_z needs no frame) and `metric_position` do not.
    Not kept: the `val{cam}/loss` tag is not reproduced -- the reference overwrites `loss` with every batch and divides the LAST
    batch's MSE by N (train.py:173, :184); `mse` is the mean squared error over all samples and components.  A time step with
    mask == 0 is selected out rather than multiplied by 0 (differs only where a masked slot holds a non-finite value).  The cosine
    is clamped to [-1, 1] before acos (the reference returns NaN when fp32 rounding pushes it past 1)."""
    glob = _eval_mode(transform_mode)
    _lib.require_gpu()
    lib = _lib.load()
    (rot, pos, rw, gt, m), dev = _eval_inputs((pred_rotation, pred_position, r_world, rotation, mask))
    if pos.dim() != 3 or pos.shape[2] != 3:
        raise ValueError('inconsistent input shapes')
    n, t, _ = pos.shape
    if rot.shape != (n, 3) or rw.shape != (n, t, 3) or gt.shape != (n, 3) or m.shape != (n, t):
        raise ValueError('inconsistent input shapes')
    with torch.cuda.device(dev):
        nbytes = int(lib.ttup_uplift_eval_workspace_bytes(n))
        ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=dev)
        sums = torch.empty((8,), dtype=torch.float64, device=dev)
        counts = torch.empty((13,), dtype=torch.int64, device=dev)
        _lib.check(lib.ttup_uplift_val_metrics(_lib.ptr(rot), _lib.ptr(pos), _lib.ptr(rw), _lib.ptr(gt), _lib.ptr(m), n, t, glob, _lib.ptr(ws), nbytes,
                                               _lib.ptr(sums), _lib.ptr(counts), _lib.stream_ptr()))
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
    number = int(counts[12])
    out = {k: float(sums[i] / number) for i, k in enumerate(_VAL_SUMS)}
    out['mse'] = float(sums[7] / (3 * number))
    tp, tn, fp, fn = (counts[3 * i:3 * i + 3].copy() for i in range(4))
    with np.errstate(invalid='ignore', divide='ignore'):
        out['accuracy'] = (tp + tn) / (tp + tn + fp + fn).astype(np.float64)
    out.update(TP=tp, TN=tn, FP=fp, FN=fn, number=number)
    return out


def roc_auc(labels, scores):
    """sklearn.metrics.roc_auc_score(labels, scores) for binary labels in {0, 1}: the rank statistic with average ranks for ties
    (Mann-Whitney U / (n_pos n_neg)), in numpy.  ValueError for a single class, as roc_auc_score raises, and for a NaN score."""
    y, s = np.asarray(labels).astype(bool).ravel(), np.asarray(scores, np.float64).ravel()
    if y.shape != s.shape:
        raise ValueError('labels and scores differ in length')
    if np.isnan(s).any():
        raise ValueError('Input contains NaN.')
    n_pos = int(y.sum())
    n_neg = int(y.size - n_pos)
    if n_pos == 0 or n_neg == 0:
        raise ValueError('Only one class present in y_true. ROC AUC score is not defined in that case.')
    order = np.argsort(s, kind='mergesort')
    ss = s[order]
    first = np.r_[True, ss[1:] != ss[:-1]]                      # start of each run of equal scores
    start = np.flatnonzero(first)
    end = np.r_[start[1:], ss.size]
    avg = (start + 1 + end) / 2.0                                # mean of the 1-based ranks start+1 .. end
    ranks = np.empty(ss.size, np.float64)
    ranks[order] = np.repeat(avg, end - start)
    return float((ranks[y].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def val_real_metrics(pred_rotation, pred_position, r_img, mask, Mint, Mext, spin_class, transform_mode='global'):
    """The metrics of the reference's val_real() (uplifting/train.py:250-297) over N samples in one launch.
    pred_rotation (N,3), pred_position (N,T,3), r_img (N,T,2) normalised image coordinates (what the model is fed), mask (N,T),
    Mint (N,3,3), Mext (N,4,4) per sample, spin_class (N) integers (1 topspin, 2 backspin, 0 not annotated); T >= 2.
    With transform_mode 'global' the predicted spin goes through transform_rotationaxes(pred_rotation, pred_position) -- the
    PREDICTED positions (train.py:253).  The 2-D metric is the masked mean distance, in pixels of the 2560 x 1440 image of
    uplifting/helper.py, between cam2img(world2cam(pred_position, Mext), Mint) and r_img * (WIDTH, HEIGHT).
    -> {'metric_2D', 'metric_2D_normed', 'accuracy', 'macro_f1', 'roc_auc': float, 'TP', 'TN', 'FP', 'FN': int, 'scores': float64 (A),
    'labels': int64 (A) of the A annotated samples in order (score = local spin component 1, label 1 = topspin), 'number': N}.
    The ratios are the reference's own expressions on Python ints, in its order, so its errors come out too: ZeroDivisionError with
    no annotated sample (and wherever one of its F1 denominators is 0), then roc_auc's ValueError with a single class present.
    The device part (`val_real_counts`) is fp64 with a fixed summation tree (two calls return the same bits); the AUC is computed
    on the host."""
    out = val_real_counts(pred_rotation, pred_position, r_img, mask, Mint, Mext, spin_class, transform_mode)
    TP, TN, FP, FN = out['TP'], out['TN'], out['FP'], out['FN']
    out['accuracy'] = (TP + TN) / (TP + TN + FP + FN)          # train.py:287-291, in its order
    f1_plus = 2 * TP / (2 * TP + FP + FN)
    f1_minus = 2 * TN / (2 * TN + FN + FP)
    out['macro_f1'] = (f1_plus + f1_minus) / 2
    out['roc_auc'] = roc_auc(out['labels'], out['scores'])
    return out


def val_real_counts(pred_rotation, pred_position, r_img, mask, Mint, Mext, spin_class, transform_mode='global'):
    """What the device computes of `val_real_metrics` (same arguments), without the ratios and their errors:
    {'metric_2D', 'metric_2D_normed', 'TP', 'TN', 'FP', 'FN', 'scores', 'labels', 'number'}."""
    glob = _eval_mode(transform_mode)
    _lib.require_gpu()
    lib = _lib.load()
    (rot, pos, img, m, mint, mext), dev = _eval_inputs((pred_rotation, pred_position, r_img, mask, Mint, Mext))
    if pos.dim() != 3 or pos.shape[2] != 3:
        raise ValueError('inconsistent input shapes')
    n, t, _ = pos.shape
    cls = torch.as_tensor(spin_class).to(dev, torch.int32).contiguous()
    if rot.shape != (n, 3) or img.shape != (n, t, 2) or m.shape != (n, t) or mint.shape != (n, 3, 3) or mext.shape != (n, 4, 4) or cls.shape != (n,):
        raise ValueError('inconsistent input shapes')
    with torch.cuda.device(dev):
        nbytes = int(lib.ttup_uplift_eval_workspace_bytes(n))
        ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.float64, device=dev)
        sums = torch.empty((1,), dtype=torch.float64, device=dev)
        counts = torch.empty((5,), dtype=torch.int64, device=dev)
        scores = torch.empty((max(n, 1),), dtype=torch.float64, device=dev)
        labels = torch.empty((max(n, 1),), dtype=torch.int32, device=dev)
        _lib.check(lib.ttup_uplift_val_real_metrics(_lib.ptr(rot), _lib.ptr(pos), _lib.ptr(img), _lib.ptr(m), _lib.ptr(mint), _lib.ptr(mext), _lib.ptr(cls), n, t,
                                                    glob, _lib.ptr(ws), nbytes, _lib.ptr(sums), _lib.ptr(counts), _lib.ptr(scores), _lib.ptr(labels),
                                                    _lib.stream_ptr()))
    sums, counts, scores, labels = sums.cpu().numpy(), counts.cpu().numpy(), scores.cpu().numpy(), labels.cpu().numpy().astype(np.int64)
    TP, TN, FP, FN, number = (int(c) for c in counts)
    keep = labels >= 0
    scores, labels = scores[keep], labels[keep]
    metric_2D = float(sums[0] / number)
    return {'metric_2D': metric_2D, 'metric_2D_normed': metric_2D / (WIDTH ** 2 + HEIGHT ** 2) ** 0.5, 'TP': TP, 'TN': TN, 'FP': FP, 'FN': FN,
            'scores': scores, 'labels': labels, 'number': number}


class CheckpointSelector:
    """Which checkpoint files the reference's epoch loop writes after an epoch (uplifting/train.py:75-102), as host logic.
    `update(metric_trajectory, metric_spin, metric_synthetic)` takes val_real's return pair (d['metric_2D_normed'], d['macro_f1'])
    and val's return value (d['metric']) and returns, in the reference's order, the names among 'model_trajectory.pt',
    'model_spin.pt', 'model_synthetic.pt', 'model.pt' to write this epoch; the caller writes them with
    UpliftTrainer.save(path, ema=True, epoch=e)."""

    def __init__(self, threshold_trajectory_metric=0.007):
        self.threshold_trajectory_metric = threshold_trajectory_metric
        self.best_metric_trajectory, self.best_metric_spin, self.best_metric_synthetic = 1e8, 0, 1e8
        self.best_metric_spin_mixed, self.best_metric_trajectory_mixed = 0, 1e8

    def update(self, metric_trajectory, metric_spin, metric_synthetic):
        names = []
        if metric_trajectory < self.best_metric_trajectory:
            self.best_metric_trajectory = metric_trajectory
            names.append('model_trajectory.pt')
        if metric_spin >= self.best_metric_spin:          # larger F1 is better; a tie saves again
            self.best_metric_spin = metric_spin
            names.append('model_spin.pt')
        if metric_synthetic < self.best_metric_synthetic:
            self.best_metric_synthetic = metric_synthetic
            names.append('model_synthetic.pt')
        if metric_trajectory <= self.threshold_trajectory_metric:
            if metric_spin > self.best_metric_spin_mixed:
                self.best_metric_spin_mixed = metric_spin
                names.append('model.pt')
                self.best_metric_trajectory_mixed = metric_trajectory          # the value of the saved model
            elif metric_spin == self.best_metric_spin_mixed:          # 100 % is realistic: decide by the trajectory metric
                if metric_trajectory < self.best_metric_trajectory_mixed:
                    self.best_metric_trajectory_mixed = metric_trajectory
                    names.append('model.pt')
        return tuple(names)
