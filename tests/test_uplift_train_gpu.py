"""uplift.UpliftTrainer on the MI355X against K = 4 training steps of the reference (tests/golden/uplift_train_*.npz,
tools/make_goldens_uplift_train.py: its model, loss, clip_grad_norm_, torch.optim.Adam and update_ema on a different batch per
step).  The reference is never read here.

Bars: ten times the fixture's own stored self noise of the quantity (the reference run a second time with every batch reversed and
one thread; worst step / worst tensor), the gradient fixture's margin rule.  Per step loss_rot, loss_pos and the norm before
clipping; after the four steps, per tensor, the relative L2 of the CHANGE of the parameters since step 0, of exp_avg and of
exp_avg_sq, and of the EMA -- its change in the ema_decay 0.9 case, the full tensors in the 0.999 cases.

Measured on the MI355X, worst step / worst tensor, and the bar (= 10 x the stored self noise):
  case                   loss_rot         loss_pos         norm             param change     exp_avg          exp_avg_sq       ema
  global_ema999          7.6e-8 / 7.6e-7  0      / 1.5e-6  9.9e-8 / 6.6e-7  1.8e-3 / 4.3e-3  9.2e-7 / 4.6e-6  6.7e-7 / 7.2e-6  full   3.0e-8 / 7.9e-8
  local_ema900           8.9e-8 / 8.0e-7  2.4e-7 / 2.4e-6  1.1e-7 / 1.1e-6  9.6e-4 / 2.6e-3  1.1e-6 / 1.1e-5  7.6e-7 / 8.7e-6  change 1.3e-3 / 2.7e-3
  noclip_global_ema999   6.5e-8 / 6.0e-7  2.2e-7 / 2.9e-6  8.0e-8 / 1.9e-6  6.7e-4 / 3.5e-3  6.7e-7 / 5.7e-6  5.3e-7 / 7.5e-6  full   1.2e-8 / 1.0e-7
(every run prints its own.)  The third case reaches "clipping inactive" with max_norm 1e4: from random weights no
scaling of the targets brings the gradient norm under 5 (tools/make_goldens_uplift_train.py)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import has_gpu
from helpers import uplift_train_cases as C

pytestmark = pytest.mark.gpu
if has_gpu():
    from upliftingtabletennis_amd import _lib, inference, uplift, weights

FORWARD_BAR = 1e-4          # the uplift family test's bar
_RUNS = {}


def dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def make_trainer(c, sd=None, **kw):
    return uplift.UpliftTrainer(c.state_dict() if sd is None else sd, size=C.SIZE, lr=C.LR, betas=C.BETAS, eps=C.EPS, ema_decay=c.ema_decay, max_grad_norm=c.max_norm,
                                transform_mode=c.mode, max_batch=8, max_len=32, **kw)


def run(key):
    """The case's K steps through a trainer, once per session -> (case, trainer, per-step (loss_rot, loss_pos, norm))."""
    if key not in _RUNS:
        c = C.Case(key)
        tr = make_trainer(c)
        steps = []
        for k in range(C.STEPS):
            out = tr.step(*dev(c.inputs(k)))
            assert all(t.is_cuda and t.dim() == 0 for t in out)
            steps.append([float(t) for t in out])
        _RUNS[key] = (c, tr, np.array(steps, np.float64))
    return _RUNS[key]


def buffers(tr):
    """the four device buffers' bits, as one tensor each"""
    return [torch.cat([t.reshape(-1) for t in tr._read(w).values()]) for w in (_lib.OPT_PARAM, _lib.OPT_EMA, _lib.OPT_M, _lib.OPT_V)]


@pytest.mark.parametrize('key', sorted(C.EXPECTED))
def test_steps_match_the_reference(key):
    c, tr, steps = run(key)
    assert tr.steps == C.STEPS
    err = np.abs(steps - c.losses) / np.abs(c.losses)
    sd0 = c.state_dict()
    got = {'param': tr.state_dict(), 'ema': tr.state_dict(ema=True)}
    opt = tr.optimizer_state()
    assert opt['step'] == C.STEPS and sorted(opt['exp_avg']) == sorted(c.used) == sorted(opt['exp_avg_sq'])
    got['exp_avg'], got['exp_avg_sq'] = opt['exp_avg'], opt['exp_avg_sq']
    worst = {q: (0.0, None) for q in C.QUANTITIES}
    for q in C.QUANTITIES:
        ref = c.final(q)
        change = q == 'param' or (q == 'ema' and c.ema_decay < 0.99)
        for k in c.used:
            g = got[q][k].numpy()
            assert g.shape == ref[k].shape and np.isfinite(g).all(), (q, k)
            e = C.rel_l2(g - (sd0[k] if change else 0), ref[k] - (sd0[k] if change else 0))
            if e > worst[q][0]:
                worst[q] = (e, k)
    print('%s: loss_rot %.2e (bar %.2e), loss_pos %.2e (%.2e), norm %.2e (%.2e); ' % (key, err[:, 0].max(), c.bar('loss_rot'), err[:, 1].max(), c.bar('loss_pos'),
                                                                                       err[:, 2].max(), c.bar('norm'))
          + '; '.join('%s%s %.2e at %s (%.2e)' % (q, ' change' if q == 'param' or (q == 'ema' and c.ema_decay < 0.99) else '', worst[q][0], worst[q][1], c.bar(q))
                      for q in C.QUANTITIES))
    assert ((steps[:, 2] > c.max_norm).all() if c.clipped else (steps[:, 2] < c.max_norm).all())
    for i, q in enumerate(('loss_rot', 'loss_pos', 'norm')):
        assert err[:, i].max() <= c.bar(q), (q, err[:, i], c.bar(q))
    for q in C.QUANTITIES:
        assert worst[q][0] <= c.bar(q), (q, worst[q], c.bar(q))


@pytest.mark.parametrize('key', sorted(C.EXPECTED))
def test_exported_dicts_carry_the_untrained_tensors_within_the_reference_drift(key):
    """state_dict() has the reference's keys in its order; embed.* and inv_freq are the initial dict's -- equal to the reference's
    model, and within the stored drift of its EMA, which update_ema moves by rounding alone."""
    c, tr, _ = run(key)
    sd0 = c.state_dict()
    from upliftingtabletennis_amd import arch
    for ema in (False, True):
        sd = tr.state_dict(ema=ema)
        assert list(sd) == [k for k, _ in arch.uplift_schema(C.SIZE)]
        assert all(not t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == tuple(sd0[k].shape) for k, t in sd.items())
        for k in c.fixed:
            assert np.array_equal(sd[k].numpy(), sd0[k]), k
    ref = c.ema_fixed()
    sd = tr.state_dict(ema=True)
    assert max(float(np.abs((sd[k].numpy() - ref[k]) / ref[k]).max()) for k in c.fixed) <= c.drift * (1 + 1e-6)


def test_two_trainers_end_with_equal_bits_and_a_resumed_one_continues_them():
    c, tr, _ = run('local_ema900')
    other = make_trainer(c)
    for k in range(C.STEPS):
        other.step(*dev(c.inputs(k)), check_mask=False)
    for a, b in zip(buffers(tr), buffers(other)):
        assert torch.equal(a, b)
    # resume: parameters, EMA and optimizer state into a new trainer, then one more step on both
    resumed = make_trainer(c, sd=other.state_dict(), ema_state_dict=other.state_dict(ema=True))
    resumed.load_optimizer_state(other.optimizer_state())
    assert resumed.steps == C.STEPS
    for a, b in zip(buffers(other), buffers(resumed)):
        assert torch.equal(a, b)
    nxt = dev(C.step_inputs(c.seed, C.STEPS))
    out_a, out_b = other.step(*nxt), resumed.step(*nxt)
    assert all(torch.equal(x, y) for x, y in zip(out_a, out_b)) and other.steps == resumed.steps == C.STEPS + 1
    for a, b in zip(buffers(other), buffers(resumed)):
        assert torch.equal(a, b)


def test_inference_model_of_the_trainer_serves_the_trained_weights():
    """trainer.model(ema=False) is get_model on the exported dict, and its outputs are the forward outputs of the gradient pass on the
    trainer's next step (which reads the same weights in their plain form)."""
    c, _, _ = run('global_ema999')
    tr = make_trainer(c)
    tr.step(*dev(c.inputs(0)))
    inputs = dev(c.inputs(1))
    model = tr.model(ema=False)
    assert isinstance(model, uplift.MultiStageModel) and model is not tr._model
    rot, pos = model(*inputs[:4])
    rot2, pos2 = uplift.get_model('connectstage', C.SIZE, 'dynamic', 'new', state_dict=tr.state_dict(), max_batch=8, max_len=32)(*inputs[:4])
    keep = inputs[2] != 0
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())      # noqa: E731
    assert rel(rot, rot2) <= FORWARD_BAR and rel(pos[keep], pos2[keep]) <= FORWARD_BAR
    _, _, grads = tr._model.loss_and_grad(*inputs, transform_mode=c.mode)
    e_rot, e_pos = rel(rot, grads.rot), rel(pos[keep], grads.pos[keep])
    print('inference model against the gradient pass on the trained weights: rot %.2e pos %.2e' % (e_rot, e_pos))
    assert e_rot <= FORWARD_BAR and e_pos <= FORWARD_BAR
    ema = tr.model()          # the EMA's weights: after one step of decay 0.999 still close to, not equal to, the initial ones
    rot3, _ = ema(*inputs[:4])
    assert not torch.equal(rot3, rot) and bool(torch.isfinite(rot3).all())


def test_save_round_trips_through_the_checkpoint_loader(tmp_path):
    c, tr, _ = run('local_ema900')
    path = str(tmp_path / 'model.pt')
    tr.save(path, ema=True, epoch=7)
    d = torch.load(path, map_location='cpu', weights_only=True)
    assert sorted(d) == ['additional_info', 'identifier', 'model_state_dict'] and d['additional_info']['epoch'] == 7
    info = d['additional_info']
    assert (info['name'], info['size'], info['tabletoken_mode'], info['time_rotation'], info['transform_mode']) == ('connectstage', C.SIZE, 'dynamic', 'new', 'local')
    model, transform, transform_mode = inference.load_uplifting_model(path, max_batch=8, max_len=32)
    assert (model.name, model.mode, model.size, model.time_rotation, transform_mode) == ('connectstage', 'dynamic', C.SIZE, 'new', 'local')
    inputs = dev(c.inputs(0))
    rot, pos = model(*inputs[:4])
    rot2, pos2 = tr.model(ema=True)(*inputs[:4])
    assert torch.equal(rot, rot2) and torch.equal(pos, pos2)


def test_forward_on_a_trained_handle_is_refused():
    c, _, _ = run('global_ema999')
    tr = make_trainer(c)
    inputs = dev(c.inputs(0))
    rot0, pos0 = tr._model.forward(*inputs[:4])          # untrained: the private handle still serves
    tr.step(*inputs)
    rot = torch.full((C.BATCH, 3), 7.0, device='cuda')
    pos = torch.full((C.BATCH, C.T + C.PAD, 3), 7.0, device='cuda')
    lib = tr._lib
    rc = lib.ttup_uplift_forward(tr._model._handle, *[_lib.ptr(t) for t in inputs[:4]], C.BATCH, C.T + C.PAD, _lib.ptr(rot), _lib.ptr(pos), 1, _lib.stream_ptr())
    assert rc == _lib.ESTALE and b'stale' in lib.ttup_last_error() and b'trainer' in lib.ttup_last_error()
    torch.cuda.synchronize()
    assert bool((rot == 7.0).all()) and bool((pos == 7.0).all())          # it did not run
    with pytest.raises(RuntimeError, match='stale'):
        tr._model.forward(*inputs[:4])


def test_optimizer_refuses_other_variants_in_the_library_too():
    sd = weights.random_uplift_state_dict(5, 'small', 'multistage', 'stacked')
    model = uplift.MultiStageModel(sd, size='small', max_batch=4, max_len=32, name='multistage', mode='stacked')
    h = ctypes.c_void_p()
    assert model._lib.ttup_uplift_opt_create(model._handle, 1e-4, 0.9, 0.999, 1e-8, 0.999, 5.0, ctypes.byref(h)) == _lib.EINVAL
    assert b'connectstage/dynamic' in model._lib.ttup_last_error() and not h.value


def test_padded_time_steps_are_inert_through_a_step():
    c, _, _ = run('global_ema999')
    ball, table, mask, times, r_world, rotation = c.inputs(0)
    assert (mask == 0).any()
    ball2 = ball.copy()
    ball2[mask == 0] = 3.0e3
    a, b = make_trainer(c), make_trainer(c)
    out_a = a.step(*dev([ball, table, mask, times, r_world, rotation]))
    out_b = b.step(*dev([ball2, table, mask, times, r_world, rotation]))
    assert all(torch.equal(x, y) for x, y in zip(out_a, out_b))
    for x, y in zip(buffers(a), buffers(b)):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())


def test_closed_loop_from_generated_trajectories():
    """trajgen -> dataset.TableTennisDataset.batch -> three steps on the batch's own device tensors, without a host synchronisation
    in the step (check_mask=False)."""
    from upliftingtabletennis_amd import dataset, trajgen
    ds = dataset.TableTennisDataset('train', dataset.Compose([dataset.NormalizeImgCoords()]),
                                     trajectories=trajgen.get_valid_trajectories(16, 16, 'intermediate', 'left_to_right', as_numpy=False), seed=3)
    assert len(ds) == 16
    idx = np.arange(16)
    tr = uplift.UpliftTrainer(weights.random_uplift_state_dict(11, 'small'), size='small', max_batch=16, max_len=64)
    for k in range(3):
        b = ds.batch(idx, np.arange(16) + 100 * k)
        out = tr.step(b.r_img, b.table_img, b.mask, b.times, b.r_world, b.rotation, check_mask=False)
        assert all(bool(torch.isfinite(t)) for t in out), (k, out)
    assert tr.steps == 3
    for x in buffers(tr):
        assert bool(torch.isfinite(x).all())
