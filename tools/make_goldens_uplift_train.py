#!/usr/bin/env python3
"""Generate tests/golden/uplift_train_<case>_{pe,mv}.npz: K = 4 training steps of the REFERENCE -- get_model('connectstage', 'small',
'dynamic', 'new') in .train() mode, the loss of uplifting/train.py:121-127, loss.backward(), clip_grad_norm_(model.parameters(), 5.0),
torch.optim.Adam(lr=1e-4).step(), update_ema(model, model_ema, ema_decay) (train.py:56-58, :73, :128-132) -- from
weights.random_uplift_state_dict, on a DIFFERENT batch per step (tests/helpers/uplift_train_cases.py: step_inputs; B = 3, T = 17 + 3 pad).

Runs only where the reference sources are (TTUP_REFERENCE); the tests read the files alone.  Cases (uplift_train_cases.EXPECTED):
  global_ema999          transform_mode 'global', ema_decay 0.999 (the reference's configuration); clipping active at every step
  local_ema900           'local', ema_decay 0.9: the EMA's change over four steps is then far above fp32 rounding of the EMA itself
  noclip_global_ema999   as the first with clip_grad_norm_(., 1e4): the norm stays below the threshold, clipping inactive at every step.
                         (Scaling the targets cannot do that from random weights: the spin loss is a sum of vector LENGTHS, whose
                         gradient does not shrink with the targets -- 16 to 60 on these seeds -- and the position loss's gradient is
                         dominated by the untrained model's own output, 300 to 400, whatever the targets are.)

Stored per case (_pe: param, ema and everything small; _mv: exp_avg, exp_avg_sq -- four full buffers pass 1 MiB):
  seed; steps (K,3) loss_rot, loss_pos, the norm clip_grad_norm_ returns, per step; relu_margin (K,);
  param, ema, exp_avg, exp_avg_sq: the final tensors, flat in arch.uplift_grad_layout order (embed.* slots zero);
  ema_fixed/<name>: the reference's final EMA of embed.* and the inv_freq buffers, which update_ema runs alpha x + (1 - alpha) x over;
  drift: the largest relative distance of those from their initial values (rounding alone);
  self_noise_steps (K,3) and self_noise_<quantity> (per tensor): relative distance to a second run of the same K steps with every
  batch reversed and one thread -- for param and, in the ema_decay 0.9 case, ema the relative L2 of the CHANGE since step 0.

Conditions, ASSERTED here from the reference's numbers alone (a seed that misses one moves on by SEED_STEP):
  * the ReLU-kink condition of tools/make_goldens_uplift_grad.py at every step;
  * self noise under uplift_train_cases.NOISE_CEILING for every quantity;
  * clipping active (norm > max_norm) at every step of the first two cases, inactive (norm < max_norm) at every step of the third;
  * drift <= 2 K fp32 ulps.

    python tools/make_goldens_uplift_train.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TTUP_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from helpers import uplift_train_cases as C  # noqa: E402
from make_goldens_uplift_grad import RELU_MARGIN, SEED_STEP, SEED_TRIES, relu_inputs  # noqa: E402
from upliftingtabletennis_amd import arch, weights  # noqa: E402

FIRST_SEED = {'global_ema999': 700, 'local_ema900': 701, 'noclip_global_ema999': 702}


def run_reference(ref, sd, seed, mode, ema_decay, max_norm, reverse):
    """-> (steps (K,3), relu margins (K,), model, model_ema, optimizer) after K steps of train.py's loop body"""
    get_model, transform_rotationaxes, update_ema = ref
    load = lambda: {k: torch.from_numpy(v.copy()) for k, v in sd.items()}      # noqa: E731
    model, model_ema = get_model('connectstage', C.SIZE, 'dynamic', 'new'), get_model('connectstage', C.SIZE, 'dynamic', 'new')
    model.load_state_dict(load(), strict=True)
    model_ema = update_ema(model, model_ema, 0)
    optimizer = torch.optim.Adam(model.parameters(), lr=C.LR)
    assert (optimizer.defaults['betas'], optimizer.defaults['eps']) == (C.BETAS, C.EPS)
    margins = {}

    def hook(name):
        def f(mod, args, y):
            with torch.no_grad():
                s = args[0].abs() @ mod.weight.abs().T + mod.bias.abs()
                margins[name] = min(margins.get(name, np.inf), float((y.abs() / s).min()))
        return f
    for name, m in relu_inputs(model):
        m.register_forward_hook(hook(name))
    loss_fn = lambda angle, pred_angle: torch.sum(torch.sqrt(torch.sum((angle - pred_angle) ** 2, dim=1)))      # noqa: E731  (train.py:107)
    model.train()
    steps, relu = [], []
    for k in range(C.STEPS):
        r_img, table_img, mask, times, r_world, rotation = [torch.from_numpy(a[::-1].copy() if reverse else a) for a in C.step_inputs(seed, k)]
        margins.clear()
        optimizer.zero_grad()
        pred_rotation, pred_position = model(r_img, table_img, mask, times)
        if mode == 'local':
            rotation = transform_rotationaxes(rotation, r_world)
        loss_rot = loss_fn(pred_rotation, rotation)
        loss_pos = torch.sum(torch.nn.functional.mse_loss(pred_position, r_world, reduction='none') * mask.unsqueeze(-1)) / torch.sum(mask)
        loss = loss_rot + loss_pos
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
        optimizer.step()
        model_ema = update_ema(model, model_ema, ema_decay)
        steps.append([loss_rot.item(), loss_pos.item(), norm.item()])
        relu.append(min(margins.values()))
    return np.array(steps, np.float64), np.array(relu), model, model_ema, optimizer


def buffers(model, model_ema, optimizer):
    """{quantity: {name: array}} over the parameters Adam holds state for"""
    params = dict(model.named_parameters())
    out = {'param': {}, 'ema': {}, 'exp_avg': {}, 'exp_avg_sq': {}}
    ema = dict(model_ema.named_parameters())
    for k, p in params.items():
        if p in optimizer.state:
            out['param'][k], out['ema'][k] = p.detach().numpy().copy(), ema[k].detach().numpy().copy()
            out['exp_avg'][k], out['exp_avg_sq'][k] = optimizer.state[p]['exp_avg'].numpy().copy(), optimizer.state[p]['exp_avg_sq'].numpy().copy()
    return out


def main():
    import make_goldens
    make_goldens.install_stubs()
    from uplifting.helper import transform_rotationaxes, update_ema
    from uplifting.model import get_model
    ref = (get_model, transform_rotationaxes, update_ema)
    threads = min(16, os.cpu_count() or 1)
    layout, n = arch.uplift_grad_layout(C.SIZE)
    for key, (mode, ema_decay, max_norm, clipped) in C.EXPECTED.items():
        for seed in range(FIRST_SEED[key], FIRST_SEED[key] + SEED_STEP * SEED_TRIES, SEED_STEP):
            sd = weights.random_uplift_state_dict(seed, C.SIZE)
            torch.set_num_threads(threads)
            steps, relu, model, model_ema, opt = run_reference(ref, sd, seed, mode, ema_decay, max_norm, False)
            torch.set_num_threads(1)
            steps2, _, model2, model_ema2, opt2 = run_reference(ref, sd, seed, mode, ema_decay, max_norm, True)
            a, b = buffers(model, model_ema, opt), buffers(model2, model_ema2, opt2)
            used = [k for k, _, _, u in layout if u]
            assert sorted(a['param']) == sorted(used), 'Adam holds state for other parameters than arch.uplift_grad_layout marks used'
            noise_steps = np.abs(steps2 - steps) / np.abs(steps)
            noise = {}
            for q in C.QUANTITIES:
                change = q == 'param' or (q == 'ema' and ema_decay < 0.99)
                noise[q] = np.array([C.rel_l2(b[q][k] - (sd[k] if change else 0), a[q][k] - (sd[k] if change else 0)) for k in used])
            ema_sd = model_ema.state_dict()
            fixed = {k: ema_sd[k].numpy().copy() for k, _ in arch.uplift_schema(C.SIZE) if k.endswith('.inv_freq') or k.startswith('embed.')}
            assert all(np.array_equal(model.state_dict()[k].numpy(), sd[k]) for k in fixed), 'a training step moved embed.* or inv_freq of the model itself'
            drift = max(float(np.abs((fixed[k] - sd[k]) / sd[k]).max()) for k in fixed)
            worst = {**{q: noise_steps[:, i].max() for i, q in enumerate(('loss_rot', 'loss_pos', 'norm'))}, **{q: noise[q].max() for q in C.QUANTITIES}}
            over = [q for q in worst if not worst[q] <= C.NOISE_CEILING[q]]
            why = ('a ReLU input is %.2e of its terms (< 2^-24) at step %d: on the kink' % (relu.min(), int(relu.argmin())) if relu.min() < RELU_MARGIN else
                   'the reference\'s own reorder noise of %s is %.2e (> %g)' % (over[0], worst[over[0]], C.NOISE_CEILING[over[0]]) if over else
                   'clipping is not %s at every step: norms %s' % ('active' if clipped else 'inactive', steps[:, 2]) if not ((steps[:, 2] > max_norm).all() if clipped else (steps[:, 2] < max_norm).all()) else
                   'embed.* / inv_freq of the EMA drift by %.2e' % drift if drift > 2 * C.STEPS * 2.0 ** -23 else None)
            if why is None:
                break
            print('%-22s seed %d skipped: %s' % (key, seed, why), flush=True)
        assert why is None, 'no seed meets the fixture conditions'
        print('%-22s seed %d norms %s | smallest ReLU margin %.2e | drift %.2e\n    self noise: %s' % (key, seed, np.array2string(steps[:, 2], precision=4), relu.min(), drift,
              ', '.join('%s %.2e' % (q, worst[q]) for q in worst)), flush=True)
        flat = {q: np.zeros(n, np.float32) for q in C.QUANTITIES}
        for q in C.QUANTITIES:
            for k, shape, off, u in layout:
                if u:
                    flat[q][off:off + a[q][k].size] = a[q][k].ravel()
        small = {'seed': np.array(seed, np.int64), 'steps': steps, 'relu_margin': relu, 'self_noise_steps': noise_steps, 'drift': np.array(drift)}
        small.update({'self_noise_' + q: noise[q] for q in C.QUANTITIES})
        small.update({'ema_fixed/' + k: v for k, v in fixed.items()})
        for part, qs in C.FILES.items():
            path = os.path.join(OUT, 'uplift_train_%s_%s.npz' % (key, part))
            np.savez_compressed(path, **{q: flat[q] for q in qs}, **(small if part == 'pe' else {}))
            print('   ', os.path.basename(path), os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
