"""Reading tests/golden/uplift_train_*.npz (tools/make_goldens_uplift_train.py): K training steps of the reference -- its model, its
loss, clip_grad_norm_, torch.optim.Adam, update_ema -- on a different seeded batch per step.  Shared by the fixture tool, the host
test of the fixture's own conditions and the GPU test of uplift.UpliftTrainer."""
import os

import numpy as np

from upliftingtabletennis_amd import arch, synth, weights

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden')
SIZE, BATCH, T, PAD, STEPS = 'small', 3, 17, 3, 4
LR, BETAS, EPS, MAX_NORM = 1e-4, (0.9, 0.999), 1e-8, 5.0          # uplifting/config.py, train.py:73, :129
# case -> (transform_mode, ema_decay, max_norm of clip_grad_norm_, clipping active at every step)
EXPECTED = {
    'global_ema999': ('global', 0.999, MAX_NORM, True),
    'local_ema900': ('local', 0.9, MAX_NORM, True),
    'noclip_global_ema999': ('global', 0.999, 1.0e4, False),
}
QUANTITIES = ('param', 'ema', 'exp_avg', 'exp_avg_sq')
FILES = {'pe': ('param', 'ema'), 'mv': ('exp_avg', 'exp_avg_sq')}          # two files per case: four full buffers pass 1 MiB
# what the tool asserts of the reference's own reorder noise (relative; worst step / worst tensor of a quantity)
NOISE_CEILING = {'loss_rot': 1e-6, 'loss_pos': 1e-6, 'norm': 1e-6, 'param': 1e-3, 'ema': 1e-3, 'exp_avg': 1e-4, 'exp_avg_sq': 1e-4}
MARGIN = 10.0          # bar = MARGIN x the stored self noise of the quantity (the gradient fixture's rule)


def step_inputs(seed, k):
    """ball, table, mask, times, r_world, rotation (numpy float32) of step k of the case with that seed: a different batch per step."""
    s = seed + 1000 * (k + 1)
    return list(synth.ragged_uplift_batch(BATCH, T, seed=s, pad=PAD)) + list(synth.uplift_targets(BATCH, T + PAD, s))


def rel_l2(got, ref):
    return float(np.linalg.norm(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) / np.linalg.norm(np.asarray(ref, np.float64)))


class Case:
    def __init__(self, key):
        self.key = key
        self.mode, self.ema_decay, self.max_norm, self.clipped = EXPECTED[key]
        z = {}
        for part in FILES:
            with np.load(os.path.join(GOLDEN, 'uplift_train_%s_%s.npz' % (key, part)), allow_pickle=False) as f:
                z.update({n: f[n] for n in f.files})
        self.z = z
        self.seed = int(z['seed'])
        self.losses, self.noise_steps = z['steps'], z['self_noise_steps']          # (K, 3): loss_rot, loss_pos, norm before clipping
        self.relu_margin = z['relu_margin']                                         # (K,)
        self.layout, self.n_floats = arch.uplift_grad_layout(SIZE)
        self.used = [k for k, _, _, u in self.layout if u]
        self.fixed = [k for k, _ in arch.uplift_schema(SIZE) if k.endswith('.inv_freq') or k.startswith('embed.')]
        self.drift = float(z['drift'])

    def state_dict(self):
        return weights.random_uplift_state_dict(self.seed, SIZE)

    def inputs(self, k):
        return step_inputs(self.seed, k)

    def final(self, quantity):
        """{name: array} of the reference after STEPS steps"""
        flat = self.z[quantity]
        return {k: flat[off:off + int(np.prod(shape))].reshape(shape) for k, shape, off, u in self.layout if u}

    def noise(self, quantity):
        """the stored self noise of a quantity: worst over its steps / tensors"""
        if quantity in ('loss_rot', 'loss_pos', 'norm'):
            return float(self.noise_steps[:, ('loss_rot', 'loss_pos', 'norm').index(quantity)].max())
        return float(self.z['self_noise_' + quantity].max())

    def bar(self, quantity):
        return MARGIN * self.noise(quantity)

    def ema_fixed(self):
        """the reference's EMA of embed.* and the inv_freq buffers after STEPS steps"""
        return {k: self.z['ema_fixed/' + k] for k in self.fixed}
