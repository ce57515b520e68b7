"""Reading tests/golden/uplift_grad.npz / uplift_grad_sampled.npz / uplift_grad_edges.npz (tools/make_goldens_uplift_grad.py) and comparing a gradient
against a case: shared by the CPU test of the torch restatement and the GPU test of the library."""
import os

import numpy as np

from upliftingtabletennis_amd import arch, synth, weights

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden')
FILES = ('uplift_grad.npz', 'uplift_grad_sampled.npz', 'uplift_grad_edges.npz')
# the cases the fixture must hold: (size, time_rotation, transform_mode, batch, t, pad, stored in full)
EXPECTED = {
    'small_new_global_T20': ('small', 'new', 'global', 3, 17, 3, True),
    'small_old_global_T20': ('small', 'old', 'global', 3, 17, 3, True),
    'small_new_local_T20': ('small', 'new', 'local', 3, 17, 3, True),
    'base_new_global_T20': ('base', 'new', 'global', 2, 17, 3, False),
    'large_new_global_T50': ('large', 'new', 'global', 4, 43, 7, False),
    'large_new_global_T121': ('large', 'new', 'global', 3, 120, 1, False),
    'huge_new_global_T20': ('huge', 'new', 'global', 2, 17, 3, False),
    'edge_small_new_global_T16': ('small', 'new', 'global', 4, 13, 3, True),
    'edge_small_old_local_T16': ('small', 'old', 'local', 4, 13, 3, True),
}
# their input kind: 'ragged' (synth.ragged_uplift_batch) unless named here
EXPECTED_KIND = {'edge_small_new_global_T16': 'edge', 'edge_small_old_local_T16': 'edge'}
INPUTS = {'ragged': synth.ragged_uplift_batch, 'edge': synth.edge_uplift_batch}
N_SAMPLES = 256


class Case:
    def __init__(self, key, z):
        g = lambda f: z['%s/%s' % (key, f)]      # noqa: E731
        self.key = key
        self.seed, self.b, self.t, self.pad, local = [int(v) for v in g('meta')]
        self.size, self.rot_kind = [str(v) for v in g('variant')]
        self.mode = 'local' if local else 'global'
        self.kind = str(g('kind')) if ('%s/kind' % key) in z.files else 'ragged'
        self.loss, self.rot, self.pos = g('loss'), g('rot'), g('pos')
        self.unused = [str(v) for v in g('unused')]
        self.norms, self.self_noise, self.relu_margin = g('norms'), g('self_noise'), float(g('relu_margin'))
        self.full = ('%s/grad' % key) in z.files
        self.grad = g('grad') if self.full else None
        self.samples = None if self.full else g('samples')
        self.layout, self.n_floats = arch.uplift_grad_layout(self.size)

    def state_dict(self):
        return weights.random_uplift_state_dict(self.seed, self.size, 'connectstage', 'dynamic', self.rot_kind)

    def inputs(self):
        """ball, table, mask, times, r_world, rotation (numpy float32)"""
        return list(INPUTS[self.kind](self.b, self.t, seed=self.seed, pad=self.pad)) + list(synth.uplift_targets(self.b, self.t + self.pad, self.seed))

    def compare(self, grads):
        """grads: {name: numpy array or None}.  -> (worst relative L2 over the tensors' stored entries, worst relative norm error);
        every tensor of the layout is compared, an unused one must be None or exactly zero."""
        assert sorted(grads) == sorted(k for k, _, _, _ in self.layout)
        worst, worst_norm, at = 0.0, 0.0, 0
        for i, (k, shape, off, used) in enumerate(self.layout):
            n = int(np.prod(shape))
            g = grads[k]
            if not used:
                assert k in self.unused and (g is None or not np.any(g)), '%s must receive no gradient' % k
                at += 0 if self.full else min(n, N_SAMPLES)
                continue
            assert g is not None and g.shape == tuple(shape) and np.isfinite(g).all(), k
            g = g.astype(np.float64).ravel()
            if self.full:
                ref = self.grad[off:off + n].astype(np.float64)
                got = g
            else:
                idx = synth.sample_indices(n, N_SAMPLES, self.seed)
                ref = self.samples[at:at + idx.size].astype(np.float64)
                got = g[idx]
                at += idx.size
            worst = max(worst, np.linalg.norm(got - ref) / np.linalg.norm(ref))
            worst_norm = max(worst_norm, abs(np.linalg.norm(g) - self.norms[i]) / self.norms[i])
        return worst, worst_norm


def load_cases():
    out = {}
    for f in FILES:
        z = np.load(os.path.join(GOLDEN, f), allow_pickle=False)
        for key in sorted({n.split('/')[0] for n in z.files}):
            out[key] = Case(key, z)
    return out
