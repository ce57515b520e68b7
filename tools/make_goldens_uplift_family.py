#!/usr/bin/env python3
"""Generate tests/golden/uplift_family.npz and uplift_family_schema.json by running the REFERENCE's own uplift models
(uplifting/model.py:get_model) for every variant a checkpoint can name, on seeded weights.

Runs only where the reference sources are (TTUP_REFERENCE); the tests read the two files alone.  Per case the reference model is
built by ``get_model(name, size, mode, time_rotation)``, loaded ``strict=True`` with ``weights.random_uplift_state_dict`` of the
same arguments and run on ``synth.ragged_uplift_batch`` (second trajectory shorter, irregular time stamps on the first, two
invisible keypoints).  Stored per case: seeds and shape (`meta` = weight/input seed, batch, t, pad), the variant's names, ``rot``,
``pos``, ``rot_local`` (uplifting/helper.py:transform_rotationaxes) and ``flip`` = the distance, relative to max|output|, of (rot,
pos) to the output of the SAME weights under the other time_rotation: what a parity test must be able to resolve.

Cases: all 18 (name, mode, time_rotation) at `small`; at `large` eight variants with 'new' and two with 'old', at padded lengths
11, 50 and 121; one `base` and one `huge`.

    python tools/make_goldens_uplift_family.py

With --edges it writes tests/golden/uplift_family_edges.npz instead and leaves the two files above alone: the cases `FAMILY` of
tests/helpers/uplift_forward_cases.py (every non-default variant at a length, tile or mask edge of its kernels, on
``synth.edge_uplift_batch``; four default-variant cases that pin the torch restatement the forward's edge sweep is compared with),
inputs built by that module's ``make_inputs``.  Stored per case: ``rot``, ``pos``, ``meta``, ``variant`` and ``kind`` only.

    python tools/make_goldens_uplift_family.py --edges
"""
import json
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

from upliftingtabletennis_amd import arch, synth, weights  # noqa: E402

# (size, name, mode, time_rotation, seed, batch, t, pad)
# (seed 107 of small connectstage/stacked gave a new-vs-old distance of 6.7e-4 on pos, under ten times the parity bar: it runs on SEED_SMALL instead)
SEED_SMALL = {('connectstage', 'stacked'): 307}
CASES = [('small', n, m, r, SEED_SMALL.get((n, m), 100 + i // 2), 3, 17, 3) for i, (n, m, r) in enumerate(arch.uplift_variants())] + [
    ('large', 'singlestage', 'free', 'new', 201, 4, 8, 3),
    ('large', 'singlestage', 'dynamic', 'new', 202, 4, 43, 7),
    ('large', 'singlestage', 'stacked', 'new', 203, 3, 120, 1),
    ('large', 'singlestage', 'stacked', 'old', 204, 3, 6, 2),
    ('large', 'multistage', 'dynamic', 'new', 205, 4, 8, 3),
    ('large', 'multistage', 'stacked', 'new', 206, 4, 43, 7),
    ('large', 'multistage', 'stacked', 'old', 207, 4, 43, 7),
    ('large', 'multistage', 'originalmethod', 'new', 208, 3, 120, 1),
    ('large', 'connectstage', 'stacked', 'new', 209, 3, 120, 1),
    ('large', 'connectstage', 'originalmethod', 'new', 210, 4, 8, 3),
    ('base', 'singlestage', 'stacked', 'old', 211, 2, 17, 3),
    ('huge', 'multistage', 'originalmethod', 'new', 212, 2, 17, 3),
]


def case_name(size, name, mode, rot, t, pad):
    return '%s_%s_%s_%s_T%d' % (size, name, mode, rot, t + pad)


def edges():
    import make_goldens
    make_goldens.install_stubs()
    from helpers import uplift_forward_cases as C
    from uplifting.model import get_model
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {}
    for c in C.FAMILY:
        sd = weights.random_uplift_state_dict(c.seed, c.size, c.name, c.mode, c.rot)
        m = get_model(c.name, c.size, c.mode, c.rot)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        m.eval()
        with torch.no_grad():
            rot, pos = [a.numpy() for a in m(*[torch.from_numpy(a) for a in C.make_inputs(c)])]
        assert np.isfinite(rot).all() and np.isfinite(pos).all(), 'non-finite reference output: %s' % C.key(c)
        key = C.key(c)
        assert key + '/rot' not in out, key
        out[key + '/rot'], out[key + '/pos'] = rot, pos
        out[key + '/meta'] = np.array([c.seed, c.b, c.t, c.pad], np.int64)
        out[key + '/variant'] = np.array([c.size, c.name, c.mode, c.rot])
        out[key + '/kind'] = np.array(c.kind)
        print('%-56s max|rot| %.3e max|pos| %.3e' % (key, np.abs(rot).max(), np.abs(pos).max()), flush=True)
    np.savez_compressed(os.path.join(OUT, 'uplift_family_edges.npz'), **out)


def main():
    import make_goldens
    make_goldens.install_stubs()
    from uplifting.helper import transform_rotationaxes
    from uplifting.model import get_model
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out, schema = {}, {}
    for size, name, mode, rot_kind, seed, b, t, pad in CASES:
        sd = weights.random_uplift_state_dict(seed, size, name, mode, rot_kind)
        inputs = [torch.from_numpy(a) for a in synth.ragged_uplift_batch(b, t, seed=seed, pad=pad)]
        res = {}
        for r in arch.UPLIFT_ROTATIONS:
            m = get_model(name, size, mode, r)
            schema['%s/%s/%s' % (name, size, mode)] = [(k, list(v.shape)) for k, v in m.state_dict().items()]
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            m.eval()
            with torch.no_grad():
                rot, pos = m(*inputs)
                res[r] = (rot.numpy(), pos.numpy(), transform_rotationaxes(rot, pos.clone()).numpy())
        rot, pos, rot_local = res[rot_kind]
        o_rot, o_pos, _ = res['old' if rot_kind == 'new' else 'new']
        assert all(np.isfinite(a).all() for a in (rot, pos, rot_local)), 'non-finite reference output'
        flip = np.array([np.abs(rot - o_rot).max() / np.abs(rot).max(), np.abs(pos - o_pos).max() / np.abs(pos).max()])
        key = case_name(size, name, mode, rot_kind, t, pad)
        assert key + '/rot' not in out, key
        out[key + '/rot'], out[key + '/pos'], out[key + '/rot_local'] = rot, pos, rot_local
        out[key + '/meta'] = np.array([seed, b, t, pad], np.int64)
        out[key + '/variant'] = np.array([size, name, mode, rot_kind])
        out[key + '/flip'] = flip
        print('%-48s new-vs-old relative distance: rot %.3e pos %.3e' % (key, flip[0], flip[1]), flush=True)
    for name, mode, _ in arch.uplift_variants():          # every size's key list is checked; those without a case are not stored
        for size in arch.UPLIFT_SIZES:
            ref = schema.get('%s/%s/%s' % (name, size, mode)) or [(a, list(v.shape)) for a, v in get_model(name, size, mode, 'new').state_dict().items()]
            assert [(a, tuple(s)) for a, s in ref] == [(a, tuple(s)) for a, s in arch.uplift_variant_schema(name, size, mode)], (name, size, mode)
    np.savez_compressed(os.path.join(OUT, 'uplift_family.npz'), **out)
    with open(os.path.join(OUT, 'uplift_family_schema.json'), 'w') as f:
        json.dump(schema, f, sort_keys=True)


if __name__ == '__main__':
    if sys.argv[1:] not in ([], ['--edges']):
        sys.exit('usage: make_goldens_uplift_family.py [--edges]')
    edges() if sys.argv[1:] else main()
