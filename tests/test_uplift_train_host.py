"""What of the uplift optimizer step can be checked without a GPU: the C-ABI's new symbols, the mapping between the gradient layout and
the handle's plain weights, UpliftTrainer's refusals, and the conditions of tests/golden/uplift_train_*.npz re-checked from the
stored numbers (tools/make_goldens_uplift_train.py asserts them from the reference when it writes the files)."""
import os
import re

import numpy as np
import pytest

from helpers import uplift_train_cases as C
from upliftingtabletennis_amd import _lib, arch, uplift, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('ttup_opt_flat_scratch_bytes', 'ttup_opt_flat_step', 'ttup_uplift_opt_create', 'ttup_uplift_opt_destroy', 'ttup_uplift_opt_step',
           'ttup_uplift_opt_read', 'ttup_uplift_opt_load', 'ttup_uplift_opt_set_step', 'ttup_uplift_opt_get_step')


def test_header_declares_the_optimizer_symbols():
    hdr = open(os.path.join(ROOT, 'include', 'ttup.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r'#define\s+TTUP_ESTALE\s+6\b', hdr) and _lib.ESTALE == 6
    for i, which in enumerate(('PARAM', 'EMA', 'M', 'V')):
        assert re.search(r'#define\s+TTUP_OPT_%s\s+%d\b' % (which, i), hdr)
    assert (_lib.OPT_PARAM, _lib.OPT_EMA, _lib.OPT_M, _lib.OPT_V) == (0, 1, 2, 3)
    assert 'uplift_opt.hip' in __import__('upliftingtabletennis_amd.build', fromlist=['SOURCES']).SOURCES


def test_library_refuses_bad_arguments_before_a_device_is_touched():
    from upliftingtabletennis_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    lib = _lib.load()
    assert lib.ttup_version() == 103
    assert lib.ttup_opt_flat_scratch_bytes() >= 1024 * 8 + 8
    hyper = (1e-4, 0.9, 0.999, 1e-8, 0.999, 5.0)
    assert lib.ttup_opt_flat_step(None, None, None, None, None, 4, 0, 0, *hyper, 1, None, None, None) == _lib.EINVAL
    assert b'null' in lib.ttup_last_error()
    one = 16          # any non-null, aligned address: the arguments are refused before it is looked at
    assert lib.ttup_opt_flat_step(one, one, one, one, one, 4, 5, 0, *hyper, 1, one, None, None) == _lib.EINVAL          # hole begins past n
    assert b'hole' in lib.ttup_last_error()
    assert lib.ttup_opt_flat_step(one, one, one, one, one, 4, 0, 0, *hyper, 0, one, None, None) == _lib.EINVAL          # 1-based step count
    assert b'1-based' in lib.ttup_last_error()
    assert lib.ttup_opt_flat_step(one, one, one, one, one, 4, 0, 0, 1e-4, 1.0, 0.999, 1e-8, 0.999, 5.0, 1, one, None, None) == _lib.EINVAL
    assert b'hyper' in lib.ttup_last_error()
    import ctypes
    h = ctypes.c_void_p()
    assert lib.ttup_uplift_opt_create(None, *hyper, ctypes.byref(h)) == _lib.EINVAL
    for fn, args in ((lib.ttup_uplift_opt_step, (None, None, None, None)), (lib.ttup_uplift_opt_read, (None, 0, None, None)),
                     (lib.ttup_uplift_opt_load, (None, 0, None, None)), (lib.ttup_uplift_opt_set_step, (None, 0)), (lib.ttup_uplift_opt_get_step, (None, None))):
        assert fn(*args) == _lib.EINVAL
    lib.ttup_uplift_opt_destroy(None)


@pytest.mark.parametrize('size', sorted(arch.UPLIFT_SIZES))
def test_hole_between_gradient_layout_and_plain_weights(size):
    """The plain device weights are the blob's records after inv_freq (weights.pack_uplift_blob): the layout without embed.*.  The
    hole sits right after cls_token and is D*3 + D + D*D + D long; walking the blob's records and the layout side by side with
    arch.uplift_grad_hole gives the same tensor at every plain offset."""
    d = arch.UPLIFT_SIZES[size][0]
    begin, length = arch.uplift_grad_hole(size)
    assert (begin, length) == (d, d * 3 + d + d * d + d)
    layout, n = arch.uplift_grad_layout(size)
    body = [(k, shape) for k, shape in arch.uplift_schema(size) if not k.endswith('inv_freq') and not k.startswith('embed.')]          # pack_uplift_blob's record order
    by_name = {k: (shape, off, used) for k, shape, off, used in layout}
    plain = 0
    for k, shape in body:
        lshape, off, used = by_name[k]
        assert used and tuple(lshape) == tuple(shape)
        assert off == plain + (length if plain >= begin else 0), k
        plain += int(np.prod(shape))
    assert plain == n - length
    assert all(begin <= off < begin + length for k, _, off, used in layout if not used)
    assert [k for k, _, _, used in layout if not used] == ['embed.fc1.weight', 'embed.fc1.bias', 'embed.fc2.weight', 'embed.fc2.bias']


@pytest.mark.parametrize('name,mode', [('multistage', 'dynamic'), ('connectstage', 'stacked'), ('singlestage', 'free'), ('multistage', 'originalmethod')])
def test_trainer_refuses_other_variants_before_the_library_is_asked(monkeypatch, name, mode):
    def touched(*a, **k):
        raise AssertionError('the native library was touched')
    monkeypatch.setattr(_lib, 'load', touched)
    monkeypatch.setattr(_lib, 'require_gpu', touched)
    sd = weights.random_uplift_state_dict(3, 'small', name, mode)
    with pytest.raises(ValueError, match='%s/%s' % (name, mode)):
        uplift.UpliftTrainer(sd, size='small', name=name, mode=mode)
    with pytest.raises(ValueError, match='transform_mode'):
        uplift.UpliftTrainer(weights.random_uplift_state_dict(3, 'small'), size='small', transform_mode='ball')
    with pytest.raises(ValueError, match='size'):
        uplift.UpliftTrainer(sd, size='tiny')


@pytest.mark.parametrize('key', sorted(C.EXPECTED))
def test_fixture_conditions_hold_in_the_stored_numbers(key):
    c = C.Case(key)
    assert c.losses.shape == (C.STEPS, 3) and np.isfinite(c.losses).all()
    norms = c.losses[:, 2]
    assert (norms > c.max_norm).all() if c.clipped else (norms < c.max_norm).all(), norms
    assert (c.relu_margin >= 2.0 ** -24).all()
    for q in ('loss_rot', 'loss_pos', 'norm') + C.QUANTITIES:
        assert 0 < c.noise(q) <= C.NOISE_CEILING[q], (q, c.noise(q))
    assert 0 <= c.drift <= 2 * C.STEPS * 2.0 ** -23
    sd = c.state_dict()
    for q in C.QUANTITIES:
        final = c.final(q)
        assert sorted(final) == sorted(c.used)
        flat = c.z[q]
        begin, length = arch.uplift_grad_hole(C.SIZE)
        assert flat.shape == (c.n_floats,) and not flat[begin:begin + length].any() and np.isfinite(flat).all()
    # the parameters moved by about lr per step, the second moments are positive, and the ema_decay 0.9 case's EMA moved with them
    moved = np.concatenate([(c.final('param')[k] - sd[k]).ravel() for k in c.used])
    assert 0.5 * C.LR < np.abs(moved).mean() < C.STEPS * C.LR * 1.01
    assert all((c.final('exp_avg_sq')[k] >= 0).all() for k in c.used)
    ema_moved = np.concatenate([(c.final('ema')[k] - sd[k]).ravel() for k in c.used])
    assert np.abs(ema_moved).mean() > (1e-5 if c.ema_decay < 0.99 else 1e-8)
    fixed = c.ema_fixed()
    assert sorted(fixed) == sorted(c.fixed)
    assert max(float(np.abs((fixed[k] - sd[k]) / sd[k]).max()) for k in fixed) == c.drift
