"""The uplift training loss and its parameter gradients, CPU side: the C-ABI's new entry points refuse null arguments before any
device is touched, the flat gradient layout, the differentiable torch restatement (tests/helpers/uplift_torch_grad.py) against the
reference's own autograd (tests/golden/uplift_grad*.npz, tools/make_goldens_uplift_grad.py), and the Python surface's refusal of
the variants that have no gradients."""
import ctypes

import numpy as np
import pytest

from helpers import uplift_grad_cases as C
from helpers import uplift_torch_grad as R
from upliftingtabletennis_amd import _lib, arch, uplift

# The fixture's asserted ceiling on the reference's own reorder noise (batch reversed, one thread).  The restatement is the same
# fp32 arithmetic on the same torch build, so it is held to that ceiling.
NOISE_CEILING = 1e-5
CASES = C.load_cases()


def test_new_symbols_refuse_null_arguments_before_any_device():
    lib = _lib.load()
    for name in ('ttup_uplift_grad_layout', 'ttup_uplift_grad_workspace_bytes', 'ttup_uplift_loss_grad'):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.ttup_version() == 103
    n, k = ctypes.c_longlong(0), ctypes.c_int(0)
    assert lib.ttup_uplift_grad_layout(None, ctypes.byref(n), ctypes.byref(k), None, None, 0) == _lib.EINVAL
    assert b'null pointer' in lib.ttup_last_error()
    assert lib.ttup_uplift_grad_workspace_bytes(None, 4, 50) == 0
    assert lib.ttup_uplift_loss_grad(None, None, None, None, None, None, None, 4, 50, 0, None, 0, None, None, None, None, None) == _lib.EINVAL
    assert b'null pointer' in lib.ttup_last_error()


@pytest.mark.parametrize('size', sorted(arch.UPLIFT_SIZES))
def test_grad_layout_is_the_schema_without_inv_freq(size):
    layout, n = arch.uplift_grad_layout(size)
    schema = [(k, tuple(s)) for k, s in arch.uplift_variant_schema('connectstage', size, 'dynamic') if not k.endswith('.inv_freq')]
    assert [(k, s) for k, s, _, _ in layout] == schema
    off = 0
    for k, shape, o, used in layout:
        assert o == off, k
        off += int(np.prod(shape))
        assert used == (not k.startswith('embed.')), k
    assert off == n
    assert sum(1 for e in layout if not e[3]) == 4
    if size == 'small':
        assert n + 12 * (32 // 4 // 2) == 82134          # with the 12 layers' inv_freq buffers: the reference's parameter count


def test_fixture_holds_the_cases_and_its_own_conditions():
    assert sorted(CASES) == sorted(C.EXPECTED)
    for key, want in C.EXPECTED.items():
        c = CASES[key]
        assert (c.size, c.rot_kind, c.mode, c.b, c.t, c.pad, c.full) == want, key
        assert c.kind == C.EXPECTED_KIND.get(key, 'ragged'), key
        if c.kind == 'edge':          # the mask forms the edge cases are there for, on the inputs the case rebuilds
            _, table, mask, _ = c.inputs()[:4]
            vis = (table[:, :, 2] == 1).sum(1)
            assert mask[0, 2] == 0 and mask[0, 1] == 1 and mask[0, 3] == 1 and mask[1].sum() == 1 and not mask[3].any()
            assert vis[0] == 0 and vis[2] == 1
        used = np.array([u for _, _, _, u in c.layout])
        assert c.self_noise.max() <= NOISE_CEILING
        assert c.relu_margin >= R.RELU_MARGIN == 2.0 ** -24          # no ReLU of the reference's forward on its kink
        total = np.sqrt((c.norms ** 2).sum())
        assert (c.norms[used] / total).min() >= 1e-4
        assert c.unused == [k for k, _, _, u in c.layout if not u]


@pytest.mark.parametrize('key', sorted(C.EXPECTED))
def test_restatement_matches_the_reference_autograd(key):
    c = CASES[key]
    margins = []
    l_rot, l_pos, grads, rot, pos = R.loss_and_grad(c.state_dict(), c.size, *c.inputs(), time_rotation=c.rot_kind, transform_mode=c.mode, margins=margins)
    m = R.relu_margin(margins)          # the restatement's measure is the fixture tool's (a near-zero sum itself moves with the last bits)
    assert m >= R.RELU_MARGIN and 0.5 * c.relu_margin <= m <= 2 * c.relu_margin, (m, c.relu_margin)
    worst, worst_norm = c.compare(grads)
    print('%s: worst tensor %.3e, worst norm %.3e, losses %.9g %.9g (fixture %.9g %.9g)' % (key, worst, worst_norm, l_rot, l_pos, c.loss[0], c.loss[1]))
    assert worst <= NOISE_CEILING and worst_norm <= NOISE_CEILING
    assert abs(l_rot - c.loss[0]) <= 1e-6 * abs(c.loss[0]) and abs(l_pos - c.loss[1]) <= 1e-6 * abs(c.loss[1])
    np.testing.assert_allclose(rot, c.rot, rtol=0, atol=1e-5 * np.abs(c.rot).max())
    np.testing.assert_allclose(pos, c.pos, rtol=0, atol=1e-5 * np.abs(c.pos).max())


@pytest.mark.parametrize('name,mode', [(n, m) for n, m, r in arch.uplift_variants() if r == 'new' and (n, m) != ('connectstage', 'dynamic')])
def test_unsupported_variants_raise_before_the_library_is_asked(name, mode, monkeypatch):
    model = object.__new__(uplift.MultiStageModel)          # no handle, no library: the check must come first
    model.name, model.mode, model.size = name, mode, 'small'
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('the library was asked'))
    z = np.zeros(1)
    with pytest.raises(ValueError, match='%s/%s' % (name, mode)):
        model.loss_and_grad(z, z, z, z, z, z)
    with pytest.raises(ValueError, match='%s/%s' % (name, mode)):
        model.grad_layout()
