"""The uplift gradient pass (uplift.MultiStageModel.loss_and_grad -> ttup_uplift_loss_grad) at the shapes and masks where its kernels
change form, against the torch restatement's autograd on the host (tests/helpers/uplift_torch_grad.py, pinned to the reference's own
autograd by the CPU suite -- on the edge-mask inputs too, tests/golden/uplift_grad_edges.npz).  The reference is never read here.

What the sweep reaches that the four padded lengths of test_uplift_grad_gpu.py (20, 50, 121, 250) do not:
  * attention width: the kernels run P = the smallest power of two >= max(16, S) threads per sequence and pack 64 / P sequences into
    a workgroup below 64; S = len in the time stage, len + 1 in the spin stage, 14 in the table stage.  P = 16 (len <= 15), lengths
    at which the two stages fall on different P (16, 32, 64, 128), fewer sequences than a workgroup packs (B = 1), the upper end
    (len 255: a spin sequence of 256 tokens);
  * the LDS opt-in above 48 KB, which head_dim 8 (`small`) never needs: base / large / huge at long sequences, up to the largest
    launch there is (`large`, S = 256: 135 KB of the 160 KB cap);
  * row counts that are an exact multiple of the 512-row reduction slice (B = 4, len 128), that leave a last slice of one row (B = 3,
    len 171: 513 rows) and M = 1 in the rotation head (B = 1);
  * masks that tail padding never gives (synth.edge_uplift_batch): interior holes, a single valid step, a trajectory padded
    throughout, tables with no and with one visible keypoint.

Bars.  Every used tensor in full, in two metrics: relative L2 <= 1e-4 and max |got - ref| <= 1e-4 max |ref| -- the second is the
form the forward tests use; a relative L2 alone lets one entry of a 49 152-entry tensor be off by 2 % of the tensor's rms.  1e-4 is
the project's uplift bar; the restatement's own reorder noise (batch reversed, one thread) is <= 1.4e-6 in the max metric on these
cases, so the bar sits about 70x above it.

ReLU kinks: as in test_uplift_grad_gpu.py, a case runs on a seed on which no ReLU input of a layer over fewer than 1 / BAR rows
lies within 2^-24 of the sum of its terms.  The margin comes from the restatement alone and is looked at before the device result;
a seed that misses it is skipped (printed) for seed + 100, four times at the most.  Measured values per case: DESIGN.md 17."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import has_gpu
from helpers import uplift_torch_grad as R
from test_uplift_grad_gpu import BAR, KINK_ROWS, assert_same_bits, dev, grads_layout, make_model, rel_max, to_numpy

pytestmark = pytest.mark.gpu
if has_gpu():
    from upliftingtabletennis_amd import _lib, synth, weights

FIRST_SEED, SEED_STEP, SEED_TRIES = 900, 100, 5

# (size, B, len, time_rotation, transform_mode, input kind, pad[, first seed: FIRST_SEED if absent])
SWEEP = (
    # attention widths, small: P = 16 | 16 / 32 | 32 / 64 | 64 / 128 | 128 / 256 | 256
    [('small', b, n, 'new', 'global', 'ragged', 1) for b, n in
     ((1, 2), (1, 15), (3, 16), (2, 17), (1, 31), (5, 32), (2, 33), (3, 63), (1, 64), (2, 65), (2, 127), (1, 128), (2, 129), (2, 255), (1, 255))] +
    # other head dims (32, 24, 16), the LDS opt-in
    [('large', 1, 16, 'new', 'global', 'ragged', 1), ('large', 2, 255, 'new', 'global', 'ragged', 1), ('huge', 2, 64, 'new', 'global', 'ragged', 1),
     ('huge', 1, 255, 'new', 'global', 'ragged', 1), ('base', 3, 128, 'new', 'global', 'ragged', 1)] +
    # reduction slices: 512 temporal rows = one full slice (7 168 table rows = 14 full slices); 513 rows = a last slice of one row
    [('small', 4, 128, 'new', 'global', 'ragged', 1), ('small', 3, 171, 'new', 'global', 'ragged', 1)] +
    # the shortest trajectory transform_mode 'local' takes
    [('small', 2, 2, 'new', 'local', 'ragged', 1)] +
    # edge masks; the first one on the seed of the fixture case edge_small_new_global_T16, so on its very inputs
    [('small', 4, 16, 'new', 'global', 'edge', 3, 320), ('large', 4, 33, 'new', 'global', 'edge', 3), ('huge', 4, 64, 'old', 'global', 'edge', 3),
     ('base', 4, 128, 'new', 'local', 'edge', 3)])


def case_id(c):
    size, b, n, rot_kind, mode, kind = c[:6]
    return '%s-B%d-len%d-%s-%s-%s' % (size, b, n, rot_kind, mode, kind)


def batch_inputs(kind, b, length, seed, pad):
    make = synth.ragged_uplift_batch if kind == 'ragged' else synth.edge_uplift_batch
    return list(make(b, length - pad, seed=seed, pad=pad)) + list(synth.uplift_targets(b, length, seed))


def vetted_case(size, b, length, rot_kind, mode, kind, pad, first_seed=FIRST_SEED):
    """The first seed of first_seed, +100, ... whose restatement has no ReLU input of a short layer on its kink.
    -> (seed, skipped seeds, margin, state dict, inputs, the restatement's results)"""
    skipped = []
    for seed in range(first_seed, first_seed + SEED_STEP * SEED_TRIES, SEED_STEP):
        sd = weights.random_uplift_state_dict(seed, size, time_rotation=rot_kind)
        inputs = batch_inputs(kind, b, length, seed, pad)
        margins = []
        ref = R.loss_and_grad(sd, size, *inputs, time_rotation=rot_kind, transform_mode=mode, margins=margins)
        margin = R.relu_margin(margins, KINK_ROWS)
        if margin >= R.RELU_MARGIN:
            return seed, skipped, margin, sd, inputs, ref
        print('%s B=%d len=%d: seed %d skipped, a ReLU input of a layer of < %d rows is %.2e of its terms (< 2^-24)' % (size, b, length, seed, KINK_ROWS, margin))
        skipped.append(seed)
    pytest.fail('no seed of %s meets the ReLU criterion' % skipped)


@pytest.mark.parametrize('case', SWEEP, ids=case_id)
def test_gradients_match_the_restatement_at_the_kernels_edges(case):
    size, b, length, rot_kind, mode, kind = case[:6]
    seed, skipped, margin, sd, inputs, (r_rot, r_pos, ref, ref_rot, ref_pos) = vetted_case(*case)
    mask = inputs[2]
    assert np.isfinite(ref_rot).all() and np.isfinite(ref_pos).all() and np.isfinite([r_rot, r_pos]).all()
    model = make_model(size, sd, rot_kind, max_batch=b, max_len=length)
    args = dev(inputs)
    first = model.loss_and_grad(*args, transform_mode=mode)
    l_rot, l_pos, grads = first
    assert_same_bits(first, model.loss_and_grad(*args, transform_mode=mode))
    g = to_numpy(grads)
    for t in (l_rot, l_pos, grads.flat, grads.rot, grads.pos):
        assert bool(torch.isfinite(t).all())
    worst_l2, at_l2, worst_max, at_max = 0.0, None, 0.0, None
    for k, shape, off, used in grads_layout(size):
        if not used:
            assert ref[k] is None and not np.any(g[k]), k
            continue
        assert ref[k].shape == tuple(shape) and np.isfinite(ref[k]).all(), k
        d = g[k].astype(np.float64) - ref[k]
        e_l2 = np.linalg.norm(d) / np.linalg.norm(ref[k].astype(np.float64))
        e_max = np.abs(d).max() / np.abs(ref[k]).max()
        if e_l2 > worst_l2:
            worst_l2, at_l2 = e_l2, k
        if e_max > worst_max:
            worst_max, at_max = e_max, k
    keep = mask != 0
    e_rot, e_pos = abs(float(l_rot) - r_rot) / abs(r_rot), abs(float(l_pos) - r_pos) / abs(r_pos)
    o_rot = rel_max(grads.rot.cpu().numpy(), ref_rot)          # every row: that of a trajectory padded throughout too (its cls token attends to itself)
    o_pos = rel_max(grads.pos.cpu().numpy()[keep], ref_pos[keep])
    f_rot, f_pos = model.forward(*args[:4])
    a_rot = rel_max(f_rot.cpu().numpy(), grads.rot.cpu().numpy().astype(np.float64))
    a_pos = rel_max(f_pos.cpu().numpy()[keep], grads.pos.cpu().numpy()[keep].astype(np.float64))
    print('%s: seed %d (skipped %s) | worst tensor L2 %.2e (%s), max %.2e (%s) | losses %.1e / %.1e | rot / pos %.1e / %.1e | forward rot / pos %.1e / %.1e | margin %.1e'
          % (case_id(case), seed, skipped or 'none', worst_l2, at_l2, worst_max, at_max, e_rot, e_pos, o_rot, o_pos, a_rot, a_pos, margin))
    assert worst_l2 <= BAR and worst_max <= BAR
    assert e_rot <= BAR and e_pos <= BAR and o_rot <= BAR and o_pos <= BAR
    assert a_rot <= BAR and a_pos <= BAR


@pytest.mark.parametrize('rot_kind', ['new', 'old'])
def test_masked_rows_are_inert_on_the_edge_masks(rot_kind):
    """test_masked_rows_are_inert on interior holes, a trajectory of one valid step, one padded throughout and tables with no / one
    visible keypoint: large finite values in every mask == 0 slot of ball, times and r_world, and in the xy of every invisible
    keypoint, change no bit of any gradient, of the losses, of rot or of pos on valid rows; everything stays finite."""
    sd = weights.random_uplift_state_dict(412, 'large', time_rotation=rot_kind)
    ball, table, mask, times, r_world, rotation = batch_inputs('edge', 4, 33, 412, 3)
    pad = mask == 0
    assert pad[0, 2] and not pad[0, 1] and not pad[0, 3] and mask[1].sum() == 1 and pad[3].all()
    assert not (table[0, :, 2] == 1).any() and (table[2, :, 2] == 1).sum() == 1
    model = make_model('large', sd, rot_kind, max_batch=4, max_len=33)
    base = model.loss_and_grad(*dev([ball, table, mask, times, r_world, rotation]))
    ball2, times2, world2, table2 = ball.copy(), times.copy(), r_world.copy(), table.copy()
    ball2[pad] = 3.0e3; times2[pad] = 977.123; world2[pad] = -4.0e4
    table2[table[:, :, 2] == 0, :2] = 2.5e3
    keep = torch.from_numpy(mask != 0).cuda()
    for changed in ([ball2, table, mask, times2, world2, rotation], [ball, table2, mask, times, r_world, rotation], [ball2, table2, mask, times2, world2, rotation]):
        got = model.loss_and_grad(*dev(changed))
        assert_same_bits(base, got)
        assert torch.equal(base[2].pos[keep], got[2].pos[keep])
        for t in (got[0], got[1], got[2].flat, got[2].rot, got[2].pos):
            assert bool(torch.isfinite(t).all())


# ------------------------------------------------------------------ limits: refused before anything is launched
SENTINEL = -7.25


def raw_call(model, b, length, flags, short_by=0, shift=0):
    """ttup_uplift_loss_grad through ctypes on zero inputs, with sentinel-filled outputs and a workspace `short_by` bytes smaller
    than asked for / moved by `shift` bytes.  -> (return code, message, outputs still hold the sentinel everywhere)"""
    lib = model._lib
    z = lambda *s: torch.zeros(s, device='cuda')          # noqa: E731
    ins = [z(b, length, 2), z(b, 13, 3), z(b, length), z(b, length), z(b, length, 3), z(b, 3)]
    n = model.grad_layout()[1]
    nbytes = int(lib.ttup_uplift_grad_workspace_bytes(model._handle, b, length))
    assert nbytes > 0
    ws = torch.zeros(nbytes // 4 + 8, device='cuda')
    assert ws.data_ptr() % 16 == 0
    outs = [torch.full(s, SENTINEL, device='cuda') for s in ((n,), (2,), (b, 3), (b, length, 3))]
    rc = lib.ttup_uplift_loss_grad(model._handle, *[_lib.ptr(t) for t in ins], b, length, flags, ctypes.c_void_p(ws.data_ptr() + shift), nbytes - short_by,
                                   *[_lib.ptr(t) for t in outs], _lib.stream_ptr())
    msg = lib.ttup_last_error()
    torch.cuda.synchronize()
    return rc, msg, all(bool((t == SENTINEL).all()) for t in outs)


def test_calls_outside_the_limits_are_refused_before_anything_is_written():
    """len = 256, 'local' on a single position, time_rotation='old' beyond the handle's RoPE table, a workspace one byte short and a
    misaligned one: TTUP_EINVAL with its message from the library, ValueError from Python, and -- the refusals come before the
    first memset -- the gradient, loss, rot and pos buffers keep what they held."""
    sd = weights.random_uplift_state_dict(5, 'small')
    new = make_model('small', sd, 'new', max_batch=2, max_len=16)
    old = make_model('small', sd, 'old', max_batch=2, max_len=16)
    for model, length, flags, kwargs, text in ((new, 256, 0, {}, b'sequence length 256 outside'), (new, 1, 1, {}, b"'local' needs at least two positions"),
                                               (old, 17, 0, {}, b"sequence length 17 above the handle's 16"), (new, 8, 0, {'short_by': 1}, b'workspace of'),
                                               (new, 8, 0, {'shift': 4}, b'16-byte aligned')):
        rc, msg, untouched = raw_call(model, 2, length, flags, **kwargs)
        assert rc == _lib.EINVAL and text in msg, (length, flags, kwargs, rc, msg)
        assert untouched, (length, flags, kwargs)
    rc, msg, untouched = raw_call(new, 2, 8, 0)          # the same call inside the limits runs, and writes
    assert rc == _lib.OK and not untouched
    z = lambda *s: torch.zeros(s)          # noqa: E731
    for model, length, mode, text in ((new, 256, 'global', 'sequence length 256 outside'), (new, 1, 'local', 'at least two positions'), (old, 17, 'global', "above the handle's 16")):
        with pytest.raises(ValueError, match=text):
            model.loss_and_grad(z(2, length, 2), z(2, 13, 3), z(2, length), z(2, length), z(2, length, 3), z(2, 3), transform_mode=mode, check_mask=False)


# ------------------------------------------------------------------ the mask format
def test_a_mask_that_forward_refuses_is_refused_here_too():
    """The reference's training step goes through model.forward, which raises ValueError unless the mask is {0,1} with both values
    present (model.py:541-546).  forward(check_mask=True) mirrors it; loss_and_grad(check_mask=True) must raise for the same masks.
    check_mask=False keeps the unchecked call: it raises for none of them and returns the bits of the checked call on a good mask."""
    seed, b, length = 7, 2, 8
    sd = weights.random_uplift_state_dict(seed, 'small')
    model = make_model('small', sd, max_batch=b, max_len=length)
    ball, table, mask, times, r_world, rotation = batch_inputs('ragged', b, length, seed, 2)
    assert set(np.unique(mask)) == {0.0, 1.0}
    half = mask.copy(); half[0, 1] = 0.5
    bad = {'all ones': np.ones_like(mask), 'all zeros': np.zeros_like(mask), 'one entry 0.5': half,
           'additive {-1e9, 0}': np.where(mask == 0, np.float32(-1e9), np.float32(0))}
    for name, m in bad.items():
        args = dev([ball, table, m, times, r_world, rotation])
        with pytest.raises(ValueError, match='wrong format for masks'):
            model.forward(*args[:4])
        with pytest.raises(ValueError, match='wrong format for masks'):
            model.loss_and_grad(*args)
    args = dev([ball, table, np.ones_like(mask), times, r_world, rotation])
    l_rot, l_pos, grads = model.loss_and_grad(*args, check_mask=False)          # today's behaviour: no check, numbers come back
    assert bool(torch.isfinite(grads.flat).all()) and bool(torch.isfinite(l_rot)) and bool(torch.isfinite(l_pos))
    args = dev([ball, table, mask, times, r_world, rotation])
    checked, unchecked = model.loss_and_grad(*args), model.loss_and_grad(*args, check_mask=False)
    assert_same_bits(checked, unchecked)
    assert torch.equal(checked[2].pos, unchecked[2].pos)
