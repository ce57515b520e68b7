"""The uplift training loss and its parameter gradients on the MI355X, through the C-ABI (uplift.MultiStageModel.loss_and_grad ->
ttup_uplift_loss_grad), against the reference's own autograd (tests/golden/uplift_grad*.npz) and the torch restatement
(tests/helpers/uplift_torch_grad.py, pinned to that fixture by the CPU suite).  The reference is never read here.

Bar: the project's uplift bar of 1e-4, per tensor.  The fixture asserts that the reference's own reorder noise stays under 1e-5 per
tensor and that every tensor holds at least 1e-4 of the gradient's norm, so the bar sits 10x above the reference's noise.
Measured worst values per case: DESIGN.md 17.

The two comparisons against the restatement run on seeds vetted by the fixture tool's ReLU criterion (no ReLU input within 2^-24 of
the sum of its terms: below that its sign, and with it one token's whole gradient through that unit, depends on the order of
summation), applied to every layer over fewer than 1 / BAR = 10 000 rows, where one token is more than the bar's share of the rows;
the margin is computed by the restatement and asserted, so a host on which it does not hold fails loudly."""
import numpy as np
import pytest
import torch

from conftest import has_gpu
from helpers import uplift_grad_cases as C
from helpers import uplift_torch_grad as R

pytestmark = pytest.mark.gpu
if has_gpu():
    from upliftingtabletennis_amd import dataset, synth, uplift, weights

BAR = 1e-4
SEED_LARGE = 610
CASES = C.load_cases()


def make_model(size, sd, rot_kind='new', max_batch=64, max_len=128):
    return uplift.MultiStageModel(sd, size=size, max_batch=max_batch, max_len=max_len, time_rotation=rot_kind)


def dev(arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def to_numpy(grads):
    return {k: v.cpu().numpy() for k, v in grads.items()}


def rel_max(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


def assert_same_bits(a, b):
    (la0, la1, ga), (lb0, lb1, gb) = a, b
    assert torch.equal(ga.flat, gb.flat) and torch.equal(la0, lb0) and torch.equal(la1, lb1) and torch.equal(ga.rot, gb.rot)


@pytest.mark.parametrize('key', sorted(C.EXPECTED))
def test_gradients_match_the_reference_autograd(key):
    """Every case of the fixture, the time_rotation='old' and transform_mode='local' ones among them: every tensor within 1e-4
    (full tensors whole, sampled ones on their stored entries, every norm), embed.* exactly zero, losses / rot / pos within 1e-4."""
    c = CASES[key]
    model = make_model(c.size, c.state_dict(), c.rot_kind, max_batch=8)
    l_rot, l_pos, grads = model.loss_and_grad(*dev(c.inputs()), transform_mode=c.mode)
    assert [k for k in grads] == [k for k, _, _, _ in c.layout] and grads.flat.numel() == c.n_floats
    g = to_numpy(grads)
    for k in c.unused:
        assert not np.any(g[k]), k
    worst, worst_norm = c.compare(g)
    e_rot, e_pos = abs(float(l_rot) - c.loss[0]) / c.loss[0], abs(float(l_pos) - c.loss[1]) / c.loss[1]
    o_rot, o_pos = rel_max(grads.rot.cpu().numpy(), c.rot), rel_max(grads.pos.cpu().numpy(), c.pos)
    print('%s: worst tensor %.3e, worst norm %.3e, loss_rot %.3e, loss_pos %.3e, rot %.3e, pos %.3e (bar %.0e)' % (key, worst, worst_norm, e_rot, e_pos, o_rot, o_pos, BAR))
    assert np.isfinite(grads.flat.cpu().numpy()).all()
    assert worst <= BAR and worst_norm <= BAR
    assert e_rot <= BAR and e_pos <= BAR and o_rot <= BAR and o_pos <= BAR


KINK_ROWS = int(round(1 / BAR))


def training_batch(seed=410, b=64, t=43, pad=7):
    return list(synth.ragged_uplift_batch(b, t, seed=seed, pad=pad)) + list(synth.uplift_targets(b, t + pad, seed))


def against_restatement(size, seed, b, t, pad, max_len):
    """loss_and_grad of `b` trajectories against the restatement's autograd on the host CPU: every tensor in full, both losses, rot
    and pos at the bar; a second call returns the same bits.  -> worst relative L2 over the tensors"""
    sd = weights.random_uplift_state_dict(seed, size)
    inputs = training_batch(seed, b, t, pad)
    margins = []
    r_rot, r_pos, ref, ref_rot, ref_pos = R.loss_and_grad(sd, size, *inputs, margins=margins)
    margin = R.relu_margin(margins, KINK_ROWS)
    assert margin >= R.RELU_MARGIN, 'seed %d puts a ReLU input of a short layer on its kink (%.2e of its terms)' % (seed, margin)
    model = make_model(size, sd, max_batch=b, max_len=max_len)
    first = model.loss_and_grad(*dev(inputs))
    l_rot, l_pos, grads = first
    assert_same_bits(first, model.loss_and_grad(*dev(inputs)))
    g = to_numpy(grads)
    worst, at = 0.0, None
    for k, shape, off, used in grads_layout(size):
        if not used:
            assert ref[k] is None and not np.any(g[k]), k
            continue
        assert np.isfinite(g[k]).all(), k
        e = np.linalg.norm((g[k] - ref[k]).astype(np.float64)) / np.linalg.norm(ref[k].astype(np.float64))
        if e > worst:
            worst, at = e, k
    e_rot, e_pos = abs(float(l_rot) - r_rot) / r_rot, abs(float(l_pos) - r_pos) / r_pos
    o_rot, o_pos = rel_max(grads.rot.cpu().numpy(), ref_rot), rel_max(grads.pos.cpu().numpy(), ref_pos)
    print('%s B=%d T=%d against the restatement: worst tensor %.3e (%s), loss_rot %.3e, loss_pos %.3e, rot %.3e, pos %.3e; smallest ReLU margin over layers of < %d rows %.2e'
          % (size, b, t + pad, worst, at, e_rot, e_pos, o_rot, o_pos, KINK_ROWS, margin))
    assert worst <= BAR
    assert e_rot <= BAR and e_pos <= BAR and o_rot <= BAR and o_pos <= BAR
    return worst


def test_gradients_match_the_restatement_at_the_training_shape():
    """large, B = 64 (the reference's BATCH_SIZE), T = 50: every tensor in full."""
    against_restatement('large', SEED_LARGE, 64, 43, 7, 128)


def test_batch_larger_than_a_group_matches_the_restatement():
    """The pass cuts a batch into groups of 262 144 // (14 len) trajectories that share the workspace; the gradients and the loss
    terms accumulate over the groups, every group reads its own rows of the eight arrays, and loss_pos is normalised by the whole
    batch's mask sum.  small, T = 250: a group holds 74 trajectories, so 80 are a full group and a ragged one of 6."""
    assert 262144 // (14 * 250) == 74
    against_restatement('small', 420, 80, 243, 7, 256)


def grads_layout(size):
    from upliftingtabletennis_amd import arch
    return arch.uplift_grad_layout(size)[0]


def test_two_calls_and_another_chunking_return_the_same_bits():
    """No floating-point atomics: a second call returns the same bits, and so does a handle whose scratch holds fewer trajectories
    than the batch (max_len 4096: its forward would run 64 trajectories in two chunks) -- the gradient pass never looks at it."""
    sd = weights.random_uplift_state_dict(411, 'large')
    inputs = dev(training_batch(411))
    model = make_model('large', sd)
    first = model.loss_and_grad(*inputs)
    assert_same_bits(first, model.loss_and_grad(*inputs))
    other = make_model('large', sd, max_batch=64, max_len=4096)
    assert_same_bits(first, other.loss_and_grad(*inputs))
    assert torch.equal(first[2].pos, other.loss_and_grad(*inputs)[2].pos)


@pytest.mark.parametrize('rot_kind', ['new', 'old'])
def test_masked_rows_are_inert(rot_kind):
    """Large finite values in the padded slots of ball, times and r_world, and in the xy of invisible keypoints, change no bit of any
    gradient, of the losses or of rot; everything stays finite."""
    sd = weights.random_uplift_state_dict(412, 'large', time_rotation=rot_kind)
    ball, table, mask, times, r_world, rotation = training_batch(412, b=16)
    assert (mask == 0).any() and (table[:, :, 2] == 0).any()
    model = make_model('large', sd, rot_kind)
    base = model.loss_and_grad(*dev([ball, table, mask, times, r_world, rotation]))
    pad = mask == 0
    ball2, times2, world2, table2 = ball.copy(), times.copy(), r_world.copy(), table.copy()
    ball2[pad] = 3.0e3; times2[pad] = 977.123; world2[pad] = -4.0e4
    table2[table[:, :, 2] == 0, :2] = 2.5e3
    for changed in ([ball2, table, mask, times2, world2, rotation], [ball, table2, mask, times, r_world, rotation], [ball2, table2, mask, times2, world2, rotation]):
        got = model.loss_and_grad(*dev(changed))
        assert_same_bits(base, got)
        keep = torch.from_numpy(mask != 0).cuda()
        assert torch.equal(base[2].pos[keep], got[2].pos[keep])
        for t in (got[0], got[1], got[2].flat, got[2].rot, got[2].pos):
            assert bool(torch.isfinite(t).all())


def test_forward_is_untouched_and_agrees_with_the_gradient_pass():
    sd = weights.random_uplift_state_dict(413, 'large')
    inputs = dev(training_batch(413))
    model = make_model('large', sd)
    rot0, pos0 = model.forward(*inputs[:4])
    _, _, grads = model.loss_and_grad(*inputs)
    rot1, pos1 = model.forward(*inputs[:4])
    assert torch.equal(rot0, rot1) and torch.equal(pos0, pos1)
    keep = inputs[2] != 0          # (a padded slot's own pos row is whatever its padding gives: both paths compute it, neither uses it)
    e_rot = rel_max(grads.rot.cpu().numpy(), rot0.cpu().numpy().astype(np.float64))
    e_pos = rel_max(grads.pos[keep].cpu().numpy(), pos0[keep].cpu().numpy().astype(np.float64))
    print('gradient pass against forward: rot %.3e pos %.3e' % (e_rot, e_pos))
    assert e_rot <= BAR and e_pos <= BAR


def test_unsupported_variant_is_refused_by_the_library_too():
    import ctypes
    from upliftingtabletennis_amd import _lib
    sd = weights.random_uplift_state_dict(5, 'small', 'multistage', 'stacked')
    model = uplift.MultiStageModel(sd, size='small', max_batch=4, max_len=32, name='multistage', mode='stacked')
    n, k = ctypes.c_longlong(0), ctypes.c_int(0)
    assert model._lib.ttup_uplift_grad_layout(model._handle, ctypes.byref(n), ctypes.byref(k), None, None, 0) == _lib.EINVAL
    assert b'multistage/stacked' in model._lib.ttup_last_error()
    assert model._lib.ttup_uplift_grad_workspace_bytes(model._handle, 4, 20) == 0
    z = torch.zeros(4096, device='cuda')
    rc = model._lib.ttup_uplift_loss_grad(model._handle, *[_lib.ptr(z)] * 6, 4, 20, 0, _lib.ptr(z), 16384, *[_lib.ptr(z)] * 4, _lib.stream_ptr())
    assert rc == _lib.EINVAL and b'multistage/stacked' in model._lib.ttup_last_error()
    with pytest.raises(ValueError, match='multistage/stacked'):
        model.loss_and_grad(z, z, z, z, z, z)


def test_samples_built_on_the_device_go_straight_into_the_gradient_pass(golden):
    """End of the chain: dataset.TableTennisDataset.batch -> loss_and_grad on the batch's own device tensors (float32, contiguous:
    the call makes no copy of them), against the same call on the fixture's copy of those samples.  The device build is held to 2
    float32 ulps of the fixture (test_dataset_gpu.py); it has been bit-equal on every MI355X run, and then the two calls must return
    the same bits.  Were an input to differ in its last bits, the results are held to the bar instead; which of the two was checked
    is printed."""
    from test_dataset_gpu import make_dataset
    g = golden('dataset.npz')
    ds = make_dataset(g, 'full')
    b = ds.batch(g['full/traj'], g['full/seed'])
    sd = weights.random_uplift_state_dict(414, 'large')
    model = make_model('large', sd, max_batch=128)
    rows = (b.r_img, b.table_img, b.mask, b.times, b.r_world, b.rotation)
    for t in rows:
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        assert t.to(model.device, torch.float32).contiguous().data_ptr() == t.data_ptr()          # what loss_and_grad does with it
    l_rot, l_pos, grads = model.loss_and_grad(*rows)
    host = [g['full/' + k].astype(np.float32) for k in ('r_img', 'table_img', 'mask', 'times', 'r_world', 'rotation')]
    same_inputs = all(np.array_equal(t.cpu().numpy(), h) for t, h in zip(rows, host))
    r_rot, r_pos, ref = model.loss_and_grad(*dev(host))
    worst = max(float(torch.linalg.norm((grads[k] - ref[k]).double()) / torch.linalg.norm(ref[k].double())) for k, _, _, used in grads_layout('large') if used)
    print('device-built samples against the fixture copy: inputs bit-identical %s -> checked %s; worst tensor %.3e' % (same_inputs, 'bit equality' if same_inputs else 'the 1e-4 bar', worst))
    assert bool(torch.isfinite(grads.flat).all())
    if same_inputs:
        assert_same_bits((l_rot, l_pos, grads), (r_rot, r_pos, ref))
    assert worst <= BAR
    assert abs(float(l_rot) - float(r_rot)) <= BAR * float(r_rot) and abs(float(l_pos) - float(r_pos)) <= BAR * float(r_pos)
