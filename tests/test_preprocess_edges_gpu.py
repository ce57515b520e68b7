"""The pre-processing kernels (csrc/conv_pointwise.h) against the oracle's fixed-point resize and float64 normalisation table
(oracle/glue_ref.py), bit for bit, at the shapes where they change path: clamps on all four sides, taps that are not loaded, odd and
one-pixel sources, column-block tails, the clip's last pixel, the smallest clips (cases: tests/helpers/preprocess_edge_cases.py;
tests/test_preprocess_edges_host.py shows on the CPU that the table reaches those branches).  The resize is integer arithmetic and
the table is rounded once, so the bar is equality; a tolerance would hide a one-grey-level error.

The records written inside the nets cannot be read back as such: preprocess_frames4_kernel is compared with the general kernel
through the heatmaps, indices and windows of `forward_frames` here, and the records against the oracle through the first conv's taps
in tests/test_wasb_taps_gpu.py and tests/test_wasb_f32_taps_gpu.py (cases *_pre_*)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import has_gpu
from helpers import preprocess_edge_cases as P

pytestmark = pytest.mark.gpu
if has_gpu():
    from upliftingtabletennis_amd import wasb


def _equal_bits(got, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    return got.shape == ref.shape and got.dtype == ref.dtype and np.array_equal(got.view(np.int32), ref.view(np.int32))


def _where(got, ref):
    got = got.cpu().numpy()
    bad = np.argwhere(got != ref)
    return '%d of %d values differ, first at %s: %r against %r' % (len(bad), ref.size, bad[0].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])]) if len(bad) else 'shapes %s %s' % (got.shape, ref.shape)


@pytest.mark.parametrize('case', P.CASES, ids=lambda c: c.id)
def test_both_entry_points_match_the_oracle_bit_for_bit(case):
    clip = P.frames(case)
    dev = torch.from_numpy(clip.copy()).cuda()
    ref = P.oracle_frames(clip, case)
    got = wasb.preprocess_frames(dev, (case.dw, case.dh))
    assert _equal_bits(got, ref), _where(got, ref)
    ref3 = P.oracle_triples(clip, case)
    assert ref3.shape == (P.N_FRAMES - 2, 9, case.dh, case.dw)
    got3 = wasb.preprocess_triples(dev, (case.dw, case.dh))
    assert _equal_bits(got3, ref3), _where(got3, ref3)


@pytest.mark.parametrize('cid', P.SMALLEST_IDS)
def test_smallest_clips(cid):
    """Exactly three frames give one triple, exactly one frame one sample: the clip ends right behind the only sample's last frame."""
    case = P.BY_ID[cid]
    clip = P.frames(case)
    three, one = clip[:3], clip[1:2]
    got3 = wasb.preprocess_triples(torch.from_numpy(three.copy()).cuda(), (case.dw, case.dh))
    ref3 = P.oracle_triples(three, case)
    assert ref3.shape[0] == 1 and _equal_bits(got3, ref3), _where(got3, ref3)
    got1 = wasb.preprocess_frames(torch.from_numpy(one.copy()).cuda(), (case.dw, case.dh))
    ref1 = P.oracle_frames(one, case)
    assert ref1.shape[0] == 1 and _equal_bits(got1, ref1), _where(got1, ref1)


@pytest.mark.parametrize('cid', P.LAST_PIXEL_IDS)
@pytest.mark.parametrize('side', ['behind', 'before'])
def test_the_clips_last_pixel_and_the_bytes_around_the_clip(cid, side):
    """The last frame is dark but for its last pixel, which the last output pixel reads; the clip is a slice of a larger device buffer
    whose bytes behind (or before) the slice are 0 in one run and 255 in the other.  Neither may reach the output: both runs equal
    each other and the oracle.  This shows that no foreign byte is used as pixel data and that the last pixel's three bytes arrive.
    It does NOT show that the byte-load fallback for the clip's last pixel is taken: the fourth byte of the 4-byte load is masked off
    on every path, so an over-read by one byte would give the same output.  The odd offset of the slice moves every 4-byte load off
    its alignment."""
    case = P.BY_ID[cid]
    clip = P.last_pixel_frames(case)
    ref, ref3 = P.oracle_frames(clip, case), P.oracle_triples(clip, case)
    # the planted pixel is what the last output pixel shows: not the dark level
    dark = P.oracle_frames(np.zeros_like(clip[-1:]), case)[0, :, -1, -1]
    assert (ref[-1, :, -1, -1] != dark).all()
    n, pad = clip.size, 67
    outs = []
    for fill in (0, 255):
        buf = torch.full((pad + n + pad,), 7, dtype=torch.uint8, device='cuda')
        if side == 'behind':
            buf[pad + n:] = fill
        else:
            buf[:pad] = fill
        buf[pad:pad + n] = torch.from_numpy(clip.reshape(-1)).cuda()
        view = buf[pad:pad + n].view(clip.shape)
        assert view.data_ptr() == buf.data_ptr() + pad and view.is_contiguous()
        outs.append((wasb.preprocess_frames(view, (case.dw, case.dh)), wasb.preprocess_triples(view, (case.dw, case.dh))))
        torch.cuda.synchronize()
        assert torch.equal(buf[:pad].cpu(), torch.full((pad,), fill if side == 'before' else 7, dtype=torch.uint8))
    for got, got3 in outs:
        assert _equal_bits(got, ref), _where(got, ref)
        assert _equal_bits(got3, ref3), _where(got3, ref3)
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))


def test_frame_record_fast_path_equals_the_general_kernel_at_its_block_edges(tmp_path):
    """preprocess_frames4_kernel (equal source and network width; 4 pixels per thread, 1024 per workgroup, 4 rows per workgroup)
    against preprocess_kernel<bf16_t> writing the same records: heatmaps, indices and windows of `forward_frames` are bit-identical
    with TTUP_NO_PRE4=1, at widths below one block, one record short of it, exactly one and one record past it, with upscaled,
    downscaled and identical rows.  The switch is read once per process: one fresh child per setting, one after the other."""
    script = (
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "from upliftingtabletennis_amd import wasb, weights\n"
        "sd = weights.random_wasb_state_dict(47, planted=True)\n"
        "out = {}\n"
        "for nw in %r:\n"
        "    net = wasb.WASBNet(sd, resolution=(nw, %d), max_batch=4, dtype='bf16')\n"
        "    for sh in %r:\n"
        "        fr = torch.from_numpy(np.random.default_rng(nw + sh).integers(0, 256, (5, sh, nw, 3), dtype=np.uint8)).cuda()\n"
        "        h, i, w = net.forward_frames(fr, want_heatmap=True)\n"
        "        k = '%%d_%%d' %% (nw, sh)\n"
        "        out['h' + k], out['i' + k], out['w' + k] = h.cpu().numpy(), i.cpu().numpy(), w.cpu().numpy()\n"
        "np.savez(sys.argv[1], **out)\n"
    ) % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), P.FAST_WIDTHS, P.FAST_NET_H, P.FAST_SRC_H)
    outs = {}
    for tag, env in (('fast', {}), ('general', {'TTUP_NO_PRE4': '1'})):
        out = str(tmp_path / (tag + '.npz'))
        e = dict(os.environ); e.pop('TTUP_NO_PRE4', None); e.update(env)
        r = subprocess.run([sys.executable, '-c', script, out], env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = np.load(out)
    assert len(outs['fast'].files) == 3 * len(P.FAST_WIDTHS) * len(P.FAST_SRC_H)
    for k in outs['fast'].files:
        a, b = outs['fast'][k], outs['general'][k]
        assert a.shape == b.shape and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b), k
    # the heatmaps are not all alike: the frames reach the output
    assert not np.array_equal(outs['fast']['h1024_24'], outs['fast']['h1024_36'])
