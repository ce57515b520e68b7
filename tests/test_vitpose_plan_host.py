"""The ViTPose detector's device-free decisions (csrc/vitpose_plan.h) on the CPU, through the stand-alone program
tests/helpers/host_vitpose_plan.cpp built with AddressSanitizer and UndefinedBehaviorSanitizer.  The program runs as a child
process (nothing of it is loaded into python) and carries its sanitizer runtimes itself (linked statically); every run must end with
status 0 and an empty stderr, i.e. without a sanitizer report.

Layout: the C++ tensor table -- from which ttup_vitpose_create sets every weight pointer -- against weights.vitpose_schema,
weights.pack_vitpose_blob and the sizes include/ttup.h documents.  Refusals: what ttup_vitpose_create turns away before it touches a
device.  Buffers: the arena of every edge shape x micro-batch x dtype on 256-byte boundaries, disjoint, inside the total, and large
enough for every step of the forward's GEMM list.  Taps: the C++ table against vitpose.TAPS.  The micro-batch rule on a table."""
import os
import subprocess

import numpy as np
import pytest

from helpers import vitpose_edge_cases as edges
from upliftingtabletennis_amd import _lib, vitpose, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM, DEPTH, MLP, DEC = weights.VITPOSE_DIM, weights.VITPOSE_DEPTH, weights.VITPOSE_MLP, weights.VITPOSE_DECONV
# (h, w, in_ch, out_ch): every shape of the edge sweep, and the two detectors at their own resolution
SHAPES = sorted({c[:4] for c in edges.CASES}) + [(640, 1152, 9, 1), (640, 1152, 3, 13)]


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('hostvitplan') / 'host_vitpose_plan')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-static-libubsan', '-o', exe,
                           os.path.join(ROOT, 'tests', 'helpers', 'host_vitpose_plan.cpp')])
    return exe


def run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == '', (args, r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def layout(prog, in_ch, out_ch, n_pos):
    """(total, [(offset, count)] in blob order, {name: offset})"""
    out = run(prog, 'layout', in_ch, out_ch, n_pos)
    head = out[0].split()
    assert (head[0], head[2]) == ('tensors', 'total')
    recs = [tuple(int(v) for v in l.split()[1:]) for l in out[1:] if l.startswith('t ')]
    assert len(recs) == int(head[1])
    return int(head[3]), recs, {l.split()[1]: int(l.split()[2]) for l in out if l.startswith('at ')}


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%d_%dto%d' % s)
def test_layout_is_the_packed_blob(prog, shape):
    """Total, backbone offsets and folded-head sizes; four tensors read back from the blob at the table's offsets."""
    h, w, cin, cout = shape
    n_pos = (h // 16) * (w // 16) + 1
    total, recs, at = layout(prog, cin, cout, n_pos)
    sd = weights.random_vitpose_state_dict(3, in_ch=cin, out_ch=cout, resolution=(w, h))
    blob = weights.pack_vitpose_blob(sd, in_ch=cin, out_ch=cout)
    assert 40 + 4 * total == len(blob)
    # the backbone: the schema's tensors in its order, offsets their running sum
    schema = weights.vitpose_schema(cin, cout, resolution=(w, h))
    backbone = [(k, int(np.prod(s))) for k, s in schema if '.backbone.' in k]
    assert len(backbone) == 3 + 12 * DEPTH + 2
    off = 0
    for (k, count), rec in zip(backbone, recs):
        assert rec == (off, count), k
        off += count
    # the head, BN folded into four 2x2 sub-convolutions per deconvolution
    assert [c for _, c in recs[len(backbone):]] == [4 * DEC * 4 * DIM, DEC, 4 * DEC * 4 * DEC, DEC, cout * DEC, cout]
    assert [o for o, _ in recs[len(backbone):]] == [at[k] for k in ('dc_w0', 'dc_b0', 'dc_w1', 'dc_b1', 'fin_w', 'fin_b')]
    assert recs[-1][0] + recs[-1][1] == total

    def tensor(name, key):
        v = sd[key]
        got = np.frombuffer(blob, np.float32, v.size, 40 + 4 * at[name])
        assert np.array_equal(got, v.ravel()), key
    tensor('pos', 'model.backbone.pos_embed')
    tensor('blk5.qkvw', 'model.backbone.blocks.5.attn.qkv.weight')
    tensor('lnw', 'model.backbone.last_norm.weight')
    tensor('fin_b', 'model.keypoint_head.final_layer.bias')


def test_refusals_need_no_device(prog, tmp_path):
    """ttup_vitpose_create's answer to a wrong size, channel count or blob: TTUP_EINVAL for the arguments (before the blob is
    looked at), TTUP_EFORMAT for the blob."""
    case = edges.find(16, 16)
    h, w, cin, cout, _, _ = case
    blob = weights.pack_vitpose_blob(edges.state_dict(case), in_ch=cin, out_ch=cout)
    path = str(tmp_path / 'blob.bin')
    with open(path, 'wb') as f:
        f.write(blob)

    def create(height=h, width=w, in_ch=cin, out_ch=cout, max_batch=2, micro=0, path=path, delta=None):
        args = (height, width, max_batch, micro, in_ch, out_ch)
        out = run(prog, 'create', path, *args) if delta is None else run(prog, 'create_resized', path, delta, *args)
        return int(out[0].split()[1]), out[1] if len(out) > 1 else ''
    assert create() == (_lib.OK, '')
    for bad in (dict(height=8), dict(width=8), dict(height=24), dict(width=40), dict(height=0), dict(height=-16)):
        rc, msg = create(**bad)
        assert rc == _lib.EINVAL and 'multiples of 16' in msg, (bad, msg)
    for bad in (dict(out_ch=17), dict(out_ch=0), dict(in_ch=0), dict(max_batch=0), dict(micro=-1)):
        rc, msg = create(**bad)
        assert rc == _lib.EINVAL and 'in_ch' in msg and 'out_ch' in msg, (bad, msg)
    for bad in (dict(in_ch=3), dict(out_ch=2)):
        rc, msg = create(**bad)
        assert rc == _lib.EFORMAT and 'asked for' in msg, (bad, msg)
    for bad in (dict(height=32), dict(width=48)):          # n_pos 2 + 1 / 3 + 1 against the blob's 1 + 1
        rc, msg = create(**bad)
        assert rc == _lib.EFORMAT and 'pos_embed' in msg, (bad, msg)
    for delta in (-1, 1):
        rc, msg = create(delta=delta)
        assert rc == _lib.EFORMAT and '%d bytes, expected %d' % (len(blob) + delta, len(blob)) in msg, (delta, msg)
    # the header alone: under a wrong magic it is no blob, under the right one it is short; fewer than 40 bytes are never read
    for name, data, want in (('magic', b'TTUPVIT2' + blob[8:40], 'not a ViTPose blob'), ('header', blob[:40], 'bytes, expected'),
                             ('short', blob[:39], 'not a ViTPose blob'), ('depth', blob[:20] + b'\x0b\0\0\0' + blob[24:40], 'ViTPose-small')):
        p = str(tmp_path / name)
        with open(p, 'wb') as f:
            f.write(data)
        rc, msg = create(path=p)
        assert rc == _lib.EFORMAT and want in msg, (name, msg)


def test_buffers_are_aligned_disjoint_and_large_enough(prog):
    """Every shape x micro {1, 2, 8} x dtype {f32, bf16}: 256-byte boundaries (2 MiB for a buffer of 2 MiB or more), no overlap,
    stats64 on bf16 handles only, frames of micro + in_ch / 3 - 1 records where in_ch is a whole number of frames; every step of the
    GEMM list fits its output buffer at batch = micro (deconvolution 1 in hid, last_norm in att), reads a buffer it does not write,
    and lies on both kernels' tiles."""
    lines = run(prog, 'buffers', *[v for s in SHAPES for v in s])
    assert not [l for l in lines if l.startswith('FAIL')], lines[:20]
    assert lines[-2:] == ['cases %d' % (len(SHAPES) * 6), 'failures 0']


def test_tap_table_is_vitpose_taps(prog):
    lines = run(prog, 'taps')
    assert lines[0] == 'stages %d depth %d' % (vitpose.STAGES, DEPTH) and vitpose.STAGES == DEPTH + 2
    taps = {l.split()[1]: tuple(int(v) for v in l.split()[2:]) for l in lines[1:]}
    assert len(taps) == len(lines) - 1 and set(taps) == set(vitpose.TAPS)
    for name, (first, last, cols, narrow) in taps.items():
        assert (cols or None, bool(narrow)) == vitpose.TAPS[name], name
        # stage 0 leaves x alone; the blocks x, x_attn, qkv, att, hid; the head ln, d1, d2, heat
        want = (0, DEPTH) if name == 'x' else (DEPTH + 1, DEPTH + 1) if name in ('ln', 'd1', 'd2', 'heat') else (1, DEPTH)
        assert (first, last) == want, name


def test_micro_batch_rule(prog):
    table = {(32, 0): 8, (3, 0): 3, (3, 2): 2, (2, 5): 2, (1, 0): 1, (8, 0): 8, (9, 0): 8, (32, 32): 32}
    out = run(prog, 'micro', *[v for k in table for v in k])
    assert [int(l) for l in out] == list(table.values())
