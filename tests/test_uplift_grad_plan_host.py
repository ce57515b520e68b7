"""The uplift gradient pass's device-free decisions (csrc/uplift_grad_plan.h) on the CPU, through the stand-alone program
tests/helpers/host_uplift_grad_plan.cpp built with AddressSanitizer and UndefinedBehaviorSanitizer.  The program runs as a child
process (nothing of it is loaded into python) and carries its sanitizer runtimes itself (linked statically); every run must end with
status 0 and an empty stderr, i.e. without a sanitizer report.

Layout: the C++ tensor table -- which ttup_uplift_grad_layout, the parameter walk of the pass and the optimizer's hole all read --
against arch.uplift_grad_layout / arch.uplift_grad_hole, the Python statement of the same facts.  Groups: group_size on a table.
Workspace: every buffer of the plan on a 16-byte boundary, disjoint, inside the total and at least as large as what a full group
puts into it, the sliced-reduction scratch included, over sizes x batches x lengths.  Attention: the launch geometry of every head
dim and sequence length, and the one "is this length served" decision the entry point takes."""
import os
import subprocess

import pytest

from upliftingtabletennis_amd import arch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = tuple(arch.UPLIFT_SIZES)
N_TABLE = 13


@pytest.fixture(scope='module')
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('hostgradplan') / 'host_uplift_grad_plan')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-static-libasan', '-static-libubsan', '-o', exe,
                           os.path.join(ROOT, 'tests', 'helpers', 'host_uplift_grad_plan.cpp')])
    return exe


def run(prog, *args):
    r = subprocess.run([prog] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stderr == '', (args, r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def dims(size):
    """D, head dim, table keypoints and the three stages' layer counts of connectstage/dynamic"""
    d, _, heads = arch.UPLIFT_SIZES[size]
    pos, first, second = arch.uplift_variant_layers('connectstage', size, 'dynamic')
    return d, d // heads, N_TABLE, len(pos), len(first), len(second)


def _no_failures(lines):
    assert not [l for l in lines if l.startswith('FAIL')], lines[:20]
    assert lines[-1] == 'failures 0', lines[-3:]
    return lines


@pytest.mark.parametrize('size', SIZES)
def test_layout_table_is_arch_uplift_grad_layout(prog, size):
    """Count, offset, element count and `used` of every tensor, the total and the hole."""
    out = run(prog, 'layout', *dims(size))
    layout, n_floats = arch.uplift_grad_layout(size)
    head = out[0].split()
    assert (head[0], head[2], head[4]) == ('tensors', 'total', 'hole')
    assert (int(head[1]), int(head[3])) == (len(layout), n_floats)
    assert (int(head[5]), int(head[6])) == arch.uplift_grad_hole(size)
    recs = [tuple(int(v) for v in l.split()[1:]) for l in out[1:]]
    assert len(recs) == len(layout)
    for (n, k, off, used), (name, shape, want_off, want_used) in zip(recs, layout):
        assert (off, n * k if k else n, bool(used)) == (want_off, arch._numel(shape), want_used), name
        assert (n, k) == (tuple(shape) if len(shape) == 2 else (shape[-1], 0)), name          # cls_token is (1, 1, D)


GROUPS = [  # batch, len
    (100, 250), (100, 255), (74, 250), (73, 250), (75, 250), (73, 255), (72, 255), (74, 255), (1, 1), (5, 1), (20000, 1), (18724, 1), (18725, 1),
    (80, 128), (4, 18724), (4, 18725), (4, 9363), (4, 9362), (1, 100000), (64, 17), (2, 171),
]


def test_group_size_table(prog):
    out = run(prog, 'group', *[v for case in GROUPS for v in case])
    assert [int(l) for l in out] == [min(b, max(1, 262144 // (14 * t))) for b, t in GROUPS]
    got = dict(zip(GROUPS, (int(l) for l in out)))
    assert got[(100, 250)] == 74 and got[(100, 255)] == 73          # the trainer's lengths
    assert got[(4, 18725)] == 1 and got[(4, 9363)] == 1 and got[(4, 9362)] == 2 and got[(1, 100000)] == 1          # long enough for one trajectory a group
    assert (got[(73, 250)], got[(74, 250)], got[(75, 250)]) == (73, 74, 74)          # batch below, at and above the group size


@pytest.mark.parametrize('size', SIZES)
def test_workspace_buffers_are_aligned_disjoint_and_large_enough(prog, size):
    """batch {1, 2, 3, 5, 64, 80} x len {1, 2, 15, 16, 17, 64, 128, 171, 250, 255}"""
    lines = _no_failures(run(prog, 'workspace', *dims(size)))
    assert lines[-2] == 'cases 60'


def test_attention_geometry_of_every_length(prog):
    """hd {8, 16, 24, 32} x S 1 .. 256 x {forward, backward}: P the smallest power of two >= max(16, S), 64 / P sequences a workgroup
    below 64, at most 256 threads, at most 160 KB of LDS; S = 257 and other head dims are refused.  The largest launch is the
    backward one at hd 32, S 256: (4 * 256 * 32 + 3 * 256 + 256) * 4 bytes."""
    lines = _no_failures(run(prog, 'attention'))
    assert lines[-2] == 'cases %d max_lds %d' % (4 * 257 * 2 + 5, (4 * 256 * 32 + 3 * 256 + 256) * 4)
    assert (4 * 256 * 32 + 3 * 256 + 256) * 4 == 135168


def test_served_lengths(prog):
    """Every size at len 255 (a spin stage of 256 tokens) is served; len 256 is not."""
    for size in SIZES:
        hd = dims(size)[1]
        assert run(prog, 'served', hd, N_TABLE, 255) == ['1'], size
        assert run(prog, 'served', hd, N_TABLE, 1) == ['1'], size
        assert run(prog, 'served', hd, N_TABLE, 256) == ['0'], size
    assert run(prog, 'served', 12, N_TABLE, 16) == ['0']          # a head dim without a kernel
