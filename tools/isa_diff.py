#!/usr/bin/env python3
"""Compare the device code of csrc units between a git revision and the working tree, kernel by kernel.  Needs no GPU.

    python tools/isa_diff.py [--keep DIR] <rev> <unit>...          e.g.  python tools/isa_diff.py HEAD uplift.hip uplift_grad.hip

The revision's csrc/ and include/ are checked out to a temporary directory, both sides are compiled to gfx950 assembly with exactly
build.py's FLAGS (plus --cuda-device-only -S), and every kernel's text is compared after dropping comments, .loc / .file / .ident
lines, the per-build __hip_cuid_* symbol, the function's position in the unit that block labels carry and the section of its own that a
template instance gets.  Per kernel it prints
`identical` or the number of differing lines (a kernel found on one side only is paired with one of the other side that has the
same code under another name: `identical (was NAME)`) -- and, for a kernel that differs, whether the sequence of matrix, LDS and vector-memory instructions is still the same (the other differences a refactor
may leave are commuted integer address arithmetic, kernel-argument offsets and renamed symbols) -- followed by the resource
metadata (vgpr_count, sgpr_count, agpr_count, private_segment_fixed_size, group_segment_fixed_size) of both sides where they differ.
--keep DIR leaves the normalised text of every kernel that differs in DIR (<kernel>.old / .new) for diff(1).
Exit status 1 when a kernel's metadata changed or a kernel exists on one side only."""
import concurrent.futures
import difflib
import io
import os
import re
import shutil
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from upliftingtabletennis_amd.build import FLAGS, HIPCC  # noqa: E402

PKG = 'upliftingtabletennis_amd'
META = ('vgpr_count', 'sgpr_count', 'agpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')
HEAVY = ('v_mfma', 'v_smfma', 'ds_', 'global_', 'buffer_', 'flat_', 'scratch_')


def assemble(csrc, unit, out):
    cmd = [HIPCC] + FLAGS + ['--cuda-device-only', '-S', os.path.join(csrc, unit), '-o', out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise SystemExit('hipcc failed:\n%s\n%s' % (' '.join(cmd), r.stdout))
    with open(out) as f:
        return f.read().split('\n')


def kernels(lines):
    """{kernel symbol: (normalised body lines, metadata dict)}"""
    names = [ln.split()[1] for ln in lines if ln.strip().startswith('.amdhsa_kernel ')]
    body = {}
    for n in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(n + ':')) + 1
        out = []
        for ln in lines[start:]:
            if ln.startswith(('.Lfunc_end', '.section', '.amdhsa_kernel')):
                break
            s = re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid', ln.split(';')[0]).strip()
            s = re.sub(r'\.LBB\d+_', '.LBB_', s)          # block labels carry the function's position in the unit
            if re.match(r'\.section\s+\.text\.', s):          # a template instance lies in a comdat section of its own, a plain kernel in .text
                s = '.text'
            if s and not s.startswith(('.loc', '.file', '.ident')):
                out.append(re.sub(r'\s+', ' ', s))
        body[n] = out
    meta, cur = {}, None
    for ln in lines:
        if ln.startswith('  - '):          # a new entry of amdhsa.kernels (argument entries are indented deeper)
            cur = {}
        m = re.match(r'\s+(?:- )?\.(\w+):\s+(\S+)\s*$', ln)
        if m and cur is not None:
            if m.group(1) == 'name' and ln.startswith('    .name'):
                meta[m.group(2)] = cur
            elif m.group(1) in META:
                cur[m.group(1)] = int(m.group(2))
    return {n: (body[n], meta.get(n, {})) for n in names}


def heavy(body):
    return [ln.split(' ')[0] for ln in body if ln.startswith(HEAVY)]


def demangle(names):
    """kernel symbol -> `name<template arguments>`"""
    try:
        filt = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
        out = subprocess.run([filt] + names, stdout=subprocess.PIPE, text=True, check=True).stdout.split('\n')
    except (OSError, TypeError, subprocess.CalledProcessError):          # no demangler: the symbols as they are
        return {n: n for n in names}
    return {n: re.sub(r'^void ', '', o.replace('(anonymous namespace)::', '')).split('(')[0] for n, o in zip(names, out)}


def main():
    args = sys.argv[1:]
    keep = None
    if args[:1] == ['--keep']:
        keep, args = args[1], args[2:]
        os.makedirs(keep, exist_ok=True)
    if len(args) < 2:
        raise SystemExit(__doc__)
    rev, units = args[0], args[1:]
    bad = False
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(['git', '-C', ROOT, 'archive', rev, PKG + '/csrc', 'include'], stdout=subprocess.PIPE, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        jobs = []
        with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
            for u in units:
                jobs.append((u, ex.submit(assemble, os.path.join(tmp, PKG, 'csrc'), u, os.path.join(tmp, 'old_' + u + '.s')),
                             ex.submit(assemble, os.path.join(ROOT, PKG, 'csrc'), u, os.path.join(tmp, 'new_' + u + '.s'))))
        for u, fo, fn in jobs:
            old, new = kernels(fo.result()), kernels(fn.result())
            short = demangle(sorted(set(old) | set(new)))
            print('%s  (%s -> working tree)' % (u, rev))
            print('  %-64s %-34s %s' % ('kernel', 'code', ' '.join(m.replace('_fixed_size', '').replace('_count', '') for m in META)))
            renamed = {}          # a kernel of the working tree <- the revision's kernel with the same code under another name
            for n in set(new) - set(old):
                for o in set(old) - set(new) - set(renamed.values()):
                    if [ln.replace(o, n) for ln in old[o][0]] == new[n][0] and old[o][1] == new[n][1]:
                        renamed[n] = o
                        break
            for n in sorted(set(old) | set(new), key=lambda k: short[k]):
                if n in renamed.values():
                    continue
                if n in renamed:
                    print('  %-64s %-34s %s' % (short[n], 'identical (was %s)' % short[renamed[n]], ' '.join(str(new[n][1].get(k)) for k in META)))
                    continue
                if n not in old or n not in new:
                    side = new if n in new else old
                    print('  %-64s %-34s %s' % (short[n], 'only in ' + ('the working tree' if n in new else rev), ' '.join(str(side[n][1].get(k)) for k in META)))
                    if keep:
                        with open(os.path.join(keep, re.sub(r'\W+', '_', short[n]) + ('.new' if n in new else '.old')), 'w') as f:
                            f.write('\n'.join(side[n][0]) + '\n')
                    bad = True
                    continue
                (bo, mo), (bn, mn) = old[n], new[n]
                if bo == bn:
                    code = 'identical'
                else:
                    ops = difflib.SequenceMatcher(None, bo, bn, autojunk=False).get_opcodes()
                    nd = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in ops if tag != 'equal')
                    if keep:
                        for ext, b in (('.old', bo), ('.new', bn)):
                            with open(os.path.join(keep, re.sub(r'\W+', '_', short[n]) + ext), 'w') as f:
                                f.write('\n'.join(b) + '\n')
                    code = '%d of %d lines differ, mfma/lds/vmem %s' % (nd, len(bo), 'same' if heavy(bo) == heavy(bn) else 'CHANGED')
                ms = ' '.join(str(mn.get(k)) for k in META)
                if mo != mn:
                    ms += '   WAS ' + ' '.join(str(mo.get(k)) for k in META)
                    bad = True
                print('  %-64s %-34s %s' % (short[n], code, ms))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
