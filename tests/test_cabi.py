"""CPU-only checks of the boundary: the library loads, exports every symbol include/ttup.h declares,
argument validation works without a GPU, and the host-side mirror functions match the goldens."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from upliftingtabletennis_amd import _lib, arch, glue, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from upliftingtabletennis_amd import build
        build.build()
    return _lib.load()


def test_header_symbols_exported(lib):
    hdr = open(os.path.join(ROOT, 'include', 'ttup.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    names = set(re.findall(r'\b(ttup_[a-z_0-9]+)\s*\(', hdr))
    assert names == set(_lib.SIGNATURES), names ^ set(_lib.SIGNATURES)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.ttup_version() >= 101


def test_library_carries_the_hash_of_this_trees_sources(lib, tmp_path, monkeypatch):
    """nothing tied the loaded libttup.so to HEAD's sources (objects are git-ignored and travel to the GPU box as
    built).  build.py hashes csrc/*.hip, csrc/*.h, include/ttup.h and the flags into the library; the binding refuses a mismatch."""
    from upliftingtabletennis_amd import build
    assert lib.ttup_build_id().decode() == build.source_id() == _lib.build_id()
    assert re.fullmatch(r'[0-9a-f]{16}', build.source_id())
    # a different tree (one more source file) -> a different id -> the check raises
    real = build.source_id
    monkeypatch.setattr(build, 'source_id', lambda: 'f' * 16)
    monkeypatch.delenv('TTUP_LIB', raising=False)
    monkeypatch.delenv('TTUP_ALLOW_STALE_LIB', raising=False)
    with pytest.raises(RuntimeError, match='built from other sources'):
        _lib._check_build_id(lib)
    monkeypatch.setattr(build, 'source_id', real)
    _lib._check_build_id(lib)


def test_no_swizzled_packed_fp32_in_the_device_code(tmp_path):
    """csrc/common.h: v_pk_*_f32 instructions that carry op_sel / op_sel_hi / neg modifiers were measured to return wrong values on
    gfx950 beside another kernel's LDS-fed MFMAs (tools/pk_coresidency_repro.hip).  The shipped library must contain none: every
    gfx950 code object of libttup.so is disassembled and scanned (the plain element-wise forms are fine and stay).
    The same scan refuses out-of-line CALLS in the device code (s_swappc_b64): a unit compiled with no-packed-fp32-ops cannot inline
    a HIP header function that lacks the attribute, which in round 3 left 1852 calls (__uint_as_float, __shfl_xor, __syncthreads ...)
    inside the uplift kernels' hot loops unnoticed (csrc/no_packed_fp32_begin.h)."""
    import struct
    objcopy, objdump = '/opt/rocm/lib/llvm/bin/llvm-objcopy', '/opt/rocm/lib/llvm/bin/llvm-objdump'
    if not (os.path.exists(objcopy) and os.path.exists(objdump)):
        pytest.skip('llvm binutils not found')
    fat = tmp_path / 'fat.bin'
    subprocess.run([objcopy, '--dump-section', '.hip_fatbin=%s' % fat, _lib.LIB_PATH, str(tmp_path / 'stripped.so')], check=True)
    data = fat.read_bytes()
    magic = b'__CLANG_OFFLOAD_BUNDLE__'
    n_objects, n_packed, bad, calls = 0, 0, [], 0
    start = data.find(magic)
    while start >= 0:
        (n_entries,) = struct.unpack_from('<Q', data, start + len(magic))
        p = start + len(magic) + 8
        for _ in range(n_entries):
            off, size, tlen = struct.unpack_from('<QQQ', data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if 'gfx950' not in triple or size == 0:
                continue
            co = tmp_path / ('dev%d.co' % n_objects)
            co.write_bytes(data[start + off:start + off + size])
            n_objects += 1
            asm = subprocess.run([objdump, '-d', '--no-show-raw-insn', str(co)], check=True, capture_output=True, text=True).stdout
            for line in asm.splitlines():
                calls += 's_swappc_b64' in line
                if re.search(r'v_pk_[a-z]+_f32', line):
                    n_packed += 1
                    if re.search(r'op_sel|neg_lo|neg_hi', line):
                        bad.append(line.strip())
        start = data.find(magic, start + 1)
    assert n_objects >= 8, 'expected one gfx950 code object per translation unit, found %d' % n_objects
    assert n_packed > 0, 'the scan found no packed fp32 instruction at all: is the disassembly empty?'
    assert not bad, '%d swizzled packed fp32 instructions, e.g. %s' % (len(bad), bad[:3])
    assert calls == 0, '%d function calls in the device code: a helper was not inlined (target-feature mismatch?)' % calls


def test_argument_validation_without_gpu(lib):
    assert lib.ttup_refine_windows(None, None, 1, 4, 4, 10, 10, 0, None, None) == _lib.EINVAL
    assert b'null' in lib.ttup_last_error()
    h = ctypes.c_void_p()
    assert lib.ttup_wasb_create(b'x' * 64, 64, 63, 64, 1, 0, ctypes.byref(h)) == _lib.EINVAL     # height not a multiple of 8
    assert lib.ttup_uplift_create(b'NOTMAGIC' + b'\0' * 64, 72, 1, 8, ctypes.byref(h)) == _lib.EFORMAT
    assert lib.ttup_wasb_create_ex(b'x' * 64, 64, 64, 64, 1, 0, 0, 5, ctypes.byref(h)) == _lib.EINVAL     # at most four lanes
    assert b'lanes' in lib.ttup_last_error()
    n = ctypes.c_int(0)
    assert lib.ttup_wasb_streams(None, None, 0, ctypes.byref(n)) == _lib.EINVAL
    assert lib.ttup_max_abs_diff(None, None, 4, None, None) == _lib.EINVAL
    # round-4 entry points: null handles / pointers are refused before anything touches a device
    assert lib.ttup_max_abs_diff_cols(None, None, 2, 8, 0, 8, None, 0, None) == _lib.EINVAL
    assert lib.ttup_slice_columns(None, 2, 8, 0, 4, None, None) == _lib.EINVAL
    for fn in (lib.ttup_wasb_certify_status, lib.ttup_wasb_certify_flags, lib.ttup_wasb_certify_margins):
        assert fn(None, 1, None, None) == _lib.EINVAL
    out3 = (ctypes.c_int * 3)()
    assert lib.ttup_uplift_graph_info(None, out3) == _lib.EINVAL
    assert lib.ttup_uplift_stage_info(None, None) == _lib.EINVAL
    assert lib.ttup_wasb_set_certify(None, 0.1, 0, 0) == _lib.EINVAL
    assert len(lib.ttup_build_id()) == 16 and lib.ttup_version() == 103
    with pytest.raises(ValueError):
        _lib.check(_lib.EINVAL)
    assert lib.ttup_refine_workspace_bytes(4, 704, 1280) >= 4 * 44


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from upliftingtabletennis_amd import refine
    with pytest.raises(RuntimeError):
        refine.extract_position_ball(np.zeros((1, 8, 8), np.float32), 10, 10)
    from upliftingtabletennis_amd.interface import BallDetector
    with pytest.raises(RuntimeError):
        BallDetector('wasb')


def test_hub_surface_keeps_the_reference_signatures(monkeypatch, tmp_path):
    """hubconf.py:11-31, :34-88: entry-point names, defaults, and the RuntimeError of a failed download; the un-vendored
    default detector raises NotImplementedError; a missing checkpoint is an error unless TTUP_SYNTHETIC_WEIGHTS=1."""
    import inspect
    import hubconf
    from upliftingtabletennis_amd import interface
    assert inspect.signature(hubconf.ball_detection).parameters['model_name'].default == 'segformerpp_b2'
    assert inspect.signature(hubconf.table_detection).parameters['model_name'].default == 'segformerpp_b2'
    assert inspect.signature(hubconf.download_example_images).parameters['local_folder'].default == 'example_images'
    assert list(inspect.signature(hubconf.full_pipeline).parameters) == []
    assert list(inspect.signature(interface.TableTennisPipeline.predict).parameters) == ['self', 'images', 'fps']
    with pytest.raises(NotImplementedError):
        hubconf.ball_detection()
    with pytest.raises(NotImplementedError):
        hubconf.table_detection()
    have = tmp_path / 'have'
    have.mkdir()
    (have / 'frame0.png').write_bytes(b'x')
    assert hubconf.download_example_images(str(have)) == str(have)       # already present: returned as is
    monkeypatch.setenv('http_proxy', 'http://127.0.0.1:9'); monkeypatch.setenv('https_proxy', 'http://127.0.0.1:9')
    with pytest.raises(RuntimeError, match='Failed to download images'):
        hubconf.download_example_images(str(tmp_path / 'missing'))
    monkeypatch.delenv('TTUP_WEIGHTS', raising=False)
    monkeypatch.delenv('TTUP_SYNTHETIC_WEIGHTS', raising=False)
    monkeypatch.setattr(interface.torch.hub, 'get_dir', lambda: str(tmp_path))
    for fn, args in ((interface._load_ball_checkpoint, ('wasb',)), (interface._load_table_checkpoint, ('hrnet',)), (interface._load_uplift_checkpoint, ())):
        with pytest.raises(RuntimeError, match='Failed to download weights'):
            fn(*args)
    monkeypatch.setenv('TTUP_SYNTHETIC_WEIGHTS', '1')
    with pytest.warns(RuntimeWarning):
        sd, res, frames = interface._load_ball_checkpoint('wasb')
    assert res == (1280, 704) and frames == 3


def test_bench_refuses_more_ranks_than_gpus():
    """`python bench.py --gpus 2` starts its ranks itself; with fewer visible devices it says so and exits 2 without touching a GPU."""
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip('two GPUs present')
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'TTUP_BENCH_SHARE_GPU')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '1', '--warmup', '0'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and 'only' in r.stderr and not r.stdout.strip()


def test_bench_refuses_zero_steps():
    """`--steps` is the number of timed steps and `ms_per_step` divides by it: fewer than one is refused before anything else runs."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--steps' in r.stderr and not r.stdout.strip()


def test_bench_refuses_ops_json_without_full(tmp_path):
    """`--ops-json` writes the per-op timings behind `roofline`, which only a `--full` run measures: without --full it is refused
    before anything runs, and nothing is written."""
    import subprocess
    import sys
    ops = tmp_path / 'ops.json'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--ops-json', str(ops)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--full' in r.stderr and not r.stdout.strip() and not ops.exists()


def test_blob_layout_roundtrip():
    sd = weights.random_wasb_state_dict(3)
    blob = weights.pack_wasb_blob(sd)
    assert blob[:8] == b'TTUPWSB1'
    n, in_ch, head, _ = np.frombuffer(blob, np.int32, 4, 8)
    assert (n, in_ch, head) == (72, 9, 3)
    off = 24
    for s in arch.hrnet_convs():
        h = np.frombuffer(blob, np.int32, 8, off); off += 32
        assert tuple(h[:6]) == (s.cout, s.cin, s.k, s.stride, 1 if s.bn else 0, 1 if s.has_bias else 0)
        nw = s.cout * s.cin * s.k * s.k
        w = np.frombuffer(blob, np.float32, nw, off); off += 4 * nw
        assert np.array_equal(w, sd[s.conv + '.weight'].ravel())
        off += 4 * s.cout * ((1 if s.has_bias else 0) + (4 if s.bn else 0))
    assert off == len(blob)
    usd = weights.random_uplift_state_dict(4, 'large')
    ub = weights.pack_uplift_blob(usd, 'large')
    assert ub[:8] == b'TTUPUPL1' and tuple(np.frombuffer(ub, np.int32, 6, 8)) == (128, 4, 4, 12, 4, 13)
    with pytest.raises(ValueError):
        bad = dict(sd); bad['model.conv1.weight'] = np.zeros((64, 3, 3, 3), np.float32)
        weights.pack_wasb_blob(bad)


@pytest.mark.parametrize('name', ['short', 'mid', 'long'])
def test_glue_matches_reference_goldens(golden, name):
    g = golden('glue.npz')
    pos, idx, times = glue.filter_trajectory_ball(g[name + '/p1'], g[name + '/p2'], float(g[name + '/fps']))
    np.testing.assert_array_equal(pos, g[name + '/pos'])
    np.testing.assert_array_equal(idx, g[name + '/idx'])
    np.testing.assert_array_equal(times, g[name + '/times'])
    b, tb, tm, mk = glue._uplifting_transform(pos, g[name + '/table'], times)
    np.testing.assert_array_equal(b.numpy(), g[name + '/u_ball'])
    np.testing.assert_array_equal(tb.numpy(), g[name + '/u_table'])
    np.testing.assert_array_equal(tm.numpy(), g[name + '/u_times'])
    np.testing.assert_array_equal(mk.numpy(), g[name + '/u_mask'])


@pytest.fixture(scope='module')
def host_fit(tmp_path_factory):
    so = str(tmp_path_factory.mktemp('hostfit') / 'host_fit.so')
    subprocess.check_call(['g++', '-O2', '-ffp-contract=off', '-shared', '-fPIC', '-Wno-unknown-pragmas', '-o', so,
                           os.path.join(ROOT, 'tests', 'helpers', 'host_fit.cpp')])
    return ctypes.CDLL(so)


_FIT_RADIUS = {}


def _fit_radius(win, variant):
    """How far the REFERENCE's own answer moves when exp() differs in the last bit: SciPy's L-BFGS-B (the reference's optimiser,
    2-point finite differences with a 1e-8 step) on the reference's loss, with every exp() result randomly left alone or moved
    up by one ulp -- what separates numpy's SIMD exp (which produced the goldens), glibc's and the device's.  Largest shift of
    the fitted offset over 5 seeded draws, per window (heatmap pixels).  Ball variant, window 36 (a sigma = 30 blob: a flat
    valley up to the sigma bound of 50): 0.08 px; glibc's exp alone moves it by 0.018 px.  Table variant: < 1e-5 px everywhere."""
    key = (variant, win.tobytes())
    if key in _FIT_RADIUS:
        return _FIT_RADIUS[key]
    from scipy.optimize import minimize
    from oracle import refine_ref as R
    n = win.shape[0]
    smax = 50 if variant == 0 else 3
    bounds = [(0, 3), (0, 3), (0.5, smax), (0.5, smax)]

    def fit(flat, expfn):
        def loss(p):
            x0, y0, sx, sy = p
            if variant == 1:
                sx, sy = max(0.5, sx), max(0.5, sy)
            return np.mean((expfn(-((R._XY[0] - x0) ** 2 / (2 * sx ** 2) + (R._XY[1] - y0) ** 2 / (2 * sy ** 2))) - flat) ** 2)
        return minimize(loss, np.array([1, 1, 1.0, 1.0], dtype=np.float32), method='L-BFGS-B', bounds=bounds).x[:2]
    flats = [np.asarray(win[i], np.float32).flatten() for i in range(n)]
    ref = np.array([fit(f, np.exp) for f in flats])
    rad = np.zeros(n)
    for draw in range(5):
        rng = np.random.default_rng(100 + draw)

        def exp_ulp(a):
            e = np.exp(a)
            return np.where(rng.uniform(size=e.shape) < 0.5, np.nextafter(e, np.inf), e)
        rad = np.maximum(rad, np.abs(np.array([fit(f, exp_ulp) for f in flats]) - ref).max(1))
    _FIT_RADIUS[key] = rad
    return rad


def _check_fit_bars(err, variant, win, device=False):
    """Bars on |offset - SciPy offset| in heatmap pixels over the 51 golden windows (tests/golden/refine.npz), tied to the
    conditioning of each fit instead of one number for all: a window must agree to 1e-6 px or to twice the distance the
    reference's OWN answer moves under one-ulp differences of exp() (`_fit_radius`), whichever is larger.
    Table variant (sigma in [0.5, 3], the hub surface): all radii are below 1e-5, so every window agrees to 2e-5 px at worst
    (measured 4e-7 on host and device).  Ball variant (sigma free up to 50): 44 of 51 windows have radii below 1e-6; the flat
    valleys of the wide blobs amplify last-bit exp() differences through the 1e-8 finite-difference step -- window 36 (sigma = 30)
    has a radius of 0.08 px, and the host build (glibc exp) / the device land 0.030 / 0.088 px from numpy's answer."""
    rad = _fit_radius(win, variant)
    bar = np.maximum(1e-6, 2.0 * rad)
    worst = int(np.argmax(err / bar))
    assert (err <= bar).all(), 'window %d: off by %.3e px, bar %.3e (radius of the reference answer %.3e)' % (worst, err[worst], bar[worst], rad[worst])
    if variant == 1:
        assert err.max() < 2e-5, (err.max(), int(err.argmax()))
    else:
        assert (err < 1e-6).sum() >= err.shape[0] - 8, np.sort(err)[-10:]
    return bar


def test_fit_solver_host_build_tracks_scipy(host_fit, golden):
    """csrc/lbfgsb.h compiled for the host against the scipy-based oracle on the golden windows
    (the same code runs per lane in the HIP fit kernel)."""
    from oracle import refine_ref
    heat = golden('refine.npz')['heat'][:, 0]
    idx, win = refine_ref.argmax_window(heat)
    n = win.shape[0]
    for variant in (0, 1):
        out = np.zeros((n, 8))
        w = np.ascontiguousarray(win.reshape(n, 9), np.float32)
        host_fit.ttup_host_fit(w.ctypes.data_as(ctypes.c_void_p), n, variant, out.ctypes.data_as(ctypes.c_void_p))
        ref = np.array([refine_ref.fit_window(win[i], variant)[:2] for i in range(n)])
        err = np.abs(out[:, :2] - ref).max(1)
        _check_fit_bars(err, variant, win)


def test_filter_trajectory_table_matches_reference(golden):
    g = golden('table.npz')
    out = glue.filter_trajectory_table(g['filter/p1'], g['filter/p2'])
    assert out.shape == (13, 3)
    np.testing.assert_allclose(out, g['filter/out'], rtol=0, atol=1e-9)


# ------------------------------------------------------------------------------------------ f4: camera calibration
def test_calibration_oracle_matches_reference_and_host_glue(golden):
    """The CPU oracle of the calibration (oracle/calib_ref.py: DLT -> 100-subset RANSAC of SciPy BFGS refinements -> refinement on
    the inliers, the reference's own calls in the same order) against the reference's output on the case with an outlier and an
    invisible keypoint (1e-9; bit-equal on the build container).  The product's host glue: `reproject` on all three cameras
    equals the reference arithmetic, and the RANSAC subsets are the reference's draws (numpy PCG64, seed 42)."""
    from oracle import calib_ref
    from upliftingtabletennis_amd import calib
    g = golden('calib.npz')
    kp = g['calib/1/keypoints']
    assert kp[7, 2] == 0
    Mint, Mext = calib_ref.calibrate_camera(kp)
    assert Mint.shape == (3, 4) and Mext.shape == (4, 4)
    assert np.allclose(Mint, g['calib/1/Mint'], rtol=1e-9, atol=1e-9) and np.allclose(Mext, g['calib/1/Mext'], rtol=1e-9, atol=1e-9)
    for ci in range(int(g['n'][0])):
        uv = calib.reproject(g['calib/%d/points' % ci], g['calib/%d/Mint' % ci], g['calib/%d/Mext' % ci])
        assert np.abs(uv - g['calib/%d/reproj' % ci]).max() <= 1e-9
        assert np.array_equal(calib_ref.reproject(g['calib/%d/points' % ci], g['calib/%d/Mint' % ci], g['calib/%d/Mext' % ci]), g['calib/%d/reproj' % ci])
    with pytest.raises(AssertionError):
        calib_ref.calibrate_camera(np.concatenate([kp[:, :2], np.zeros((13, 1))], axis=1))       # fewer than 6 visible points
    vis = [k + 1 for k in range(13) if kp[k, 2] == 1]
    sub = calib.ransac_subsets(vis)
    rnd = np.random.default_rng(seed=42)
    pool = [k for k in vis if k not in (10, 11)]
    assert sub.shape == (100, 4) and np.array_equal(sub[0], rnd.choice(pool, size=4, replace=False)) and set(sub.ravel()) <= set(pool)


# ------------------------------------------------------------------------------------------ a8: checkpoint ingestion
def test_reference_format_checkpoints_are_ingested(tmp_path, monkeypatch):
    """The reference saves {'model_state_dict', 'identifier', 'additional_info'} with torch.save (helper_balldetection.py
    :510-529, uplifting/helper.py:371-391) and lays them out as inference_<task>/<model>/model.pt; the loaders read the
    same layout from TTUP_WEIGHTS, pick resolution / size from additional_info, and the packed blobs are identical to the
    ones packed from the in-memory state_dict.  A missing file under TTUP_WEIGHTS is an error, not a silent fallback."""
    import torch
    from upliftingtabletennis_amd import interface
    ball = weights.random_wasb_state_dict(3)
    table = weights.random_wasb_state_dict(4, in_ch=3, head_out=13)
    up = weights.random_uplift_state_dict(5, 'large')
    layout = {('inference_balldetection', 'wasb'): (ball, {'model_name': 'wasb', 'image_resolution': (1280, 704), 'in_frames': 3, 'lr': 1e-3}),
              ('inference_tabledetection', 'hrnet'): (table, {'model_name': 'hrnet', 'image_resolution': (1280, 704)}),
              ('inference_uplifting', 'ours'): (up, {'name': 'connectstage', 'size': 'large', 'tabletoken_mode': 'dynamic', 'time_rotation': 'new',
                                                      'transform_mode': 'global', 'randdet_prob': 0.0, 'randmiss_prob': 0.0, 'tablemiss_prob': 0.0})}
    for (task, name), (sd, info) in layout.items():
        d = tmp_path / task / name
        d.mkdir(parents=True)
        torch.save({'model_state_dict': {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, 'identifier': 'unit-test', 'additional_info': info}, str(d / 'model.pt'))
    monkeypatch.setenv('TTUP_WEIGHTS', str(tmp_path))
    sd, res, frames = interface._load_ball_checkpoint('wasb')
    assert res == (1280, 704) and frames == 3
    assert weights.pack_wasb_blob(sd) == weights.pack_wasb_blob(ball)
    sd, res = interface._load_table_checkpoint('hrnet')
    assert res == (1280, 704) and weights.pack_wasb_blob(sd, in_ch=3, head_out=13) == weights.pack_wasb_blob(table, in_ch=3, head_out=13)
    sd, size, mode = interface._load_uplift_checkpoint()
    assert (size, mode) == ('large', 'global') and weights.pack_uplift_blob(sd, 'large') == weights.pack_uplift_blob(up, 'large')
    (tmp_path / 'inference_balldetection' / 'wasb' / 'model.pt').unlink()
    with pytest.raises(RuntimeError):
        interface._load_ball_checkpoint('wasb')
    # a checkpoint trained with the other RoPE time convention must not run silently on the 'new' path
    d = tmp_path / 'inference_uplifting' / 'ours' / 'model.pt'
    info = dict(layout[('inference_uplifting', 'ours')][1], time_rotation='old')
    torch.save({'model_state_dict': {k: torch.from_numpy(np.asarray(v)) for k, v in up.items()}, 'identifier': 'unit-test', 'additional_info': info}, str(d))
    with pytest.raises(ValueError, match='time_rotation'):
        interface._load_uplift_checkpoint()


def test_native_dbscan_labels_equal_sklearns():
    """glue._dbscan_labels replaces the scikit-learn DBSCAN call of the reference's keypoint filter (inference/utils.py:213) on the
    product side: same labels -- cluster numbering, border-point assignment, noise -- on random point sets with one to four
    clusters, including integer coordinates that put distances exactly on the threshold; and the filter built on it equals the
    oracle's (which keeps sklearn) on two disagreeing detectors."""
    from sklearn.cluster import DBSCAN
    from oracle import glue_ref
    rng = np.random.default_rng(3)
    for trial in range(400):
        n, k = int(rng.integers(3, 70)), int(rng.integers(1, 5))
        centers = rng.uniform(0, 120, (k, 2))
        pts = centers[rng.integers(k, size=n)] + rng.normal(0, rng.uniform(1, 12), (n, 2))
        if trial % 4 == 0:
            pts = np.round(pts)
        for eps, ms in ((10, 3), (10, 5), (6, 4)):
            assert np.array_equal(glue._dbscan_labels(pts, eps, ms), DBSCAN(eps=eps, min_samples=ms).fit(pts).labels_), (trial, eps, ms)
    for trial in range(20):
        T = 40
        p1 = np.zeros((T, 13, 3)); p1[:, :, :2] = rng.uniform(0, 1900, (13, 2)) + rng.normal(0, rng.uniform(0.5, 8), (T, 13, 2)); p1[:, :, 2] = rng.uniform(size=(T, 13)) < 0.9
        p2 = p1.copy(); p2[:, :, :2] += rng.normal(0, 5, (T, 13, 2)); p2[:, :, 2] = rng.uniform(size=(T, 13)) < 0.9
        if trial % 3 == 0:
            p1, p2 = np.round(p1), np.round(p2)
        assert np.array_equal(glue.filter_trajectory_table(p1, p2), glue_ref.filter_trajectory_table(p1, p2))
