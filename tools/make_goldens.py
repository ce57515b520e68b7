#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE's own Python (from /root/reference).

Runs only in the build container (the reference never travels to the GPU box).  Only tensors,
seeds and shapes are written -- never reference source.  Inputs are regenerated in the tests
from the same seeds through ``upliftingtabletennis_amd.synth`` / ``weights`` (numpy PCG64).

Stubs needed to import the reference here: ``torch.utils.tensorboard`` (absent),
``cv2`` (absent; only imported, never called on the paths used), ``torch.load`` patched while
``WASBNet.__init__`` reads its initialisation checkpoint (wasb.py:580-582).

    python tools/make_goldens.py            # writes tests/golden/
"""
import hashlib
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TTUP_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)


def install_stubs():
    import torch.utils
    tb = types.ModuleType('torch.utils.tensorboard')

    class SummaryWriter(object):
        def __init__(self, *a, **k):
            pass
    tb.SummaryWriter = SummaryWriter
    tbs = types.ModuleType('torch.utils.tensorboard.summary')
    tbs.hparams = lambda *a, **k: None
    tb.summary = tbs
    torch.utils.tensorboard = tb
    sys.modules['torch.utils.tensorboard'] = tb
    sys.modules['torch.utils.tensorboard.summary'] = tbs
    if 'cv2' not in sys.modules:
        try:
            import cv2  # noqa: F401
        except Exception:
            sys.modules['cv2'] = types.ModuleType('cv2')


def ref_wasb(sd_np):
    from balldetection.models.wasb import WASBNet
    orig = torch.load
    torch.load = lambda *a, **k: {}
    try:
        m = WASBNet(in_frames=3, resolution=(1280, 704))
    finally:
        torch.load = orig
    ref_sd = {k: v for k, v in m.state_dict().items() if 'num_batches_tracked' not in k}
    schema = [(k, list(v.shape)) for k, v in ref_sd.items()]
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=False)
    assert not unexpected and all('num_batches_tracked' in k for k in missing), (missing, unexpected)
    m.eval()
    return m, schema


def taps_summary(taps):
    """Per-tap [mean, mean|x|, x[0,0,1,2], x[-1,-1,-2,-3]] -- cheap localisation of a divergence."""
    return {k: np.array([v.mean().item(), v.abs().mean().item(), v[0, 0, 1, 2].item(), v[-1, -1, -2, -3].item()], np.float64)
            for k, v in taps.items()}


def gen_wasb():
    from upliftingtabletennis_amd import weights, synth, arch
    from oracle import wasb_ref, glue_ref
    out = {}
    cases = [('noise_64x96', 11, False, (1, 64, 96)), ('noise_96x160', 13, False, (2, 96, 160)), ('planted_96x160', 12, True, (2, 96, 160))]
    schema = None
    for name, seed, planted, (b, h, w) in cases:
        sd = weights.random_wasb_state_dict(seed, planted=planted)
        model, schema = ref_wasb(sd)
        if planted:
            frames, track = synth.synth_frames(b + 2, h, w, seed=seed)
            x = np.stack([glue_ref.triple_to_tensor(frames[i], frames[i + 1], frames[i + 2], (w, h)) for i in range(b)])
            out[name + '/track'] = track
        else:
            x = np.random.default_rng(seed).standard_normal((b, 9, h, w)).astype(np.float32)
        with torch.no_grad():
            heat, _ = model(torch.from_numpy(x))
            # hook-free taps: re-run the reference sub-modules in forward order
            hr = model.model
            t = {}
            y = hr.relu(hr.bn1(hr.conv1(torch.from_numpy(x)))); t['stem1'] = y
            y = hr.relu(hr.bn2(hr.conv2(y))); t['stem2'] = y
            y = hr.layer1(y); t['layer1'] = y
            xs = [hr.transition1[0](y), hr.transition1[1](y)]; t['trans1_0'], t['trans1_1'] = xs
            ys = hr.stage2(xs); t['stage2_0'], t['stage2_1'] = ys
            xs = [ys[0], ys[1], hr.transition2[2](ys[-1])]
            ys = hr.stage3(xs); t['stage3_0'], t['stage3_1'], t['stage3_2'] = ys
            xs = [ys[0], ys[1], ys[2], hr.transition3[3](ys[-1])]
            ys = hr.stage4(xs)
            for i, v in enumerate(ys):
                t['stage4_%d' % i] = v
        heat = heat.numpy()
        out[name + '/heat'] = heat
        out[name + '/argmax'] = heat.reshape(b, -1).argmax(1).astype(np.int64)
        for k, v in taps_summary(t).items():
            out['%s/tap/%s' % (name, k)] = v
        out[name + '/meta'] = np.array([seed, int(planted), b, h, w], np.int64)
        # sanity: our oracle restatement agrees right here
        o = wasb_ref.wasb_forward(x, sd).numpy()
        print('wasb %-16s max|ref-oracle| = %.3e  heat range [%.3f, %.3f]' % (name, np.abs(o - heat).max(), heat.min(), heat.max()))
    np.savez_compressed(os.path.join(OUT, 'wasb_small.npz'), **out)
    with open(os.path.join(OUT, 'wasb_schema.json'), 'w') as f:
        json.dump(schema, f)
    assert [(k, tuple(s)) for k, s in schema] == [(k, tuple(s)) for k, s in arch.wasb_schema()], 'schema mismatch'


def refine_cases():
    """Heatmaps (N,1,H,W) covering interior / border / corner peaks, ties, flat, negative, saturated."""
    rng = np.random.default_rng(5)
    hs = []
    H, W = 12, 14

    def blob(cx, cy, sx, sy, amp=1.0, base=0.0, noise=0.0):
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
        h = base + amp * np.exp(-((xx - cx) ** 2 / (2 * sx ** 2) + (yy - cy) ** 2 / (2 * sy ** 2)))
        return (h + noise * rng.standard_normal((H, W))).astype(np.float32)
    for _ in range(24):   # interior, various widths and amplitudes
        hs.append(blob(rng.uniform(2, W - 3), rng.uniform(2, H - 3), rng.uniform(0.4, 3.0), rng.uniform(0.4, 3.0),
                       amp=rng.uniform(0.3, 1.5), noise=0.01))
    for cx, cy in [(0.2, 5.3), (W - 1.1, 4.6), (6.4, 0.1), (7.7, H - 1.2), (0.3, 0.2), (W - 1.2, H - 1.3), (0.0, H - 1.0), (W - 1.0, 0.0)]:
        hs.append(blob(cx, cy, 1.2, 0.9))                      # border / corner peaks (zero padding in the window)
    hs.append(np.zeros((H, W), np.float32))                    # flat zero -> index 0
    hs.append(np.full((H, W), 0.7, np.float32))                # flat non-zero
    hs.append(blob(5.5, 5.5, 1.0, 1.0))                        # 4-way tie candidate
    hs.append(blob(4.0, 6.0, 0.3, 0.3))                        # narrower than the lower sigma bound
    hs.append(blob(4.0, 6.0, 30.0, 30.0))                      # very wide -> sigma upper bound (table variant)
    hs.append(blob(8.0, 3.0, 1.0, 1.0, amp=6.0))               # saturated (> 1)
    hs.append(blob(8.0, 3.0, 1.0, 1.0, amp=1.0, base=-3.0))    # everything negative
    hs.append(blob(3.3, 7.6, 2.0, 0.6, amp=0.05))              # weak peak below the table threshold
    t = np.zeros((H, W), np.float32); t[4, 5] = 1.0; t[9, 2] = 1.0
    hs.append(t)                                               # exact tie -> first index
    for _ in range(8):
        hs.append(rng.standard_normal((H, W)).astype(np.float32))   # noise-like (random-weights regime)
    # the reference's own toy case (helper_balldetection.py:535-541): 5x5 maps are padded into HxW here
    a = np.zeros((H, W), np.float32); a[2, 2] = 1.0; a[2, 3] = 1.0
    b = np.zeros((H, W), np.float32); b[1, 4] = 1.0
    hs += [a, b]
    return np.stack(hs)[:, None]


def gen_refine():
    from balldetection.helper_balldetection import extract_position_torch_gaussian as ball_fn
    from tabledetection.helper_tabledetection import extract_position_torch_gaussian as table_fn
    heat = refine_cases()
    t = torch.from_numpy(heat)
    ball = ball_fn(t, 1920, 1080)
    table = table_fn(t, 1920, 1080)
    # multi-channel table call (B=2, C=3)
    mc = heat[:6, 0].reshape(2, 3, *heat.shape[2:])
    table_mc = table_fn(torch.from_numpy(mc), 1920, 1080)
    toy = torch.tensor([[[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 1, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]],
                        [[0, 0, 0, 0, 0], [0, 0, 0, 0, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]], dtype=torch.float32)
    toy_ball = ball_fn(toy, 5, 5)
    np.savez_compressed(os.path.join(OUT, 'refine.npz'), heat=heat, ball=ball, table=table, mc=mc, table_mc=table_mc,
                        toy=toy.numpy(), toy_ball=toy_ball)
    print('refine: %d cases, ball out %s table out %s' % (heat.shape[0], ball.shape, table.shape))


def gen_uplift():
    from uplifting.model import get_model
    from uplifting.helper import transform_rotationaxes
    from upliftingtabletennis_amd import weights, synth, arch
    from oracle import uplift_ref
    out = {}
    schema = None
    for name, size, seed, b, t, pad in [('large_T8', 'large', 21, 4, 8, 3), ('large_T50', 'large', 22, 4, 43, 7),
                                        ('large_T121', 'large', 23, 3, 120, 1), ('small_T20', 'small', 24, 2, 17, 3)]:
        sd = weights.random_uplift_state_dict(seed, size)
        m = get_model('connectstage', size, 'dynamic', 'new')
        ref_sd = m.state_dict()
        if size == 'large':
            schema = [(k, list(v.shape)) for k, v in ref_sd.items()]
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        m.eval()
        ball, table, mask, times = synth.synth_trajectories(b, t, seed=seed, pad=pad)
        if b > 1:  # ragged: second trajectory shorter; irregular timestamps (dropped frames) on the first
            cut = max(3, t // 2)
            ball[1, cut:] = 0; mask[1, cut:] = 0; times[1, cut:] = 0
            keep = np.sort(np.random.default_rng(seed).choice(t + 6, t, replace=False))
            times[0, :t] = (keep / 60.0).astype(np.float32)
            table[0, 3, 2] = 0; table[0, 9, 2] = 0
        with torch.no_grad():
            rot, pos = m(*[torch.from_numpy(a) for a in (ball, table, mask, times)])
            rot_local = transform_rotationaxes(rot, pos.clone())
        out[name + '/rot'] = rot.numpy(); out[name + '/pos'] = pos.numpy(); out[name + '/rot_local'] = rot_local.numpy()
        out[name + '/ball'] = ball; out[name + '/table'] = table; out[name + '/mask'] = mask; out[name + '/times'] = times
        out[name + '/meta'] = np.array([seed, b, t, pad], np.int64)
        out[name + '/size'] = np.array(size)
        o_rot, o_pos = uplift_ref.uplift_forward(ball, table, mask, times, sd, heads=arch.UPLIFT_SIZES[size][2])
        print('uplift %-12s max|ref-oracle| rot %.3e pos %.3e' % (name, (o_rot - rot).abs().max(), (o_pos - pos).abs().max()))
    # error behaviour: all-ones mask raises (model.py:541-546)
    try:
        m(torch.zeros(1, 4, 2), torch.zeros(1, 13, 3), torch.ones(1, 4), torch.zeros(1, 4))
        raised = False
    except ValueError:
        raised = True
    out['allones_mask_raises'] = np.array(raised)
    np.savez_compressed(os.path.join(OUT, 'uplift.npz'), **out)
    with open(os.path.join(OUT, 'uplift_schema.json'), 'w') as f:
        json.dump(schema, f)
    assert [(k, tuple(s)) for k, s in schema] == [(k, tuple(s)) for k, s in arch.uplift_schema('large')], 'uplift schema mismatch'


def gen_glue():
    out = {}
    try:
        from inference.utils import filter_trajectory_ball, _uplifting_transform
        src = 'reference'
    except Exception as e:  # pragma: no cover
        print('inference.utils not importable (%s); glue goldens skipped' % e)
        return
    rng = np.random.default_rng(31)
    for name, T in [('short', 12), ('mid', 37), ('long', 70)]:
        p1 = np.concatenate([rng.uniform(0, 1920, (T, 1)), rng.uniform(0, 1080, (T, 1)), np.ones((T, 1))], 1)
        p2 = p1.copy()
        p2[:, :2] += rng.normal(0, 9.0, (T, 2))
        p2[3, 2] = 0
        p1[5, 2] = 0
        fps = {'short': 60.0, 'mid': 50, 'long': 120.0}[name]
        pos, idx, times = filter_trajectory_ball(p1, p2, fps)
        table = np.concatenate([rng.uniform(0, 1920, (13, 1)), rng.uniform(0, 1080, (13, 1)), (rng.uniform(size=(13, 1)) < 0.8).astype(float)], 1)
        b, tb, tm, mk = _uplifting_transform(pos, table, times)
        out.update({name + '/p1': p1, name + '/p2': p2, name + '/fps': np.array(fps), name + '/pos': pos, name + '/idx': idx,
                    name + '/times': times, name + '/table': table, name + '/u_ball': b.numpy(), name + '/u_table': tb.numpy(),
                    name + '/u_times': tm.numpy(), name + '/u_mask': mk.numpy()})
    from balldetection.transforms import NormalizeImage
    img = rng.integers(0, 256, (6, 8, 3), dtype=np.uint8)
    d = NormalizeImage(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])({'image': img.copy(), 'prev_image': img[::-1].copy(), 'next_image': None})
    out['norm/img'] = img
    out['norm/out'] = d['image']
    out['norm/out_prev'] = d['prev_image']
    np.savez_compressed(os.path.join(OUT, 'glue.npz'), **out)
    print('glue: filter/transform/normalise goldens from', src)


def gen_table():
    """f1: table-keypoint HRNet (tabledetection/models/hrnet.py) on seeded weights + the DBSCAN keypoint filter."""
    from tabledetection.models.hrnet import MyHRNet
    from inference.utils import filter_trajectory_table
    from upliftingtabletennis_amd import weights, arch
    from oracle import wasb_ref
    out = {}
    orig = torch.load
    torch.load = lambda *a, **k: {}
    try:
        m = MyHRNet(resolution=(1280, 704))
    finally:
        torch.load = orig
    ref_sd = {k: v for k, v in m.state_dict().items() if 'num_batches_tracked' not in k}
    schema = [(k, list(v.shape)) for k, v in ref_sd.items()]
    assert [(k, tuple(s)) for k, s in schema] == [(k, tuple(s)) for k, s in arch.wasb_schema(in_ch=3, head_out=13)], 'table schema mismatch'
    for name, seed, (b, h, w) in [('noise_64x96', 51, (2, 64, 96)), ('noise_96x160', 52, (1, 96, 160))]:
        sd = weights.random_wasb_state_dict(seed, in_ch=3, head_out=13)
        missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
        assert not unexpected and all('num_batches_tracked' in k for k in missing)
        m.eval()
        x = np.random.default_rng(seed).standard_normal((b, 3, h, w)).astype(np.float32)
        with torch.no_grad():
            heat = m(torch.from_numpy(x)).numpy()
        out[name + '/heat'] = heat
        out[name + '/meta'] = np.array([seed, b, h, w], np.int64)
        o = wasb_ref.hrnet_forward(torch.from_numpy(x), sd)[0]
        print('table %-14s heat %s max|ref-oracle| = %.3e' % (name, heat.shape, float((o - torch.from_numpy(heat)).abs().max())))
    # DBSCAN filter: 13 keypoints over 40 frames, two detectors, outliers / invisibles / too-few-detections cases
    rng = np.random.default_rng(53)
    T = 40
    true = np.stack([rng.uniform(100, 1800, 13), rng.uniform(100, 1000, 13)], 1)
    p1 = np.zeros((T, 13, 3)); p2 = np.zeros((T, 13, 3))
    for t in range(T):
        p1[t, :, :2] = true + rng.normal(0, 1.5, (13, 2)); p1[t, :, 2] = 1
        p2[t, :, :2] = true + rng.normal(0, 1.5, (13, 2)); p2[t, :, 2] = 1
    p1[::5, 3, :2] += 300            # outliers for keypoint 3
    p2[:, 7, 2] = 0                  # keypoint 7 invisible in the second detector
    p1[2:, 9, 2] = 0                 # keypoint 9: only two usable detections
    p2[:, 11, :2] += 50              # detectors disagree on keypoint 11
    p1[20:, 5, :2] += 60; p2[20:, 5, :2] += 60       # two clusters for keypoint 5
    out['filter/p1'] = p1; out['filter/p2'] = p2
    out['filter/out'] = filter_trajectory_table(p1, p2)
    np.savez_compressed(os.path.join(OUT, 'table.npz'), **out)
    print('table filter ->', out['filter/out'][[3, 5, 7, 9, 11]].tolist())


def gen_fullsize():
    """One 704x1280 planted-peak run through the reference CNN + both refine variants."""
    from upliftingtabletennis_amd import weights, synth
    from oracle import glue_ref
    from balldetection.helper_balldetection import extract_position_torch_gaussian as ball_fn
    from tabledetection.helper_tabledetection import extract_position_torch_gaussian as table_fn
    seed, h, w, b = 41, 704, 1280, 2
    sd = weights.random_wasb_state_dict(seed, planted=True)
    model, _ = ref_wasb(sd)
    frames, track = synth.synth_frames(b + 2, h, w, seed=seed)
    x = np.stack([glue_ref.triple_to_tensor(frames[i], frames[i + 1], frames[i + 2], (w, h)) for i in range(b)])
    t0 = time.time()
    with torch.no_grad():
        heat, _ = model(torch.from_numpy(x))
    dt = time.time() - t0
    ball = ball_fn(heat, 1920, 1080)
    table = table_fn(heat, 1920, 1080)
    hn = heat.numpy()
    idx = hn.reshape(b, -1).argmax(1).astype(np.int64)
    flat = np.sort(hn.reshape(b, -1), axis=1)
    crops = np.stack([hn[i, 0, max(0, idx[i] // w - 8):idx[i] // w + 8, max(0, idx[i] % w - 8):idx[i] % w + 8] for i in range(b)])
    np.savez_compressed(os.path.join(OUT, 'wasb_full.npz'), meta=np.array([seed, b, h, w], np.int64), track=track, argmax=idx,
                        ball=ball, table=table, top2=flat[:, -2:], crops=crops, sub16=hn[:, :, ::16, ::16],
                        sha256=np.array(hashlib.sha256(hn.tobytes()).hexdigest()), ref_seconds=np.array(dt))
    print('full-size: ref forward %.1f s for %d frames (%d threads); argmax %s (track %s); top2 %s'
          % (dt, b, torch.get_num_threads(), [(int(i % w), int(i // w)) for i in idx], track[1:1 + b].tolist(), flat[:, -2:].tolist()))


HARD_SETS = [          # (weight seed, weight noise scale, [(clip seed, blob sigma, brightness gain), ...])
    (0, 0.2, [(2000, 3.0, 1.3), (2001, 3.5, 1.5), (2002, 4.0, 1.6), (2003, 4.0, 1.3),      # bench.py's weights on the soak's hard content
               # three clips picked (from seeds 2020-2059, reference run on 168x168 crops around the blob) for holding the SMALLEST reference
               # top-2 margins: 2e-5, 1.4e-4, 1.8e-4 -- frames on which two fp32 evaluations need not agree
               (2050, 3.8, 1.6), (2046, 3.4, 1.3), (2024, 3.7, 1.4)]),
    (21, 1.0, [(2010, 3.5, 1.5), (2011, 4.0, 1.3)]),                                           # noisy planted weights: near-ties across the frame
]
HARD_FRAMES = 6           # per clip -> 4 triples


def gen_hard():
    """reference `WASBNet` (balldetection/models/wasb.py:596-608) at 704x1280 on NEAR-TIE content -- wide saturated
    blobs (flat-topped heatmaps) on bench.py's planted weights, plus noisy planted weights (seed 21, noise 1) -- batch 1 per triple
    like interface.py:102-119.  Per triple: the reference's argmax, its 16 largest values with their indices (the tied set under
    any tolerance), the zero-padded 3x3 window (tabledetection/helper_tabledetection.py:63-77), a 32x32 crop around the argmax and
    a 16x16 sub-sampling of the heatmap (what the test measures its HIP-fp32-vs-reference bound on).  Frames are generated AT the
    network resolution (the unpinned cv2.resize is then the identity) by `synth.hard_clip`; their sha256 travels with the fixture."""
    from upliftingtabletennis_amd import weights, synth
    from oracle import glue_ref
    h, w = 704, 1280
    out, t0, n_tr = {}, time.time(), 0
    margins = []
    for si, (wseed, weps, clips) in enumerate(HARD_SETS):
        sd = weights.random_wasb_state_dict(wseed, planted=True, eps=weps)
        model, _ = ref_wasb(sd)
        for ci, (cseed, sigma, gain) in enumerate(clips):
            frames, track = synth.hard_clip(HARD_FRAMES, h, w, seed=cseed, sigma=sigma, gain=gain)
            key = 'set%d/clip%d' % (si, ci)
            nt = HARD_FRAMES - 2
            rec = dict(argmax=np.zeros(nt, np.int64), top_idx=np.zeros((nt, 16), np.int64), top_val=np.zeros((nt, 16), np.float32),
                       win=np.zeros((nt, 9), np.float32), crop32=np.zeros((nt, 32, 32), np.float32), crop32_origin=np.zeros((nt, 2), np.int64),
                       sub16=np.zeros((nt, h // 16, w // 16), np.float32))
            for t in range(nt):
                x = glue_ref.triple_to_tensor(frames[t], frames[t + 1], frames[t + 2], (w, h))[None]
                with torch.no_grad():
                    heat, _ = model(torch.from_numpy(x))
                hm = heat.numpy()[0, 0]
                flat = hm.reshape(-1)
                idx = int(flat.argmax())                                       # first maximum, like torch.argmax
                assert idx == int(torch.argmax(heat.reshape(-1)))
                order = np.argsort(-flat, kind='stable')[:16]
                rec['argmax'][t] = idx
                rec['top_idx'][t], rec['top_val'][t] = order, flat[order]
                pad = np.pad(hm, 1)
                y, xq = idx // w, idx % w
                rec['win'][t] = pad[y:y + 3, xq:xq + 3].reshape(-1)
                y0, x0 = int(np.clip(y - 16, 0, h - 32)), int(np.clip(xq - 16, 0, w - 32))
                rec['crop32'][t], rec['crop32_origin'][t] = hm[y0:y0 + 32, x0:x0 + 32], (y0, x0)
                rec['sub16'][t] = hm[::16, ::16]
                margins.append(float(flat[order[0]] - flat[order[1]]))
                n_tr += 1
                print('hard %s t%d: argmax (%d,%d) blob (%.1f,%.1f) max %.4f margin %.5f  [%.0f s]'
                      % (key, t, xq, y, track[t + 1][0], track[t + 1][1], flat[idx], margins[-1], time.time() - t0), flush=True)
            for k, v in rec.items():
                out['%s/%s' % (key, k)] = v
            out[key + '/meta'] = np.array([wseed, cseed, HARD_FRAMES, h, w], np.int64)
            out[key + '/params'] = np.array([weps, sigma, gain], np.float64)
            out[key + '/frames_sha256'] = np.array(hashlib.sha256(frames.tobytes()).hexdigest())
    out['n_sets'] = np.array([len(HARD_SETS)])
    out['n_clips'] = np.array([len(c) for _, _, c in HARD_SETS])
    out['ref_seconds_per_triple'] = np.array((time.time() - t0) / n_tr)
    np.savez_compressed(os.path.join(OUT, 'wasb_hard.npz'), **out)
    m = np.array(margins)
    print('hard: %d triples, %.1f s each; reference top-2 margins: min %.2e median %.2e max %.2e; %d below 0.09, %d below 1e-3'
          % (n_tr, (time.time() - t0) / n_tr, m.min(), np.median(m), m.max(), (m < 0.09).sum(), (m < 1e-3).sum()))


HARD_TABLE = (81, 0.2, [(2100, 3.5, 1.5), (2101, 4.0, 1.3)])          # table weights seed / noise, clips (seed, sigma, gain); 4 frames each


def gen_hard_table():
    """The near-tie fixture for the TABLE detector (13 keypoint heatmaps per frame): the reference `MyHRNet`
    (tabledetection/models/hrnet.py:510-589) at 704x1280, batch 1 per frame like interface.py:160-165, on the hard content of
    gen_hard with seeded weights that carry a planted path to every head (flat-topped maps on all 13 channels).  Per (frame, channel):
    argmax, the 8 largest values with their indices, the zero-padded 3x3 window and a 16x16 crop around the argmax."""
    from upliftingtabletennis_amd import weights, synth
    from oracle import glue_ref
    h, w = 704, 1280
    wseed, weps, clips = HARD_TABLE
    sd = weights.random_wasb_state_dict(wseed, planted=True, in_ch=3, head_out=13, eps=weps, plant_all_heads=True)
    model = ref_table_hrnet(sd, (w, h))
    out, t0, margins = {}, time.time(), []
    nf = 4
    for ci, (cseed, sigma, gain) in enumerate(clips):
        frames, _ = synth.hard_clip(nf, h, w, seed=cseed, sigma=sigma, gain=gain)
        key = 'clip%d' % ci
        rec = dict(argmax=np.zeros((nf, 13), np.int64), top_idx=np.zeros((nf, 13, 8), np.int64), top_val=np.zeros((nf, 13, 8), np.float32),
                   win=np.zeros((nf, 13, 9), np.float32), crop16=np.zeros((nf, 13, 16, 16), np.float32), crop16_origin=np.zeros((nf, 13, 2), np.int64))
        for t in range(nf):
            # frames are generated AT the network resolution (the resize is the identity); normalisation as interface.py:160-165
            # (oracle/glue_ref.normalize_image is pinned equal to the reference's NormalizeImage by glue.npz)
            x = glue_ref.normalize_image(frames[t]).transpose(2, 0, 1).astype(np.float32)[None]
            with torch.no_grad():
                heat = model(torch.from_numpy(np.ascontiguousarray(x)))
            hm = heat.numpy()[0]
            for c in range(13):
                flat = hm[c].reshape(-1)
                order = np.argsort(-flat, kind='stable')[:8]
                idx = int(order[0])
                assert idx == int(torch.argmax(heat[0, c].reshape(-1)))
                rec['argmax'][t, c] = idx
                rec['top_idx'][t, c], rec['top_val'][t, c] = order, flat[order]
                y, xq = idx // w, idx % w
                rec['win'][t, c] = np.pad(hm[c], 1)[y:y + 3, xq:xq + 3].reshape(-1)
                y0, x0 = int(np.clip(y - 8, 0, h - 16)), int(np.clip(xq - 8, 0, w - 16))
                rec['crop16'][t, c], rec['crop16_origin'][t, c] = hm[c, y0:y0 + 16, x0:x0 + 16], (y0, x0)
                margins.append(float(flat[order[0]] - flat[order[1]]))
            print('hard table %s t%d: margins %s  [%.0f s]' % (key, t, ' '.join('%.1e' % m for m in margins[-13:]), time.time() - t0), flush=True)
        for k, v in rec.items():
            out['%s/%s' % (key, k)] = v
        out[key + '/meta'] = np.array([wseed, cseed, nf, h, w], np.int64)
        out[key + '/params'] = np.array([weps, sigma, gain], np.float64)
        out[key + '/frames_sha256'] = np.array(hashlib.sha256(frames.tobytes()).hexdigest())
    out['n_clips'] = np.array([len(clips)])
    np.savez_compressed(os.path.join(OUT, 'table_hard.npz'), **out)
    m = np.array(margins)
    print('hard table: %d heatmaps; reference top-2 margins: min %.2e median %.2e max %.2e; %d below 0.09' % (m.size, m.min(), np.median(m), m.max(), (m < 0.09).sum()))


def install_mujoco_standin(history):
    """`mujoco` is not importable here.  The reference's generator only needs containers (MjModel/MjData), the
    fixed camera pose and `mj_step`.  This stand-in provides the containers and REPLAYS states that oracle/trajgen_ref.py
    integrated beforehand (keyed by the initial state the reference itself drew), so that the reference's own sampling
    loop, bounds checks, hit counting and selection run unchanged on top of the oracle's physics.  It pins the
    reference's control flow, NOT MuJoCo's arithmetic (parity of the physics stays unpinned)."""
    from oracle import trajgen_ref as T
    mj = types.ModuleType('mujoco')
    x = T.CAMERA_RIGHT / np.linalg.norm(T.CAMERA_RIGHT)
    y = T.CAMERA_UP - x * np.dot(x, T.CAMERA_UP)
    y = y / np.linalg.norm(y)
    z = np.cross(x, y)

    class Model(object):
        cam_intrinsic = np.array([[T.FX / T.WIDTH, T.FY / T.HEIGHT, 0.0, 0.0]])
        cam_sensorsize = np.array([[1.0, 1.0]])
        cam_resolution = np.array([[T.WIDTH, T.HEIGHT]])

    class MjModel(object):
        @staticmethod
        def from_xml_string(xml):
            return Model()

    class MjData(object):
        def __init__(self, model):
            self.model = model
            self.qpos = np.zeros(7); self.qpos[3] = 1.0
            self.qvel = np.zeros(6)
            self.time = 0.0
            self.cam_xmat = np.stack([x, y, z], axis=1).reshape(1, 9)
            self.cam_xpos = T.CAMERA_POS[None].copy()
            self._row, self._step = None, 0

    def mj_step(model, data, nstep=1):
        if data._row is None:
            data._row = history[(data.qpos[:3].tobytes(), data.qvel.tobytes())]
        for _ in range(nstep):
            data._step += 1
            data.time += T.TIMESTEP
        st = data._row[data._step]
        data.qpos[:3] = st[0:3]; data.qvel[:3] = st[3:6]; data.qvel[3:6] = st[6:9]

    class mjtObj(object):
        mjOBJ_CAMERA = 7
    mj.MjModel, mj.MjData, mj.mj_step, mj.mjtObj = MjModel, MjData, mj_step, mjtObj
    mj.mj_name2id = lambda model, objtype, name: 0
    sys.modules['mujoco'] = mj
    sys.modules['mujoco_viewer'] = types.ModuleType('mujoco_viewer')
    if 'tqdm' not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except Exception:
            sys.modules['tqdm'] = types.ModuleType('tqdm')


def gen_trajgen():
    """f2: the reference's `_init_simulation`, `_count_hits` and `find_valid_trajectories_worker`, the latter two driven by the
    oracle integrator through the stand-in above."""
    from oracle import trajgen_ref as T
    history = {}
    install_mujoco_standin(history)
    import syntheticdataset.mujocosimulation as ms
    import syntheticdataset.helper as mh
    out = {}
    n_init, n_sel = 48, 160
    # ---- initial states: straight from the reference's sampler (the stand-in only holds the arrays)
    for mode in T.MODES:
        for direction in T.DIRECTIONS:
            st = []
            for seed in list(range(n_init)) + [12345, 2 ** 31 + 7, 2 ** 40 + 3]:
                _, data = ms._init_simulation(seed, mode, direction)
                st.append(np.concatenate([data.qpos[:3], data.qvel[:6]]))
            out['init/%s/%s' % (mode, direction)] = np.stack(st)
    out['init_seeds'] = np.array(list(range(n_init)) + [12345, 2 ** 31 + 7, 2 ** 40 + 3], dtype=np.int64)
    # ---- camera matrices as `_calc_cammatrices` builds them from the (stand-in) camera pose
    _, data = ms._init_simulation(0, 'intermediate', 'left_to_right')
    ex, inm = mh._calc_cammatrices(data, camera_name=mh.CAMERA_NAME)
    out['Mext'], out['Mint'] = ex, inm[:3, :3]
    # ---- worker: integrate every seed for the full second with the oracle, then let the reference select
    t0 = time.time()
    hit_cases = []
    for mode in T.MODES:
        for direction in T.DIRECTIONS:
            seeds = list(range(n_sel))
            st = [T.init_state(s, mode, direction) for s in seeds]
            r = np.stack([a[0] for a in st]); v = np.stack([a[1] for a in st]); w = np.stack([a[2] for a in st])
            hist = np.zeros((len(seeds), 1001, 9))
            hist[:, 0] = np.concatenate([r, v, w], axis=1)
            for k in range(1, 1001):
                r, v, w = T.step_ms(r, v, w, 1)
                hist[:, k] = np.concatenate([r, v, w], axis=1)
            for i in range(len(seeds)):
                history[(hist[i, 0, :3].tobytes(), hist[i, 0, 3:9].tobytes())] = hist[i]
            res = ms.find_valid_trajectories_worker((seeds, mode, direction))
            key = 'worker/%s/%s' % (mode, direction)
            out[key + '/seeds'] = np.array([t['seed'] for t in res], dtype=np.int64)
            out[key + '/n'] = np.array([len(t['positions']) for t in res], dtype=np.int64)
            out[key + '/bounces'] = np.concatenate([t['bounces'] for t in res]) if res else np.zeros(0)
            out[key + '/n_bounces'] = np.array([len(t['bounces']) for t in res], dtype=np.int64)
            if res:
                out[key + '/first_positions'] = res[0]['positions']
                out[key + '/first_velocities'] = res[0]['velocities']
                out[key + '/first_rotations'] = res[0]['rotations']
                out[key + '/first_times'] = res[0]['times']
                assert np.array_equal(res[0]['Mext'][0], ex) and np.array_equal(res[0]['Mint'][0], inm[:3, :3])
            # hit counting on raw (unselected) tracks: the sampled states at 1, 2, 4, ... ms
            picked = 0
            for i in range(len(seeds)):
                track = np.concatenate([hist[i, 1:2, :3], hist[i, 2:1000:2, :3]])
                ho, hw, hg = mh._count_hits(list(track), direction)
                if (len(ho) + len(hw) + len(hg) > 0 and picked < 3) or i == 0:
                    keep = track[:360].astype(np.float32).astype(np.float64)       # float32-representable: half the file size
                    ho, hw, hg = mh._count_hits(list(keep), direction)
                    hit_cases.append((direction, keep, ho, hw, hg))
                    picked += i != 0
            print('trajgen %s/%s: %d of %d seeds accepted (%.0f s)' % (mode, direction, len(res), len(seeds), time.time() - t0))
    # ---- seeds that the device generator accepts for every mode (found with a device search over the first ~20 000 seeds):
    # the reference worker, again on the oracle integrator, exercises every mode's acceptance and cut branch
    RARE = {"final_lose/left_to_right": [162, 166, 167, 170], "final_lose/right_to_left": [162, 167, 169, 170],
            "final_win/left_to_right": [9366, 9807, 10696, 11390], "final_win/right_to_left": [1417, 3309, 6651, 6948],
            "intermediate/left_to_right": [190, 203, 242, 296], "intermediate/right_to_left": [190, 193, 242, 251],
            "first_good/left_to_right": [290, 341, 484, 625], "first_good/right_to_left": [417, 823, 955, 1121],
            "first_short/left_to_right": [1218, 2194, 3239, 5097], "first_short/right_to_left": [592, 760, 1012, 2008],
            "first_long/left_to_right": [268, 318, 479, 686], "first_long/right_to_left": [246, 490, 494, 540]}
    for cfg, seeds in RARE.items():
        mode, direction = cfg.split('/')
        seeds = seeds + [s + 1 for s in seeds]            # the neighbours are (mostly) rejected: both outcomes per mode
        st = [T.init_state(sd, mode, direction) for sd in seeds]
        r = np.stack([a[0] for a in st]); v = np.stack([a[1] for a in st]); w = np.stack([a[2] for a in st])
        hist = np.zeros((len(seeds), 1001, 9))
        hist[:, 0] = np.concatenate([r, v, w], axis=1)
        for k in range(1, 1001):
            r, v, w = T.step_ms(r, v, w, 1)
            hist[:, k] = np.concatenate([r, v, w], axis=1)
        for i in range(len(seeds)):
            history[(hist[i, 0, :3].tobytes(), hist[i, 0, 3:9].tobytes())] = hist[i]
        res = ms.find_valid_trajectories_worker((seeds, mode, direction))
        key = 'rare/%s/%s' % (mode, direction)
        out[key + '/all_seeds'] = np.array(seeds, dtype=np.int64)
        out[key + '/seeds'] = np.array([t['seed'] for t in res], dtype=np.int64)
        out[key + '/n'] = np.array([len(t['positions']) for t in res], dtype=np.int64)
        out[key + '/bounces'] = np.concatenate([t['bounces'] for t in res]) if res else np.zeros(0)
        out[key + '/n_bounces'] = np.array([len(t['bounces']) for t in res], dtype=np.int64)
        print('trajgen rare %s: %d of %d accepted (%.0f s)' % (cfg, len(res), len(seeds), time.time() - t0))
    out['hits/n'] = np.array([len(hit_cases)])
    for j, (direction, track, ho, hw, hg) in enumerate(hit_cases):
        out['hits/%d/direction' % j] = np.array([T.DIRECTIONS.index(direction)])
        out['hits/%d/track' % j] = track.astype(np.float64)
        out['hits/%d/opponent' % j] = np.array(ho, dtype=np.float64)
        out['hits/%d/own' % j] = np.array(hw, dtype=np.float64)
        out['hits/%d/ground' % j] = np.array(hg, dtype=np.float64)
    out['n_sel'] = np.array([n_sel])
    np.savez_compressed(os.path.join(OUT, 'trajgen.npz'), **out)
    print('trajgen.npz: %d arrays, %.0f KB' % (len(out), os.path.getsize(os.path.join(OUT, 'trajgen.npz')) / 1024))



def gen_trajgen_edges():
    """f2 at its edges (tests/helpers/trajgen_edge_cases.py): the reference's `_count_hits` on every named crafted track -- the
    three hit lists only, the tracks are rebuilt from the helper -- and, for the fixed seed lists of the stop-rule tests, what
    the ORACLE's sampling loop gives (sample counts, stop reasons, margins; not reference-derived, recorded to spare the GPU
    suite a minute of numpy integration)."""
    from oracle import trajgen_ref as T
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from helpers import trajgen_edge_cases as C
    install_mujoco_standin({})
    import syntheticdataset.helper as mh
    out = {}
    cases = C.all_named_cases()
    out['names'] = np.array([c['name'] for c in cases])
    for j, key in enumerate(('opponent', 'own', 'ground')):
        lists = [mh._count_hits(list(C.track(c)), c['direction'])[j] for c in cases]
        out['hits/%s/n' % key] = np.array([len(h) for h in lists], dtype=np.int64)
        out['hits/%s/t' % key] = np.array([t for h in lists for t in h], dtype=np.float64)
    for mode in T.MODES:
        for direction in T.DIRECTIONS:
            seeds = C.stop_seeds(mode, direction)
            _, _, _, ns, why, margins = T.simulate(seeds, mode, direction, want_stop=True)
            key = 'stop/%s/%s' % (mode, direction)
            out[key + '/seeds'] = np.array(seeds, dtype=np.int64)
            out[key + '/n_saved'] = ns
            out[key + '/reason'] = np.array([T.STOP_REASONS.index(w) for w in why], dtype=np.int64)
            out[key + '/margins'] = margins
            print('trajgen edges %s/%s: %s' % (mode, direction, {w: why.count(w) for w in T.STOP_REASONS}))
    mode, direction = C.CAMERA_COMBO                  # the same seeds seen by a camera whose principal point is moved
    _, _, _, ns, why, margins = T.simulate(C.stop_seeds(mode, direction), mode, direction, camera=C.shifted_camera(), want_stop=True)
    out['stop_camera/n_saved'], out['stop_camera/margins'] = ns, margins
    out['stop_camera/reason'] = np.array([T.STOP_REASONS.index(w) for w in why], dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, 'trajgen_edges.npz'), **out)
    print('trajgen_edges.npz: %d named cases, %.0f KB' % (len(cases), os.path.getsize(os.path.join(OUT, 'trajgen_edges.npz')) / 1024))


def ref_table_hrnet(sd_np, resolution):
    from tabledetection.models.hrnet import MyHRNet
    orig = torch.load
    torch.load = lambda *a, **k: {}
    try:
        m = MyHRNet(resolution=resolution)
    finally:
        torch.load = orig
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=False)
    assert not unexpected and all('num_batches_tracked' in k for k in missing)
    m.eval()
    return m


E2E_CASES = {            # name: (frames, H, W, fps, ball seed, table seed, uplift seed, clip seed)
    'small': (51, 96, 160, 60.0, 61, 62, 63, 64),
    'full': (12, 704, 1280, 50.0, 71, 72, 73, 74),
}


def gen_e2e():
    """The whole hot path through the REFERENCE's own modules, chained as interface.py does (BallDetector.predict :93-120,
    TableDetector.predict :148-172, TableTennisPipeline.predict :265-289, UpliftingModel.predict_without_normalization :221-247):
      frames -> NormalizeImage -> WASBNet -> extract_position (table variant) -> filter_trajectory_ball          (ball)
      frames -> NormalizeImage -> MyHRNet -> extract_position (table variant) -> filter_trajectory_table (DBSCAN) (table)
      -> _uplifting_transform -> MultiStageModel -> transform_rotationaxes -> crop to T'.
    The clips are generated AT the detectors' input resolution, so that the reference's `Resize` (cv2.resize, not importable
    here: the one unpinned step of a1) is the identity and the chain is the reference's arithmetic end to end.  As on the hub
    surface without the un-vendored SegFormer++ detectors, each detector stands in for both sides of its agreement filter."""
    from balldetection.transforms import NormalizeImage as BallNorm
    from tabledetection.transforms import NormalizeImage as TableNorm
    from tabledetection.helper_tabledetection import extract_position_torch_gaussian as extract_position_table
    from inference.utils import filter_trajectory_ball, filter_trajectory_table, _uplifting_transform
    from uplifting.model import get_model
    from uplifting.helper import transform_rotationaxes
    import einops as eo
    from upliftingtabletennis_amd import weights, synth
    out = {}
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    for name, (n, h, w, fps, s_ball, s_table, s_up, s_clip) in E2E_CASES.items():
        t0 = time.time()
        frames, track = synth.synth_frames(n, h, w, seed=s_clip)
        ball_model, _ = ref_wasb(weights.random_wasb_state_dict(s_ball, planted=True))
        table_model = ref_table_hrnet(weights.random_wasb_state_dict(s_table, planted=True, in_ch=3, head_out=13, plant_all_heads=True), (w, h))
        up_model = get_model('connectstage', 'large', 'dynamic', 'new')
        up_model.load_state_dict({k: torch.from_numpy(v) for k, v in weights.random_uplift_state_dict(s_up, 'large').items()}, strict=True)
        up_model.eval()
        bnorm, tnorm = BallNorm(mean=mean, std=std), TableNorm(mean=mean, std=std)
        # 1. ball detection (interface.py:276-279 builds the triples, :102-119 runs them one by one)
        pred_pos, argmax, top2 = [], [], []
        for i in range(1, n - 1):
            data = bnorm({'image': frames[i].copy(), 'prev_image': frames[i - 1].copy(), 'next_image': frames[i + 1].copy()})
            element = np.concatenate([data['prev_image'], data['image'], data['next_image']], axis=2)
            element = eo.rearrange(element, 'h w c -> c h w').astype(np.float32)
            with torch.no_grad():
                preds, _ = ball_model(torch.tensor(element).unsqueeze(0))
                pos = extract_position_table(preds, 1920, 1080)
            pred_pos.append(pos.squeeze(0))
            flat = preds.reshape(-1)
            argmax.append(int(flat.argmax()))
            top2.append(torch.topk(flat, 2).values.numpy())
        ball_positions = np.concatenate(pred_pos, axis=0)
        filtered, valid_idx, times_ball = filter_trajectory_ball(ball_positions, ball_positions, fps)
        # 2. table detection on every frame (:281-283)
        kps, targmax = [], []
        for i in range(n):
            data = tnorm({'image': frames[i].copy()})
            element = eo.rearrange(data['image'], 'h w c -> c h w').astype(np.float32)
            with torch.no_grad():
                tp = table_model(torch.tensor(element).unsqueeze(0))
                kps.append(extract_position_table(tp, 1920, 1080))
            targmax.append(tp.reshape(13, -1).argmax(1).numpy())
        table_keypoints = np.concatenate(kps, axis=0)
        filtered_table = filter_trajectory_table(table_keypoints, table_keypoints)
        # 3. uplifting (:286-287, :221-247)
        ball_coords, table_coords, times, mask = _uplifting_transform(filtered, filtered_table, times_ball)
        with torch.no_grad():
            rot, pos3 = up_model(ball_coords, table_coords, mask, times)
            spin = transform_rotationaxes(rot, pos3.clone())
        t_prime = int(mask.sum().item())
        out.update({name + '/meta': np.array([n, h, w, s_ball, s_table, s_up, s_clip], np.int64), name + '/fps': np.array(fps),
                    name + '/track': track, name + '/ball_argmax': np.array(argmax, np.int64), name + '/ball_top2': np.stack(top2),
                    name + '/ball_positions': ball_positions, name + '/filtered': filtered, name + '/valid_idx': valid_idx,
                    name + '/times_ball': times_ball, name + '/table_argmax': np.stack(targmax).astype(np.int64),
                    name + '/table_keypoints': table_keypoints, name + '/filtered_table': filtered_table,
                    name + '/u_ball': ball_coords.numpy(), name + '/u_table': table_coords.numpy(), name + '/u_times': times.numpy(),
                    name + '/u_mask': mask.numpy(), name + '/rot': rot.numpy(), name + '/pos3d_full': pos3.numpy(),
                    name + '/spin': spin.squeeze(0).numpy(), name + '/pos3d': pos3[:, :t_prime].squeeze(0).numpy()})
        print('e2e %-5s %d frames %dx%d: %d detections kept, T\'=%d, spin %s (%.0f s); ball margin min %.3f'
              % (name, n, h, w, len(valid_idx), t_prime, spin.squeeze(0).numpy().round(4).tolist(), time.time() - t0,
                 float(np.min(np.stack(top2)[:, 0] - np.stack(top2)[:, 1]))))
    np.savez_compressed(os.path.join(OUT, 'e2e.npz'), **out)
    print('e2e.npz: %.0f KB' % (os.path.getsize(os.path.join(OUT, 'e2e.npz')) / 1024))


def gen_calib():
    """f4: the reference's `calibrate_camera` (inference/utils.py:312) and `TableTennisPipeline.reproject` arithmetic on
    synthetic keypoints: the 13 table points projected through known cameras, with pixel noise, an outlier and an
    invisible keypoint."""
    if 'mujoco' not in sys.modules:
        install_mujoco_standin({})
    for name in ('matplotlib', 'matplotlib.pyplot', 'sklearn', 'sklearn.cluster'):
        pass
    import inference.utils as iu
    from uplifting.helper import table_points, world2cam, cam2img
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(7)
    out, t0 = {}, time.time()
    cams = [(2100.0, 2050.0, [0.1, -0.3, 6.5], [2.05, 0.02, 0.03]), (1500.0, 1540.0, [-0.4, 0.2, 5.0], [1.9, -0.1, 0.4]), (2600.0, 2600.0, [0.0, 0.0, 8.0], [2.2, 0.05, -0.2])]
    for ci, (fx, fy, t, eul) in enumerate(cams):
        Mint = np.array([[fx, 0, 960, 0], [0, fy, 540, 0], [0, 0, 1, 0.0]])
        Mext = np.eye(4)
        Mext[:3, :3] = Rotation.from_euler('xyz', eul).as_matrix()
        Mext[:3, 3] = t
        uv = cam2img(world2cam(table_points.astype(np.float64), Mext), Mint)
        kp = np.concatenate([uv + rng.normal(0, 0.6, uv.shape), np.ones((13, 1))], axis=1)
        if ci == 1:
            kp[4, :2] += [40.0, -25.0]           # outlier
            kp[7, 2] = 0                          # invisible
        M_int, M_ext = iu.calibrate_camera(kp)
        out['calib/%d/keypoints' % ci] = kp
        out['calib/%d/Mint' % ci] = np.asarray(M_int)
        out['calib/%d/Mext' % ci] = np.asarray(M_ext)
        pts = rng.uniform(-1.5, 1.5, (5, 3)) + [0, 0, 1.0]
        out['calib/%d/points' % ci] = pts
        out['calib/%d/reproj' % ci] = cam2img(world2cam(pts, np.asarray(M_ext)), np.asarray(M_int))
        print('calib case %d: %.0f s, fx %.1f fy %.1f' % (ci, time.time() - t0, M_int[0][0], M_int[1][1]))
    out['n'] = np.array([len(cams)])
    np.savez_compressed(os.path.join(OUT, 'calib.npz'), **out)


def _calib64_one(job):
    import inference.utils as iu
    ci, kp = job
    M_int, M_ext = iu.calibrate_camera(kp)
    return ci, np.asarray(M_int), np.asarray(M_ext)


def gen_calib64():
    """f4, the distribution: the reference's `calibrate_camera` on 64 seeded synthetic cameras -- poses and focal
    lengths from the ranges the reference trains its uplift net on (uplifting/data.py:60-64, via upliftingtabletennis_amd.synth._random_camera),
    pixel noise sigma 0.3 / 0.6 / 1.0 px, every fourth camera with one gross outlier, every fifth with one invisible keypoint.  ~30 s of
    SciPy BFGS per camera: eight worker processes."""
    if 'mujoco' not in sys.modules:
        install_mujoco_standin({})
    import multiprocessing as mp
    import inference.utils as iu          # noqa: F401  (imported before the fork)
    from uplifting.helper import table_points, world2cam, cam2img
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from upliftingtabletennis_amd import synth
    rng = np.random.default_rng(64)
    jobs, out = [], {}
    for ci in range(64):
        R, c, f = synth._random_camera(rng)
        Mext = np.eye(4); Mext[:3, :3] = R; Mext[:3, 3] = -R @ c
        Mint = np.array([[f, 0, 960.0, 0], [0, f * rng.uniform(0.98, 1.02), 540.0, 0], [0, 0, 1, 0.0]])
        uv = cam2img(world2cam(table_points.astype(np.float64), Mext), Mint)
        kp = np.concatenate([uv + rng.normal(0, (0.3, 0.6, 1.0)[ci % 3], uv.shape), np.ones((13, 1))], axis=1)
        if ci % 4 == 3:
            kp[int(rng.integers(0, 9)), :2] += rng.choice([-1, 1], 2) * rng.uniform(20, 60, 2)          # one gross outlier (not on keys 10 / 11: fixed in every subset)
        if ci % 5 == 4:
            kp[int(rng.integers(0, 9)), 2] = 0
        out['calib64/%d/keypoints' % ci] = kp
        out['calib64/%d/Mint_true' % ci] = Mint
        out['calib64/%d/Mext_true' % ci] = Mext
        jobs.append((ci, kp))
    t0 = time.time()
    with mp.get_context('fork').Pool(8) as pool:
        for ci, mi, me in pool.imap_unordered(_calib64_one, jobs):
            out['calib64/%d/Mint' % ci] = mi
            out['calib64/%d/Mext' % ci] = me
            print('calib64 camera %d done (%.0f s)' % (ci, time.time() - t0), flush=True)
    out['n'] = np.array([64])
    np.savez_compressed(os.path.join(OUT, 'calib64.npz'), **out)


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    install_stubs()
    torch.manual_seed(0)
    which = sys.argv[1:] or ['wasb', 'refine', 'uplift', 'glue', 'full', 'table', 'trajgen', 'trajgen_edges', 'calib', 'e2e', 'hard', 'hard_table']
    for w_ in which:
        {'wasb': gen_wasb, 'refine': gen_refine, 'uplift': gen_uplift, 'glue': gen_glue, 'full': gen_fullsize, 'table': gen_table, 'trajgen': gen_trajgen, 'trajgen_edges': gen_trajgen_edges, 'calib': gen_calib, 'calib64': gen_calib64, 'e2e': gen_e2e, 'hard': gen_hard, 'hard_table': gen_hard_table}[w_]()
