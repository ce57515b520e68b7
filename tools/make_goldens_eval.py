#!/usr/bin/env python3
"""Generate tests/golden/uplift_eval.npz by running the REFERENCE's own uplifting/train.py::val() and ::val_real() on the CPU.

Runs only where the reference sources are (TTUP_REFERENCE); the tests read the .npz alone.  tensorboard / cv2 are stubbed as in
tools/make_goldens.py.  Neither function needs a dataset or a checkpoint: the model is a stub that returns recorded predictions
batch by batch, the loader is a list of batches with a `.dataset` that has one camera, the writer records `add_scalar`.  What the
reference computes but never hands to the writer is read off its own calls: the per-batch results of `helper.binary_metrics`
(val's sign counts) and the (labels, scores) it passes to `roc_auc_score` (val_real's scores, from which its four counts follow).

Cases: both transform_modes; val on 165 samples in batches of 64 + 64 + 37; val_real on 11 samples in batches of 4 + 4 + 3 (set
'a') and on 69 in batches of 64 + 5 (set 'b'); T = 50; epoch = 1, so the confusion-matrix images are skipped.

Input conditions, enforced here and re-checked by tests/test_uplift_eval_host.py (tests/helpers/uplift_eval_ref.py::input_conditions):
the angle between predicted and target spin is within [1, 179] degrees; every local spin component is at least 1e-3 of its
vector's norm; the horizontal first step is at least 1e-3 m; every mask row has a 1; every valid slot of the val_real sets lies at
a camera depth of at least 0.5 m; both spin classes and unannotated samples are present.  Under them fp32 and fp64 evaluation
cannot differ in a sign count, and the reference's fp32 acos is well conditioned.

    python tools/make_goldens_eval.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('TTUP_REFERENCE', '/root/reference')
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from tests.helpers import uplift_eval_cases as C  # noqa: E402
from tests.helpers import uplift_eval_ref as R  # noqa: E402
from tools.make_goldens import install_stubs  # noqa: E402

T = 50
MODES = ('global', 'local')
VAL_BATCHES = (64, 64, 37)
REAL_BATCHES = {'a': (4, 4, 3), 'b': (64, 5)}


def spin_ok(pred_local, gt_local=None):
    ok = (np.abs(pred_local) / np.linalg.norm(pred_local, axis=1, keepdims=True)).min(1) >= 2e-3
    if gt_local is not None:
        ok &= (np.abs(gt_local) / np.linalg.norm(gt_local, axis=1, keepdims=True)).min(1) >= 2e-3
        ang = R.angle_deg(pred_local, gt_local)
        ok &= (ang >= 1.5) & (ang <= 178.5)
    return ok


def make_val(rng, n):
    r_world = C.tracks(rng, n, T)
    mask = C.masks(rng, n, T)
    pred_position = C.f32(r_world + rng.normal(0, 0.03, r_world.shape))
    rotation = np.zeros((n, 3), np.float32)
    pred = {m: np.zeros((n, 3), np.float32) for m in MODES}
    todo = np.ones(n, bool)
    while todo.any():                                            # redraw the samples that miss a condition
        k = int(todo.sum())
        rot = C.f32(rng.normal(0, 1, (k, 3)) * rng.uniform(10, 120, (k, 1)))
        noise = rng.normal(0, 1, (k, 3)) * rng.uniform(5, 80, (k, 1))
        pg = C.f32(rot + noise)                                    # 'global': a world-frame prediction
        gt_local = R.transform_rotationaxes(rot, r_world[todo])
        pl = C.f32(gt_local + noise)                               # 'local': a ball-frame prediction
        ok = spin_ok(R.transform_rotationaxes(pg, r_world[todo]), gt_local) & spin_ok(pl.astype(np.float64), gt_local)
        idx = np.flatnonzero(todo)[ok]
        rotation[idx], pred['global'][idx], pred['local'][idx] = rot[ok], pg[ok], pl[ok]
        todo[idx] = False
    return {'r_world': r_world, 'mask': mask, 'rotation': rotation, 'pred_position': pred_position,
            'global/pred_rotation': pred['global'], 'local/pred_rotation': pred['local']}


def make_real(rng, n):
    truth = C.tracks(rng, n, T).astype(np.float64)
    mask = C.masks(rng, n, T)
    Mext, Mint = np.zeros((n, 4, 4)), np.zeros((n, 3, 3))
    for i in range(n):                                           # a camera of its own per sample
        side = 1.0 if i % 2 else -1.0
        cam = np.array([rng.uniform(-1.5, 1.5), side * rng.uniform(7.0, 10.0), rng.uniform(1.2, 3.5)])
        Mext[i] = C.look_at(cam, np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), rng.uniform(0.0, 0.4)]))
        f = rng.uniform(1800, 3200)
        Mint[i] = [[f, 0, R.WIDTH / 2 + rng.uniform(-30, 30)], [0, f * rng.uniform(0.98, 1.02), R.HEIGHT / 2 + rng.uniform(-30, 30)], [0, 0, 1]]
    Mext, Mint = C.f32(Mext), C.f32(Mint)
    uv, _ = R.project(truth, Mint, Mext)
    r_img = C.f32((uv + rng.normal(0, 3.0, uv.shape)) / np.array([R.WIDTH, R.HEIGHT]))
    pred_position = C.f32(truth + rng.normal(0, 0.03, truth.shape))
    while True:                                                  # the local frame of 'global' is built from the PREDICTED first step
        short = np.linalg.norm(pred_position[:, 1, :2].astype(np.float64) - pred_position[:, 0, :2], axis=1) < 5e-3
        if not short.any():
            break
        pred_position[short] = C.f32(truth[short] + rng.normal(0, 0.03, truth[short].shape))
    spin_class =np.array([(1, 2, 0)[i % 3] for i in range(n)], np.int64)
    rng.shuffle(spin_class)
    pred = {}
    for m in MODES:
        rot = np.zeros((n, 3), np.float32)
        todo = np.ones(n, bool)
        while todo.any():
            k = int(todo.sum())
            cand = C.f32(rng.normal(0, 1, (k, 3)) * rng.uniform(10, 120, (k, 1)))
            loc = R.transform_rotationaxes(cand, pred_position[todo]) if m == 'global' else cand.astype(np.float64)
            ok = spin_ok(loc)
            idx = np.flatnonzero(todo)[ok]
            rot[idx] = cand[ok]
            todo[idx] = False
        # four in five annotated samples get the sign of local component 1 that their class asks for (the frame change is linear)
        loc1 = (R.transform_rotationaxes(rot, pred_position) if m == 'global' else rot.astype(np.float64))[:, 1]
        want = np.where(spin_class == R.TOPSPIN_CLASS, 1.0, -1.0) * np.where(rng.uniform(size=n) < 0.8, 1.0, -1.0)
        rot[np.sign(loc1) != want] *= -1
        pred[m] = rot
    _, depth = R.project(pred_position, Mint, Mext)
    assert depth[mask != 0].min() >= 0.5
    return {'r_img': r_img, 'mask': mask, 'Mint': Mint, 'Mext': Mext, 'spin_class': spin_class, 'pred_position': pred_position,
            'global/pred_rotation': pred['global'], 'local/pred_rotation': pred['local']}


class StubModel:
    """`model(r_img, table_img, mask, times)` -> the next recorded (pred_rotation, pred_position)."""

    def __init__(self, rot, pos, batches):
        self.chunks, at = [], 0
        for b in batches:
            self.chunks.append((torch.from_numpy(rot[at:at + b].copy()), torch.from_numpy(pos[at:at + b].copy())))
            at += b
        self.calls = 0

    def eval(self):
        return self

    def train(self):
        return self

    def __call__(self, r_img, table_img, mask, times):
        out = self.chunks[self.calls]
        assert out[0].shape[0] == r_img.shape[0]
        self.calls += 1
        return out


class Loader(list):
    def __init__(self, batches):
        super().__init__(batches)
        self.dataset = types.SimpleNamespace(num_cameras=1, cam_num=0)


class Writer:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, step):
        self.scalars[tag] = float(value)

    def add_image(self, *a, **k):
        raise AssertionError('epoch = 1 writes no confusion matrix')

    def add_text(self, *a, **k):
        pass

    def add_hparams2(self, *a, **k):
        pass


def split(arrays, batches):
    out, at = [], 0
    for b in batches:
        out.append(tuple(torch.from_numpy(np.ascontiguousarray(a[at:at + b])) for a in arrays))
        at += b
    return out


def main():
    install_stubs()
    import uplifting.train as train
    assert (train.WIDTH, train.HEIGHT, train.TOPSPIN_CLASS, train.BACKSPIN_CLASS) == (R.WIDTH, R.HEIGHT, R.TOPSPIN_CLASS, R.BACKSPIN_CLASS)
    rng = np.random.default_rng(20250)
    out = {}
    sets = {'val': make_val(rng, sum(VAL_BATCHES))}
    for s, batches in REAL_BATCHES.items():
        sets['real_' + s] = make_real(rng, sum(batches))
    for name, d in sets.items():
        for k, v in d.items():
            out['%s/%s' % (name, k)] = v

    counts = []
    binary_metrics = train.binary_metrics
    train.binary_metrics = lambda a, b: counts.append([t.numpy().copy() for t in binary_metrics(a, b)]) or tuple(torch.from_numpy(c) for c in counts[-1])
    auc_args = []
    roc_auc_score = train.roc_auc_score
    train.roc_auc_score = lambda labels, scores: auc_args.append((list(labels), list(scores))) or roc_auc_score(labels, scores)

    for mode in MODES:
        config = types.SimpleNamespace(transform_mode=mode, get_hparams=lambda: {})
        d = sets['val']
        n = d['mask'].shape[0]
        dummy = (np.zeros((n, T, 2), np.float32), np.zeros((n, 13, 3), np.float32), np.zeros((n, T), np.float32), np.zeros((n, 1), np.float32))
        r_img, table_img, times, hits = dummy
        loader = Loader(split((r_img, table_img, d['mask'], d['r_world'], d['rotation'], times, hits, hits, hits), VAL_BATCHES))
        model, writer = StubModel(d[mode + '/pred_rotation'], d['pred_position'], VAL_BATCHES), Writer()
        del counts[:]
        ret = train.val(model, loader, writer, 1, 'cpu', config)
        assert model.calls == len(VAL_BATCHES) == len(counts)
        for tag, v in writer.scalars.items():
            out['val/%s/scalar/%s' % (mode, tag)] = np.float64(v)
        out['val/%s/return' % mode] = np.float64(ret)
        for i, k in enumerate(('TP', 'TN', 'FP', 'FN')):
            out['val/%s/%s' % (mode, k)] = np.sum([c[i] for c in counts], axis=0).astype(np.int64)
        for s, batches in REAL_BATCHES.items():
            d = sets['real_' + s]
            n = d['mask'].shape[0]
            table_img, times, hits = np.zeros((n, 13, 3), np.float32), np.zeros((n, T), np.float32), np.zeros((n, 1), np.float32)
            loader = Loader(split((d['r_img'], table_img, d['mask'], times, hits, d['Mint'], d['Mext'], d['spin_class']), batches))
            model, writer = StubModel(d[mode + '/pred_rotation'], d['pred_position'], batches), Writer()
            del auc_args[:]
            ret = train.val_real(model, loader, writer, 1, 'cpu', config)
            assert model.calls == len(batches) and len(auc_args) == 1
            for tag, v in writer.scalars.items():
                out['real_%s/%s/scalar/%s' % (s, mode, tag)] = np.float64(v)
            out['real_%s/%s/return' % (s, mode)] = np.array(ret, np.float64)
            out['real_%s/%s/labels' % (s, mode)] = np.array(auc_args[0][0], np.int64)
            out['real_%s/%s/scores' % (s, mode)] = np.array(auc_args[0][1], np.float64)          # the reference's own fp32 scores
        cond = R.input_conditions(out, mode)
        assert 1.0 <= cond['val_angle'].min() and cond['val_angle'].max() <= 179.0 and cond['val_component'] >= 1e-3 and cond['val_step'] >= 1e-3
        assert cond['val_mask_rows'] >= 1
        for s in REAL_BATCHES:
            p = 'real_%s/' % s
            assert cond[p + 'component'] >= 1e-3 and cond[p + 'step'] >= 1e-3 and cond[p + 'mask_rows'] >= 1 and cond[p + 'depth'] >= 0.5
            assert cond[p + 'classes'] == {0, R.TOPSPIN_CLASS, R.BACKSPIN_CLASS}
        print(mode, {k: (v if not isinstance(v, np.ndarray) else (v.min(), v.max())) for k, v in cond.items()})
    path = os.path.join(ROOT, 'tests', 'golden', 'uplift_eval.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
