"""Seeded inputs for the evaluation metrics' shape-edge tests (tests/test_uplift_eval_gpu.py): fp32 arrays of any N and T >= 2 that
keep the conditions under which two correct fp64 evaluations agree to rounding -- every local spin component at least 1e-3 of its
vector's norm, the angle within [1, 179] degrees, a horizontal first step of at least 1e-3 m, a 1 in every mask row, every camera
at least 4 m from the track.  Mask rows cycle through: all ones, a prefix, a prefix with holes inside the track, a single 1."""
import numpy as np

from . import uplift_eval_ref as R

DT = 0.01


def f32(x):
    return np.ascontiguousarray(x, np.float32)


def masks(rng, n, t):
    m = np.zeros((n, t), np.float32)
    for i in range(n):
        kind = i % 4
        if kind == 0:
            m[i] = 1
        elif kind == 1:
            m[i, :int(rng.integers(1, t + 1))] = 1
        elif kind == 2 and t >= 4:
            length = int(rng.integers(4, t + 1))
            m[i, :length] = 1
            m[i, rng.choice(np.arange(1, length - 1), size=int(rng.integers(1, min(4, length - 1))), replace=False)] = 0
        else:
            m[i, int(rng.integers(0, t))] = 1
    return m


def tracks(rng, n, t):
    p0 = np.stack([rng.uniform(-1.4, 1.4, n), rng.uniform(-0.7, 0.7, n), rng.uniform(0.1, 0.5, n)], -1)
    heading, speed = rng.uniform(0, 2 * np.pi, n), rng.uniform(2.0, 9.0, n)
    v = np.stack([speed * np.cos(heading), speed * np.sin(heading), rng.uniform(-1.0, 3.0, n)], -1)
    tt = (np.arange(t) * DT)[None, :, None]
    pos = p0[:, None] + v[:, None] * tt
    pos[:, :, 2] -= 0.5 * 9.81 * tt[:, :, 0] ** 2
    return f32(pos)


def _components_ok(loc):
    return (np.abs(loc) / np.linalg.norm(loc, axis=1, keepdims=True)).min(1) >= 2e-3


def _draw(rng, n, accept):
    """(n, 3) fp32 vectors, each redrawn until accept(candidates, rows) holds for it."""
    out, todo = np.zeros((n, 3), np.float32), np.ones(n, bool)
    while todo.any():
        rows = np.flatnonzero(todo)
        cand = f32(rng.normal(0, 1, (rows.size, 3)) * rng.uniform(10, 120, (rows.size, 1)))
        ok = accept(cand, rows)
        out[rows[ok]] = cand[ok]
        todo[rows[ok]] = False
    return out


def val_inputs(seed, n, t, mode):
    """-> dict of the arguments of val_metrics (numpy fp32)."""
    rng = np.random.default_rng(seed)
    r_world, mask = tracks(rng, n, t), masks(rng, n, t)
    rotation = _draw(rng, n, lambda c, rows: _components_ok(R.transform_rotationaxes(c, r_world[rows])))
    gt = R.transform_rotationaxes(rotation, r_world)

    def accept(c, rows):
        loc = R.transform_rotationaxes(c, r_world[rows]) if mode == 'global' else c.astype(np.float64)
        ang = R.angle_deg(loc, gt[rows])
        return _components_ok(loc) & (ang >= 1.5) & (ang <= 178.5)
    return {'pred_rotation': _draw(rng, n, accept), 'pred_position': f32(r_world + rng.normal(0, 0.03, r_world.shape)), 'r_world': r_world,
            'rotation': rotation, 'mask': mask, 'transform_mode': mode}


def look_at(cam, target):
    fwd = (target - cam) / np.linalg.norm(target - cam)
    right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
    right /= np.linalg.norm(right)
    rot = np.stack([right, np.cross(fwd, right), fwd])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = rot, -rot @ cam
    return m


def real_inputs(seed, n, t, mode):
    """-> dict of the arguments of val_real_metrics (numpy; spin_class int64 cycling 1, 2, 0), a camera of its own per sample."""
    rng = np.random.default_rng(seed)
    truth, mask = tracks(rng, n, t).astype(np.float64), masks(rng, n, t)
    Mext, Mint = np.zeros((n, 4, 4)), np.zeros((n, 3, 3))
    for i in range(n):
        cam = np.array([rng.uniform(-1.5, 1.5), (1.0 if i % 2 else -1.0) * rng.uniform(7.0, 10.0), rng.uniform(1.2, 3.5)])
        Mext[i] = look_at(cam, np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.2, 0.2), rng.uniform(0.0, 0.4)]))
        f = rng.uniform(1800, 3200)
        Mint[i] = [[f, 0, R.WIDTH / 2 + rng.uniform(-30, 30)], [0, f * rng.uniform(0.98, 1.02), R.HEIGHT / 2 + rng.uniform(-30, 30)], [0, 0, 1]]
    Mext, Mint = f32(Mext), f32(Mint)
    uv, _ = R.project(truth, Mint, Mext)
    pred_position = f32(truth + rng.normal(0, 0.03, truth.shape))
    pred_rotation = _draw(rng, n, lambda c, rows: _components_ok(R.transform_rotationaxes(c, pred_position[rows]) if mode == 'global' else c.astype(np.float64)))
    return {'pred_rotation': pred_rotation, 'pred_position': pred_position, 'r_img': f32((uv + rng.normal(0, 3.0, uv.shape)) / np.array([R.WIDTH, R.HEIGHT])),
            'mask': mask, 'Mint': Mint, 'Mext': Mext, 'spin_class': np.array([(1, 2, 0)[i % 3] for i in range(n)], np.int64), 'transform_mode': mode}
