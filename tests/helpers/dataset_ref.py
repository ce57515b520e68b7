"""numpy restatement of the reference's synthetic uplift dataset (uplifting/data.py::TableTennisDataset.__getitem__, :77-166,
`sample_camera` :168-223, `transform_resolution` :527-553, and the train transforms of uplifting/transformations.py), written
from its behaviour so that the CPU tests can check it against the fixture the reference itself produced
(tests/golden/dataset.npz) and so that the golden tool can compute how far every decision sits from its threshold.

Randomness: two MT19937 streams rebuilt from `genrand_uint32`.
  PyRandom   CPython's `random` after `random.seed(s)` (init_by_array): `random()`, `uniform`, `randint` (rejection on getrandbits)
  NpRandom   numpy's legacy global stream after `np.random.seed(s)` (init_genrand): `random`, masked-rejection `randint` /
             `choice`, the polar-method `normal` with its cached second value
A sample with seed s is what the reference returns for `random.seed(s); np.random.seed(s); dataset[i]`.

`Sample` carries the nine outputs in float64 (the reference casts to float32 at the very end) plus the integer record:
fps, n_frames, camera_tries, camera_success, nearest-frame indices, blur sample indices, dropped frames.
"""
import numpy as np

HEIGHT, WIDTH = 1440, 2560
BASE_FX, BASE_FY = 2710, 2907
TABLE_HEIGHT, TABLE_WIDTH, TABLE_LENGTH = 0.76, 1.525, 2.74
SEQUENCE_LEN = 50
ORIGINAL_RESOLUTION = (2560, 1440)
FPS_BOUNDS = (20, 65)
EVAL_FPS = 50
MAX_TRIES = 100
TRANSFORM_NAMES = ['MotionBlur', 'RandomizeDetections', 'RandomStop', 'RandomDetection', 'RandomMissing', 'TableMissing']
ALL_ON = (1 << len(TRANSFORM_NAMES)) - 1

_W2, _W4 = TABLE_WIDTH / 2, TABLE_WIDTH / 2 + 0.1525
TABLE_POINTS = np.array([
    [-TABLE_LENGTH / 2, _W2, TABLE_HEIGHT], [-TABLE_LENGTH / 2, -_W2, TABLE_HEIGHT], [0.0, _W2, TABLE_HEIGHT], [0.0, -_W2, TABLE_HEIGHT],
    [TABLE_LENGTH / 2, _W2, TABLE_HEIGHT], [TABLE_LENGTH / 2, -_W2, TABLE_HEIGHT], [0.0, _W4, TABLE_HEIGHT], [0.0, -_W4, TABLE_HEIGHT],
    [0.0, 0.0, TABLE_HEIGHT], [0.0, _W4, TABLE_HEIGHT + 0.1525], [0.0, -_W4, TABLE_HEIGHT + 0.1525],
    [-TABLE_LENGTH / 2, 0, TABLE_HEIGHT], [TABLE_LENGTH / 2, 0, TABLE_HEIGHT]])

_PHI0 = float(np.rad2deg(np.arctan2(TABLE_WIDTH / 2, TABLE_LENGTH / 2)))
SAMPLED = {'fx': (0.6 * BASE_FX, 2.0 * BASE_FX), 'fy': (0.6 * BASE_FY, 2.0 * BASE_FY), 'distance': (7, 17),
           'phi': (_PHI0, _PHI0 + 180), 'theta': (30, 70)}


# ---------------------------------------------------------------------------------------------------- MT19937
class MT19937:
    def __init__(self):
        self.mt, self.pos, self.words, self.count = [0] * 624, 624, [], 0
        self.record = False

    def init_genrand(self, s):
        mt = self.mt
        mt[0] = s & 0xffffffff
        for i in range(1, 624):
            mt[i] = (1812433253 * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i) & 0xffffffff
        self.pos = 624

    def init_by_array(self, key):
        self.init_genrand(19650218)
        mt, i, j = self.mt, 1, 0
        for _ in range(max(624, len(key))):
            mt[i] = ((mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525)) + key[j] + j) & 0xffffffff
            i += 1
            j += 1
            if i >= 624:
                mt[0] = mt[623]
                i = 1
            if j >= len(key):
                j = 0
        for _ in range(623):
            mt[i] = ((mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941)) - i) & 0xffffffff
            i += 1
            if i >= 624:
                mt[0] = mt[623]
                i = 1
        mt[0] = 0x80000000
        self.pos = 624

    def genrand_uint32(self):
        # one element of the state is renewed per draw: the same values as the usual 624-word regeneration, which walks the
        # state in this order and reads only entries it has not passed yet (or, from 227 on, entries it has renewed)
        mt = self.mt
        i = self.pos % 624
        y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7fffffff)
        v = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908b0df if y & 1 else 0)
        mt[i] = v
        self.pos = i + 1
        self.count += 1
        v ^= v >> 11
        v ^= (v << 7) & 0x9d2c5680
        v ^= (v << 15) & 0xefc60000
        v ^= v >> 18
        if self.record:
            self.words.append(v)
        return v

    def double(self):
        a, b = self.genrand_uint32() >> 5, self.genrand_uint32() >> 6
        return (a * 67108864.0 + b) / 9007199254740992.0


class PyRandom(MT19937):
    def __init__(self, seed):
        super().__init__()
        s, key = abs(int(seed)), []
        while s:
            key.append(s & 0xffffffff)
            s >>= 32
        self.init_by_array(key or [0])

    def uniform(self, a, b):
        return a + (b - a) * self.double()

    def randint(self, a, b):
        n = b - a + 1
        k = n.bit_length()
        r = self.genrand_uint32() >> (32 - k)
        while r >= n:
            r = self.genrand_uint32() >> (32 - k)
        return a + r


class NpRandom(MT19937):
    def __init__(self, seed):
        super().__init__()
        self.init_genrand(int(seed))
        self.min_r2_margin = np.inf          # closest approach of an accepted / rejected polar r2 to 1

    def random(self):
        return self.double()

    def randint(self, lo, hi):
        rng = hi - lo - 1
        if rng == 0:
            return lo
        mask = rng
        for s in (1, 2, 4, 8, 16):
            mask |= mask >> s
        v = self.genrand_uint32() & mask
        while v > rng:
            v = self.genrand_uint32() & mask
        return lo + v

    def gauss_pair(self):
        """(first returned, second returned) of the legacy polar method."""
        while True:
            x1 = 2.0 * self.double() - 1.0
            x2 = 2.0 * self.double() - 1.0
            r2 = x1 * x1 + x2 * x2
            self.min_r2_margin = min(self.min_r2_margin, abs(r2 - 1.0))
            if r2 < 1.0 and r2 != 0.0:
                break
        f = np.sqrt(-2.0 * np.log(r2) / r2)
        return f * x2, f * x1

    def normal(self, scale, count):
        assert count % 2 == 0
        out = np.empty(count)
        for i in range(0, count, 2):
            a, b = self.gauss_pair()
            out[i], out[i + 1] = 0 + scale * a, 0 + scale * b
        return out


# ---------------------------------------------------------------------------------------------------- geometry
def _norm(v):
    return np.sqrt(v.dot(v))


def _get_mext(c, f, r):
    up = np.cross(f, r)
    up = up / _norm(up)
    R = np.stack([r, up, f])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = -(R @ c)
    return M


def project(points, mext, mint):
    p = np.atleast_2d(points)
    cam = p @ mext[:3, :3].T + mext[:3, 3]
    img = cam @ mint.T
    out = img[:, :2] / img[:, 2:3]
    return out if np.ndim(points) == 2 else out[0]


class Sample(dict):
    __getattr__ = dict.__getitem__


def nearest_frames(blur_times, fps):
    step = 1.0 / fps
    t0, t1 = blur_times[0], blur_times[-1]
    n = int(np.ceil((t1 - t0) / step))
    delta = (t0 + step) - t0
    times = t0 + np.arange(n) * delta
    if n > 1:
        times[1] = t0 + step
    ins = np.searchsorted(blur_times, times)
    ir = np.clip(ins, 0, len(blur_times) - 1)
    il = np.clip(ins - 1, 0, len(blur_times) - 1)
    dl, dr = np.abs(blur_times[il] - times), np.abs(blur_times[ir] - times)
    return times, np.where(dr < dl, ir, il)


def sample_camera(rnd, r_world, rec):
    """Up to 100 tries; returns Mint, Mext, r_img, table_img, tries.  `rec` collects the decision margins."""
    tries, valid = 0, False
    while not valid and tries < MAX_TRIES:
        fx, fy = rnd.uniform(*SAMPLED['fx']), rnd.uniform(*SAMPLED['fy'])
        mint = np.array([[fx, 0, (WIDTH - 1) / 2], [0, fy, (HEIGHT - 1) / 2], [0, 0, 1]])
        distance = rnd.uniform(*SAMPLED['distance'])
        phi = rnd.uniform(*SAMPLED['phi'])
        theta = rnd.uniform(*SAMPLED['theta'])
        lookat = np.array((rnd.uniform(-0.2, 0.2), rnd.uniform(-0.2, 0.2), TABLE_HEIGHT))
        th, ph = np.radians(theta), np.radians(phi)
        c = np.array([distance * np.sin(th) * np.cos(ph), distance * np.sin(th) * np.sin(ph), distance * np.cos(th)])
        c = c + np.array([0., 0., TABLE_HEIGHT])
        d = c - lookat
        f = -d / _norm(d)
        eps = rnd.uniform(-0.1, 0.1)
        r = np.array([-f[1] / f[0] - f[2] / f[0] * eps, 1, eps])
        r = r / _norm(r)
        u = -np.cross(f, r)
        rec['min_u2'] = min(rec['min_u2'], abs(u[2]))
        if u[2] < 0:
            r = np.array([f[1] / f[0] - f[2] / f[0] * eps, -1, eps])
            r = r / _norm(r)
        mext = _get_mext(c, f, r)
        r_img = project(r_world, mext, mint)
        table_img = project(TABLE_POINTS, mext, mint)
        lim = np.array([WIDTH, HEIGHT])
        valid = bool(np.all((r_img >= 0) & (r_img < lim)))
        ex, ey = r_img[:, 0].max() - r_img[:, 0].min(), r_img[:, 1].max() - r_img[:, 1].min()
        rec['min_border'] = min(rec['min_border'], np.abs(r_img).min(), np.abs(r_img - lim).min())
        rec['min_extent'] = min(rec['min_extent'], abs(ex - 0.15 * WIDTH), abs(ey - 0.15 * HEIGHT))
        valid = valid and bool(ex > 0.15 * WIDTH or ey > 0.15 * HEIGHT)
        tries += 1
    return mint, mext, r_img, table_img, tries


def build_sample(traj, seed, mode='train', config=None, enabled=ALL_ON):
    """traj: reference-format dictionary ('positions', 'times', 'bounces', 'rotations', 'Mext', 'Mint').
    config: dict with the six strengths (train mode).  enabled: bit k switches TRANSFORM_NAMES[k] on."""
    py, npr = PyRandom(seed), NpRandom(seed)
    rec = {'min_u2': np.inf, 'min_border': np.inf, 'min_extent': np.inf}
    blur_pos, blur_times = np.asarray(traj['positions'], np.float64), np.asarray(traj['times'], np.float64)
    bounces = np.asarray(traj['bounces'], np.float64)
    fps = py.randint(*FPS_BOUNDS) if mode == 'train' else EVAL_FPS
    times, idx = nearest_frames(blur_times, fps)
    r_world = blur_pos[idx]
    if mode == 'train':
        mint, mext, r_img, table_img, tries = sample_camera(py, r_world, rec)
    else:
        mint, mext, tries = np.array(traj['Mint'][0], np.float64), np.array(traj['Mext'][0], np.float64), 0
        r_img, table_img = project(r_world, mext, mint), project(TABLE_POINTS, mext, mint)
    T = len(times)
    L = min(T, SEQUENCE_LEN)
    mask = np.arange(SEQUENCE_LEN) < T

    def pad(a):
        out = np.zeros((SEQUENCE_LEN,) + a.shape[1:])
        out[:L] = a[:L]
        return out
    r_img, r_world, times = pad(r_img), pad(r_world), pad(times)
    widx = np.full(SEQUENCE_LEN, -1, np.int64)          # stored sample behind every r_world row (-1: zeros)
    widx[:L] = idx[:L]
    hits = bounces if len(bounces) else np.array([-1.0])
    table_img = np.concatenate([table_img, np.ones((13, 1))], axis=1)
    sx, sy = WIDTH / ORIGINAL_RESOLUTION[0], HEIGHT / ORIGINAL_RESOLUTION[1]
    for a in (r_img, table_img):
        a[:, 0] = (a[:, 0] + 0.5) * sx - 0.5
        a[:, 1] = (a[:, 1] + 0.5) * sy - 0.5
    mint = mint.copy()
    mint[0, 0], mint[1, 1] = mint[0, 0] * sx, mint[1, 1] * sy
    mint[0, 2], mint[1, 2] = (mint[0, 2] + 0.5) * sx - 0.5, (mint[1, 2] + 0.5) * sy - 0.5
    wh = np.array([WIDTH, HEIGHT], np.float64)
    blur_idx = np.full(SEQUENCE_LEN, -1, np.int64)
    dropped = np.zeros(SEQUENCE_LEN, bool)
    on = (lambda k: mode == 'train' and bool(enabled >> k & 1))
    if on(0) and config['blur_strength'] != 0:
        bs = config['blur_strength']
        before, after = times.copy(), times.copy()
        before[1:L] = times[:L - 1]
        after[:L - 1] = times[1:L]
        before[:L] = times[:L] + bs * (before - times)[:L]
        after[:L] = times[:L] + bs * (after - times)[:L]
        for i in range(L):
            lo = int(np.searchsorted(blur_times, before[i], 'left'))
            hi = int(np.searchsorted(blur_times, after[i], 'right'))
            k = lo + npr.randint(0, hi - lo)
            blur_idx[i], widx[i] = k, k
            r_world[i] = blur_pos[k]
            r_img[i] = project(blur_pos[k], mext, mint)
    if on(1):
        std = config['randomize_std']
        r_img = r_img + npr.normal(std, 2 * SEQUENCE_LEN).reshape(SEQUENCE_LEN, 2)
        table_img[:, :2] = table_img[:, :2] + npr.normal(std, 26).reshape(13, 2)
    if on(2) and not npr.random() > config['stop_prob']:
        hit = hits[0]
        if hit > 0:
            hit_ind = int(np.argmin(np.abs(times - hit)))
            seq_len = int(mask.sum())
            if seq_len - hit_ind >= 4:
                n_after = npr.randint(4, seq_len - hit_ind + 1)
                mask[hit_ind + n_after:] = False
                r_img[~mask] = r_img[~mask] * 0
                r_world[~mask] = r_world[~mask] * 0
                times[~mask] = times[~mask] * 0
    if on(3):
        p = config['randdet_prob']
        for i in range(int(mask.sum())):
            if npr.random() < p:
                r_img[i] = np.array([npr.random(), npr.random()]) * wh
        for i in range(13):
            if npr.random() < p:
                table_img[i, :2] = np.array([npr.random(), npr.random()]) * wh
    if on(4):
        p = config['randmiss_prob']
        new = [np.zeros_like(a) for a in (r_img, r_world, times)]
        new_mask, cur = np.zeros_like(mask), 0
        for i in range(int(mask.sum())):
            if not npr.random() < p:
                new_mask[cur] = True
                for dst, src in zip(new, (r_img, r_world, times)):
                    dst[cur] = src[i]
                cur += 1
            else:
                dropped[i] = True
        (r_img, r_world, times), mask = new, new_mask
    if on(5):
        p = config['tablemiss_prob']
        for i in range(13):
            if npr.random() < p:
                table_img[i, 2] = 0
                table_img[i, :2] = np.array([npr.random(), npr.random()]) * wh
    r_img = r_img / wh
    table_img[:, :2] = table_img[:, :2] / wh
    return Sample(r_img=r_img, table_img=table_img, mask=mask.astype(np.float64), r_world=r_world,
                  rotation=np.asarray(traj['rotations'][0], np.float64), times=times, bounces=np.asarray(hits[0:1], np.float64),
                  Mint=mint, Mext=mext, fps=fps, n_frames=T, camera_tries=tries, camera_success=int(mode == 'train' and tries < MAX_TRIES),
                  nearest=idx, blur_idx=blur_idx, dropped=dropped, margins=rec, r2_margin=npr.min_r2_margin,
                  py_words=py.pos, np_stream=npr, py_stream=py)


OUTPUTS = ['r_img', 'table_img', 'mask', 'r_world', 'rotation', 'times', 'bounces', 'Mint', 'Mext']


# ---------------------------------------------------------------------------------------------------- data_paths
def data_paths(counts, mode):
    """Order of `TableTennisDataset.data_paths` (data.py:28-50) as (trajectory mode, direction, index) triples.
    counts[(tm, direction)] = number of trajectory folders.  The reference shuffles the list accumulated so far with a fresh
    random.Random(0) before every (mode, direction) block is cut and appended."""
    import random
    out = []
    for tm in ['intermediate', 'final_win', 'final_lose', 'first_good', 'first_short', 'first_long']:
        for direction in ['left_to_right', 'right_to_left']:
            n = counts[(tm, direction)]
            dps = sorted('trajectory_%04d' % i for i in range(n))
            random.Random(0).shuffle(out)
            if mode == 'train':
                dps = dps[:int(0.7 * n)]
            elif mode == 'test':
                dps = dps[int(0.8 * n):]
            else:
                raise ValueError('Unknown mode %s' % mode)
            out.extend((tm, direction, int(d[-4:])) for d in dps)
    return out
