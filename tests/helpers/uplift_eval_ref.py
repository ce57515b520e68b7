"""float64 numpy restatement of the reference's evaluation metrics: val() (uplifting/train.py:141-225) and val_real() (:228-299),
with the helpers they call (uplifting/helper.py: transform_rotationaxes :394-420, binary_metrics :290-308, world2cam :190-195,
cam2img :154-157; WIDTH / HEIGHT :26).  Inputs are cast to float64 first; sums are numpy's pairwise float64 sums.

Stated as the product states them: a time step with mask == 0 is selected out, and the cosine is clamped to [-1, 1]
before acos.  On inputs with finite masked slots and a cosine inside (-1, 1) both are the reference's arithmetic."""
import numpy as np

WIDTH, HEIGHT = 2560, 1440
TOPSPIN_CLASS, BACKSPIN_CLASS = 1, 2


def transform_rotationaxes(rotation, r_gt):
    """helper.py:394-420: e_x along the horizontal first step, e_y = e_z x e_x, e_z up."""
    rotation, r_gt = np.asarray(rotation, np.float64), np.asarray(r_gt, np.float64)
    v0 = np.zeros((r_gt.shape[0], 3))
    v0[:, :2] = r_gt[:, 1, :2] - r_gt[:, 0, :2]                                  # :411
    with np.errstate(invalid='ignore', divide='ignore'):
        e_x = v0 / np.linalg.norm(v0, axis=-1, keepdims=True)                    # :412
    w_0 = rotation[:, 0] * e_x[:, 0] + rotation[:, 1] * e_x[:, 1]                # :416 (e_x has no z part; a 0 / 0 frame leaves w_2 alone)
    w_1 = rotation[:, 1] * e_x[:, 0] - rotation[:, 0] * e_x[:, 1]                # :413, :417: e_y = (-e_x[1], e_x[0], 0)
    w_2 = rotation[:, 2]                                                         # :418
    return np.stack([w_0, w_1, w_2], axis=-1)


def masked_mean(dist, mask):
    """train.py:149 / :235: sum_t dist * mask / sum_t mask per sample, masked slots selected out."""
    mask = np.asarray(mask, np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(mask != 0, dist * mask, 0.0).sum(axis=1) / mask.sum(axis=1)


def local_spins(pred_rotation, r_world, rotation, transform_mode):
    gt = transform_rotationaxes(rotation, r_world)                               # train.py:169
    pred = transform_rotationaxes(pred_rotation, r_world) if transform_mode == 'global' else np.asarray(pred_rotation, np.float64)          # :170-171
    return pred, gt


def angle_deg(pred, gt):
    """train.py:148, with the cosine clamped."""
    with np.errstate(invalid='ignore', divide='ignore'):
        cos = (pred * gt).sum(1) / (np.linalg.norm(pred, axis=1) * np.linalg.norm(gt, axis=1))
    cos = np.where(cos > 1, 1.0, np.where(cos < -1, -1.0, cos))
    return np.degrees(np.arccos(cos))


def val_metrics(pred_rotation, pred_position, r_world, rotation, mask, transform_mode='global'):
    pred, gt = local_spins(pred_rotation, r_world, rotation, transform_mode)
    n = pred.shape[0]
    d = pred - gt
    with np.errstate(invalid='ignore'):
        pos_err = np.sqrt(((np.asarray(pred_position, np.float64) - np.asarray(r_world, np.float64)) ** 2).sum(-1))
    out = {'metric': np.sqrt((d ** 2).sum(1)).sum() / n,                                                       # :143, :174, :185
           'metric_x': np.abs(d[:, 0]).sum() / n, 'metric_y': np.abs(d[:, 1]).sum() / n, 'metric_z': np.abs(d[:, 2]).sum() / n,          # :144-146
           'metric_abs': np.abs(np.linalg.norm(pred, axis=1) - np.linalg.norm(gt, axis=1)).sum() / n,          # :147
           'metric_angle': angle_deg(pred, gt).sum() / n,                                                      # :148
           'metric_position': masked_mean(pos_err, mask).sum() / n,                                            # :149
           'mse': (d ** 2).sum() / (3 * n)}
    # :181 calls binary_metrics(pred_rotation, rotation) into (rot_gt, rot_pred): the PREDICTION sits in the rot_gt slot
    s_gt, s_pred = np.sign(pred), np.sign(gt)
    out['TP'] = ((s_gt == 1) & (s_pred == 1)).sum(0)                             # helper.py:303
    out['TN'] = ((s_gt == -1) & (s_pred == -1)).sum(0)                           # :304
    out['FP'] = ((s_gt == -1) & (s_pred == 1)).sum(0)                            # :305
    out['FN'] = ((s_gt == 1) & (s_pred == -1)).sum(0)                            # :306
    with np.errstate(invalid='ignore', divide='ignore'):
        out['accuracy'] = (out['TP'] + out['TN']) / (out['TP'] + out['TN'] + out['FP'] + out['FN']).astype(np.float64)          # train.py:195
    out['number'] = n
    return out


def project(pred_position, Mint, Mext):
    """cam2img(world2cam(pred_position, Mext), Mint) with per-sample matrices (helper.py:190-195, :154-157)."""
    p = np.asarray(pred_position, np.float64)
    hom = np.concatenate([p, np.ones(p.shape[:2] + (1,))], axis=-1)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        cam = np.einsum('bij,btj->bti', np.asarray(Mext, np.float64), hom)
        cam = cam[:, :, :3] / cam[:, :, 3:4]
        img = np.einsum('bij,btj->bti', np.asarray(Mint, np.float64)[:, :3, :3], cam)
        return img[:, :, :2] / img[:, :, 2:3], cam[:, :, 2]


def roc_auc(labels, scores):
    """P(score of a positive > score of a negative) + P(equal) / 2, by counting pairs: what roc_auc_score's area equals."""
    y, s = np.asarray(labels).astype(bool), np.asarray(scores, np.float64)
    pos, neg = s[y], s[~y]
    if pos.size == 0 or neg.size == 0:
        raise ValueError('Only one class present in y_true.')
    return ((pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()) / (pos.size * neg.size)


def val_real_metrics(pred_rotation, pred_position, r_img, mask, Mint, Mext, spin_class, transform_mode='global'):
    out = val_real_counts(pred_rotation, pred_position, r_img, mask, Mint, Mext, spin_class, transform_mode)
    TP, TN, FP, FN = out['TP'], out['TN'], out['FP'], out['FN']
    out['accuracy'] = (TP + TN) / (TP + TN + FP + FN)                            # :287
    f1_plus = 2 * TP / (2 * TP + FP + FN)
    f1_minus = 2 * TN / (2 * TN + FN + FP)
    out['macro_f1'] = (f1_plus + f1_minus) / 2
    out['roc_auc'] = roc_auc(out['labels'], out['scores'])
    return out


def val_real_counts(pred_rotation, pred_position, r_img, mask, Mint, Mext, spin_class, transform_mode='global'):
    """val_real up to its counts: everything but the ratios of train.py:287-291."""
    pred =transform_rotationaxes(pred_rotation, pred_position) if transform_mode == 'global' else np.asarray(pred_rotation, np.float64)          # train.py:252-253
    n = pred.shape[0]
    uv, _ = project(pred_position, Mint, Mext)                                   # :260
    gt = np.asarray(r_img, np.float64) * np.array([WIDTH, HEIGHT], np.float64)   # :256, transformations.py:279
    with np.errstate(invalid='ignore', over='ignore'):
        dist = np.sqrt(((uv - gt) ** 2).sum(-1))
    metric_2D = masked_mean(dist, mask).sum() / n                                # :235, :285
    cls = np.asarray(spin_class).astype(np.int64)
    score = pred[:, 1]
    top, back = cls == TOPSPIN_CLASS, cls == BACKSPIN_CLASS
    TP, FN = int((top & (score > 0)).sum()), int((top & ~(score > 0)).sum())     # :267-271
    TN, FP = int((back & (score < 0)).sum()), int((back & ~(score < 0)).sum())   # :272-276
    ann = top | back
    return {'metric_2D': metric_2D, 'metric_2D_normed': metric_2D / (WIDTH ** 2 + HEIGHT ** 2) ** 0.5, 'TP': TP, 'TN': TN, 'FP': FP, 'FN': FN,
            'scores': score[ann], 'labels': top[ann].astype(np.int64), 'number': n}


def input_conditions(g, mode):
    """The fixture's conditions (tools/make_goldens_eval.py enforces them, the host test re-checks them) -> dict of margins."""
    out = {}
    pred, gt = local_spins(g['val/%s/pred_rotation' % mode], g['val/r_world'], g['val/rotation'], mode)
    out['val_angle'] = angle_deg(pred, gt)
    out['val_component'] = np.minimum(np.abs(pred) / np.linalg.norm(pred, axis=1, keepdims=True), np.abs(gt) / np.linalg.norm(gt, axis=1, keepdims=True)).min()
    rw = np.asarray(g['val/r_world'], np.float64)
    out['val_step'] = np.linalg.norm(rw[:, 1, :2] - rw[:, 0, :2], axis=1).min()
    out['val_mask_rows'] = np.asarray(g['val/mask']).sum(1).min()
    for s in ('a', 'b'):
        p = 'real_%s/' % s
        pos = np.asarray(g[p + 'pred_position'], np.float64)
        loc = transform_rotationaxes(g[p + mode + '/pred_rotation'], pos) if mode == 'global' else np.asarray(g[p + mode + '/pred_rotation'], np.float64)
        out[p + 'component'] = (np.abs(loc) / np.linalg.norm(loc, axis=1, keepdims=True)).min()
        out[p + 'step'] = np.linalg.norm(pos[:, 1, :2] - pos[:, 0, :2], axis=1).min()
        out[p + 'mask_rows'] = np.asarray(g[p + 'mask']).sum(1).min()
        _, depth = project(pos, g[p + 'Mint'], g[p + 'Mext'])
        out[p + 'depth'] = depth[np.asarray(g[p + 'mask']) != 0].min()
        out[p + 'classes'] = set(np.asarray(g[p + 'spin_class']).astype(int).tolist())
    return out
