"""The ViTPose head's training-mode forward and its backward restated in explicit float64 numpy arithmetic, without autograd
(DESIGN.md section 29): two ConvTranspose2d(k4, s2, p1, no bias) + BatchNorm2d(eps 1e-5, momentum 0.1) + ReLU, a 1x1 conv.

Parameters are a dict of arrays under short names: W1 (384,256,4,4), g1, b1, rm1, rv1 (256), W2 (256,256,4,4), g2, b2, rm2, rv2, Wf (C,256),
bf (C).  Activations are NCHW here.  `torch_reference` is the same definition through torch's own operators and autograd, in the
dtype asked for: the host test holds the restatement against it in float64, and the GPU test takes its float32 result's distance
from the restatement as the measure of what float32 arithmetic costs on each case.
"""
import numpy as np

EPS, MOMENTUM = 1e-5, 0.1
PARAMS = ('W1', 'g1', 'b1', 'rm1', 'rv1', 'W2', 'g2', 'b2', 'rm2', 'rv2', 'Wf', 'bf')
GRADS = ('W1', 'g1', 'b1', 'W2', 'g2', 'b2', 'Wf', 'bf')


def deconv(x, w):
    """conv_transpose2d(x (B,cin,h,w), w (cin,cout,4,4), stride 2, padding 1): input pixel (y, x) adds x w[:, :, ky, kx] to output pixel
    (2y - 1 + ky, 2x - 1 + kx)."""
    b, cin, h, wd = x.shape
    cout = w.shape[1]
    t = (x.transpose(0, 2, 3, 1).reshape(-1, cin) @ w.reshape(cin, cout * 16)).reshape(b, h, wd, cout, 4, 4)
    out = np.zeros((b, cout, 2 * h + 2, 2 * wd + 2), t.dtype)          # one pixel of border: output index + 1
    for ky in range(4):
        for kx in range(4):
            out[:, :, ky:ky + 2 * h:2, kx:kx + 2 * wd:2] += t[..., ky, kx].transpose(0, 3, 1, 2)
    return out[:, :, 1:-1, 1:-1]


def gather(dz):
    """G[(b,y,x), co, ky, kx] = dz[b, co, 2y - 1 + ky, 2x - 1 + kx], zero outside the map: the operand of both backward products."""
    b, cout, h2, w2 = dz.shape
    h, wd = h2 // 2, w2 // 2
    p = np.zeros((b, cout, h2 + 2, w2 + 2), dz.dtype)
    p[:, :, 1:-1, 1:-1] = dz
    g = np.empty((b, h, wd, cout, 4, 4), dz.dtype)
    for ky in range(4):
        for kx in range(4):
            g[..., ky, kx] = p[:, :, ky:ky + h2:2, kx:kx + w2:2].transpose(0, 2, 3, 1)
    return g.reshape(b * h * wd, cout * 16)


def deconv_backward(x, w, dz):
    """-> (dx like x, dw like w)"""
    b, cin, h, wd = x.shape
    g = gather(dz)
    dx = (g @ w.reshape(cin, -1).T).reshape(b, h, wd, cin).transpose(0, 3, 1, 2)
    dw = (x.transpose(0, 2, 3, 1).reshape(-1, cin).T @ g).reshape(w.shape)
    return dx, dw


def bn_forward(z, gamma, beta, run_mean, run_var, train):
    """-> y, xhat, rstd, the statistics used (mean, biased var), the running statistics afterwards"""
    if train:
        n = z.shape[0] * z.shape[2] * z.shape[3]
        mean = z.mean(axis=(0, 2, 3))
        var = ((z - mean[None, :, None, None]) ** 2).mean(axis=(0, 2, 3))
        new_mean = (1 - MOMENTUM) * run_mean + MOMENTUM * mean
        new_var = (1 - MOMENTUM) * run_var + MOMENTUM * var * n / (n - 1)
    else:
        mean, var, new_mean, new_var = run_mean, run_var, run_mean, run_var
    rstd = 1.0 / np.sqrt(var + EPS)
    xhat = (z - mean[None, :, None, None]) * rstd[None, :, None, None]
    return xhat * gamma[None, :, None, None] + beta[None, :, None, None], xhat, rstd, mean, var, new_mean, new_var


def bn_backward(dy, xhat, rstd, gamma, train):
    """-> dz, dgamma, dbeta"""
    dgamma, dbeta = (dy * xhat).sum(axis=(0, 2, 3)), dy.sum(axis=(0, 2, 3))
    c = lambda v: v[None, :, None, None]
    if train:
        n = dy.shape[0] * dy.shape[2] * dy.shape[3]
        dz = c(gamma * rstd) * (dy - c(dbeta / n) - xhat * c(dgamma / n))
    else:
        dz = dy * c(gamma * rstd)
    return dz, dgamma, dbeta


def forward(feat, p, train):
    """feat (B,384,hp,wp) float64 -> everything the backward and the tests read"""
    f = {'feat': feat}
    f['z1'] = deconv(feat, p['W1'])
    f['y1'], f['xhat1'], f['rstd1'], f['mean1'], f['var1'], f['rm1'], f['rv1'] = bn_forward(f['z1'], p['g1'], p['b1'], p['rm1'], p['rv1'], train)
    f['a1'] = np.maximum(f['y1'], 0)
    f['z2'] = deconv(f['a1'], p['W2'])
    f['y2'], f['xhat2'], f['rstd2'], f['mean2'], f['var2'], f['rm2'], f['rv2'] = bn_forward(f['z2'], p['g2'], p['b2'], p['rm2'], p['rv2'], train)
    f['a2'] = np.maximum(f['y2'], 0)
    f['heat'] = np.einsum('ck,bkhw->bchw', p['Wf'], f['a2']) + p['bf'][None, :, None, None]
    return f


def backward(f, p, dheat, train, gate1=None, gate2=None):
    """-> {'W1', 'g1', 'b1', 'W2', 'g2', 'b2', 'Wf', 'bf', 'feat'}.  gate1 / gate2: boolean masks of the two ReLUs (NCHW); default y > 0."""
    gate1 = f['y1'] > 0 if gate1 is None else gate1
    gate2 = f['y2'] > 0 if gate2 is None else gate2
    g = {'Wf': np.einsum('bchw,bkhw->ck', dheat, f['a2']), 'bf': dheat.sum(axis=(0, 2, 3))}
    dy2 = np.einsum('ck,bchw->bkhw', p['Wf'], dheat) * gate2
    dz2, g['g2'], g['b2'] = bn_backward(dy2, f['xhat2'], f['rstd2'], p['g2'], train)
    da1, g['W2'] = deconv_backward(f['a1'], p['W2'], dz2)
    dz1, g['g1'], g['b1'] = bn_backward(da1 * gate1, f['xhat1'], f['rstd1'], p['g1'], train)
    g['feat'], g['W1'] = deconv_backward(f['feat'], p['W1'], dz1)
    return g


def undecided(f, p, margin=1e-4):
    """The elements of y1, y2 whose ReLU gate float32 cannot be held to: |y| <= margin (|gamma| + |beta|)"""
    c = lambda v: v[None, :, None, None]
    return (np.abs(f['y1']) <= margin * c(np.abs(p['g1']) + np.abs(p['b1'])), np.abs(f['y2']) <= margin * c(np.abs(p['g2']) + np.abs(p['b2'])))


def torch_reference(feat, p, dheat, train, dtype):
    """The same definition through F.conv_transpose2d, F.batch_norm(training=...), relu and conv2d with autograd, in `dtype` on the CPU
    -> (heat, running statistics {'rm1','rv1','rm2','rv2'}, grads as `backward` returns them), all as float64 numpy"""
    import torch
    import torch.nn.functional as F
    t = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=k in GRADS) for k, v in p.items()}
    x = torch.tensor(feat, dtype=dtype, requires_grad=True)
    run = {k: t[k].detach().clone() for k in ('rm1', 'rv1', 'rm2', 'rv2')}
    a = x
    for l in ('1', '2'):
        z = F.conv_transpose2d(a, t['W' + l], stride=2, padding=1)
        a = torch.relu(F.batch_norm(z, run['rm' + l], run['rv' + l], t['g' + l], t['b' + l], training=train, momentum=MOMENTUM, eps=EPS))
    heat = F.conv2d(a, t['Wf'][:, :, None, None], t['bf'])
    heat.backward(torch.tensor(dheat, dtype=dtype))
    grads = {k: t[k].grad.double().numpy() for k in GRADS}
    grads['feat'] = x.grad.double().numpy()
    return heat.detach().double().numpy(), {k: v.double().numpy() for k, v in run.items()}, grads


def rel_l2(a, b):
    """|a - b|_2 / |b|_2 (0 / 0 = 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d, n = np.linalg.norm((a - b).ravel()), np.linalg.norm(b.ravel())
    return 0.0 if d == 0 else d / n if n > 0 else np.inf


def rel_max(a, b):
    """max |a - b| over the largest magnitude of b (0 / 0 = 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d, n = np.abs(a - b).max(initial=0.0), np.abs(b).max(initial=0.0)
    return 0.0 if d == 0 else d / n if n > 0 else np.inf
