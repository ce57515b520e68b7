"""A float64 numpy restatement of the gradient of the detectors' heatmap loss into the predicted heatmaps: the explicit adjoint of
`detect_eval_ref.upsample` applied to the residual 2 w (up(pred) - target).  tests/test_detect_grad_host.py pins it to what the
reference's autograd returned (tests/golden/detect_grad.npz) and to torch's float64 autograd; the GPU tests use it for the shapes
the fixture does not hold.

    grad[i, j] = scale * sum_y sum_x 2 w(y, x) (up[y, x] - target[y, x]) a_y(i) b_x(j)

a_y(i): the weight with which output row y reads source row i -- 1 - lambda on y0, lambda on y1, their sum where the clamp at the
last row makes y0 == y1; b_x(j) the same for columns."""
import numpy as np

from .detect_eval_ref import HEIGHT, WIDTH, src_coords, target, upsample


def read_weights(out, inp):
    """(out, inp) float64: row d holds the weights with which output index d reads the source indices."""
    i0, i1, lam = src_coords(out, inp)
    a = np.zeros((out, inp))
    d = np.arange(out)
    a[d, i0] = 1.0 - lam
    np.add.at(a, (d, i1), lam)          # (i1 == i0 at the clamp: the sum)
    return a


def unread(out, inp):
    """bool (inp,): the source indices no output index reads."""
    i0, i1, _ = src_coords(out, inp)
    read = np.zeros(inp, bool)
    read[i0] = read[i1] = True
    return ~read


def residual(pred, centre, has_target, sigma, weighted, size):
    """2 w (up(pred) - target) of one (h, w) map at the output size, float64."""
    up = upsample(pred, size)
    if not has_target:
        return 2.0 * up
    t = target(centre, sigma, size)
    r = 2.0 * (up - t.astype(np.float64))
    return np.where(t > np.float32(0.1), 100.0, 1.0) * r if weighted else r


def heatmap_loss_grad(pred, centres, has_target, sigma=6, weighted=True, size=(HEIGHT, WIDTH), scale=None):
    """-> (N, C, h, w) float64: the gradient of scale * sum of w (up(pred) - target)^2 with respect to pred; scale=None: the element
    mean 1 / (N C size[0] size[1])."""
    pred = np.asarray(pred, np.float32)
    n, c, h, w = pred.shape
    if scale is None:
        scale = 1.0 / (n * c * size[0] * size[1])
    a, b = read_weights(size[0], h), read_weights(size[1], w)
    out = np.zeros((n, c, h, w))
    for i in range(n):
        for j in range(c):
            out[i, j] = scale * (a.T @ residual(pred[i, j], centres[i][j], has_target[i][j], sigma, weighted, size) @ b)
    return out
