"""fp64 numpy restatement of IDRLoss's patch terms (the reference's ssim_loss_fn / get_ssim_loss / get_roughnesssmooth_loss,
code/model/loss.py:54-120, :237-253, :266-276) with their analytic gradients: slices, no convolution call, no autograd.
DESIGN.md 6n states the formulas.  Shared by the CPU and GPU tests of the patch loss."""
import os

import numpy as np

WIN, R = 11, 5
C1, C2 = 0.01 ** 2, 0.03 ** 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'patch_loss.npz')


def window():
    """The 11-tap Gaussian, sigma 1.5, as the reference formed it: its fp32 taps (kept in the golden file: numpy's exp and
    torch's differ in the last bit of four of them), cast"""
    return golden().window.astype(np.float64)


def _valid(a, g):
    """separable 'valid' filter over the last two axes"""
    V = a.shape[-1] - 2 * R
    rows = sum(g[k] * a[..., k:k + V, :] for k in range(WIN))
    return sum(g[k] * rows[..., :, k:k + V] for k in range(WIN))


def _full(a, g):
    """its transpose: V x V -> (V + 10) x (V + 10)"""
    V = a.shape[-1]
    rows = np.zeros(a.shape[:-2] + (V + 2 * R, V))
    for k in range(WIN):
        rows[..., k:k + V, :] += g[k] * a
    out = np.zeros(a.shape[:-2] + (V + 2 * R, V + 2 * R))
    for k in range(WIN):
        out[..., :, k:k + V] += g[k] * rows
    return out


def eroded(m, P):
    """m [N, P, P] bool -> the AND over the 11 x 11 window clipped to the patch"""
    e = np.ones_like(m)
    for y in range(P):
        for x in range(P):
            e[:, y, x] = m[:, max(y - R, 0):y + R + 1, max(x - R, 0):x + R + 1].all(axis=(1, 2))
    return e


def ssim_term(X, Y, m, r_patch):
    """X, Y [n, 3], m [n] bool -> (1 - sum(e S) / M, d / dX [n, 3]); (0, zeros) when no pixel survives the erosion"""
    P = 2 * r_patch
    g = window()
    x = X.astype(np.float64).reshape(-1, P, P, 3).transpose(0, 3, 1, 2)
    y = Y.astype(np.float64).reshape(-1, P, P, 3).transpose(0, 3, 1, 2)
    e = eroded(m.reshape(-1, P, P), P).astype(np.float64)
    M = int(e.sum())
    if M == 0:
        return 0.0, np.zeros((X.shape[0], 3))
    mu1, mu2, exx, eyy, exy = _valid(x, g), _valid(y, g), _valid(x * x, g), _valid(y * y, g), _valid(x * y, g)
    s11, s22, s12 = exx - mu1 * mu1, eyy - mu2 * mu2, exy - mu1 * mu2
    ln, ld, cn, cd = 2 * mu1 * mu2 + C1, mu1 * mu1 + mu2 * mu2 + C1, 2 * s12 + C2, s11 + s22 + C2
    l, cs = ln / ld, cn / cd
    S = np.ones(e.shape)
    S[:, R:P - R, R:P - R] = (l * cs).mean(axis=1)
    value = 1.0 - (S * e).sum() / M
    # the partial derivatives of l cs with respect to mu1, E[x x], E[x y] (s11, s12 and l depend on mu1)
    d_cs_s11, d_cs_s12 = -cn / (cd * cd), 2.0 / cd
    f_mu = (2 * mu2 * ld - ln * 2 * mu1) / (ld * ld) * cs + l * (d_cs_s11 * (-2 * mu1) + d_cs_s12 * (-mu2))
    f_xx, f_xy = l * d_cs_s11, l * d_cs_s12
    w = (-e[:, None, R:P - R, R:P - R] / (3.0 * M))
    dx = _full(w * f_mu, g) + 2 * x * _full(w * f_xx, g) + y * _full(w * f_xy, g)
    return value, dx.transpose(0, 2, 3, 1).reshape(-1, 3)


def roughness_term(rough, normal, m, r_patch):
    """rough [n] or [n, 1], normal [n, 3], m [n] bool -> (value, d / d rough [n])"""
    k = 4 * r_patch * r_patch
    a = m.reshape(-1, k).all(axis=1)
    mc = int(a.sum())
    r = rough.astype(np.float64).reshape(-1, k)
    if mc == 0:
        return 0.0, np.zeros(r.size)
    nv = normal.astype(np.float64).reshape(-1, k, 3).var(axis=1, ddof=1).mean(axis=1)
    value = (a * r.var(axis=1, ddof=1) * (4 - nv)).sum() / mc
    dr = (a * (4 - nv))[:, None] * 2 * (r - r.mean(axis=1, keepdims=True)) / (k - 1) / mc
    return value, dr.reshape(-1)


def patch_terms(idr, sg, gt, net, obj, rough, normal, r_patch, weights):
    """-> terms [4] = (weighted sum, idr_ssim, sg_ssim, roughnesssmooth) and d (weighted sum) / d (idr, sg, rough)"""
    wi, ws, wr = (float(w) for w in weights)
    m = net & obj
    n = idr.shape[0]
    vi = vs = vr = 0.0
    gi, gs, gr = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    if r_patch >= 1 and (wi != 0 or ws != 0):
        vi, gi = ssim_term(idr, gt, m, r_patch)
        vs, gs = ssim_term(sg, gt, m, r_patch)
    if r_patch >= 1 and wr != 0:
        vr, gr = roughness_term(rough, normal, m, r_patch)
    return np.array([wi * vi + ws * vs + wr * vr, vi, vs, vr]), wi * gi, ws * gs, wr * gr


class Golden:
    """tests/golden/patch_loss.npz, read once; case(i) -> dict of that case's arrays"""

    def __init__(self):
        z = np.load(GOLDEN)
        self.names = [str(s) for s in z['names']]
        self.loss_keys = [str(s) for s in z['loss_keys']]
        self.window = z['window']
        assert self.window.dtype == np.float32 and self.window.shape == (WIN,)
        self.cases = []
        for i in range(len(self.names)):
            pre = 'c%d_' % i
            self.cases.append({k[len(pre):]: z[k] for k in z.files if k.startswith(pre)})
        # a single scalar can match by chance: the scalar bound is the largest yardstick of the file
        self.scalar_yard = max(float(np.abs(c['terms32'] - c['terms64']).max()) for c in self.cases)


_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = Golden()
    return _golden


MARGIN = 8.0        # the yardstick is one sample of fp32 rounding; a different summation order moves it by a small factor


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def check_against_golden(case, terms, g_idr, g_sg, g_rough, what=''):
    """terms [4] and the three gradients against the reference's fp64 values, within MARGIN x the reference's own fp32 error.
    Prints every figure before it asserts.  Where the reference's gradient is zero the result must be zero too."""
    G = golden()
    bound = MARGIN * G.scalar_yard
    err = np.abs(np.asarray(terms, np.float64) - case['terms64'])
    print(what, 'scalar errors', err, 'bound', bound)
    fails = []
    if not (err <= bound).all():
        fails.append(('scalars', err.tolist(), bound))
    for name, got, yard in zip(('idr', 'sg', 'rough'), (g_idr, g_sg, g_rough), case['g_yard']):
        want = case['g_' + name].reshape(-1)
        got = np.asarray(got, np.float64).reshape(-1)
        if not want.any():
            print(what, name, 'gradient: reference is zero, largest |got|', np.abs(got).max())
            if got.any():
                fails.append((name, 'non-zero where the reference is zero'))
            continue
        e = rel_l2(got, want)
        print(what, name, 'gradient rel L2', e, 'yardstick', yard, 'bound', MARGIN * yard)
        if not e <= MARGIN * yard:
            fails.append((name, e, MARGIN * yard))
    assert not fails, fails
