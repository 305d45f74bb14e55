"""fp64 yardstick of the SG shading tests (tests/test_gpu_shading.py, tests/test_oracle_golden.py, make_golden.py).

The reference for every kernel output is oracle/shading.py run in float64 on the fp32 inputs the kernel saw.  The same
oracle run in float32 measures how well the computation is conditioned at those inputs, and sets the bound:

    err(gpu, fp64) <= min(cap, max(factor * err(fp32 oracle, fp64), floor))

so the bound is tight where the maths is well conditioned and honest where fp32 itself loses digits, and a hard cap
no conditioning argument can widen.  Errors are computed in double.  Where a ratio is ill-conditioned per element
(the GGX pdf near n.h = 1) quantiles of the pointwise relative error are judged the same way.  Clamp gates
(max(sum, 0)) that come out differently on the two sides are counted explicitly by `gate_flips`, capped by the caller,
and taken out of the gradient comparison by zeroing their upstream gradient on both sides.

Also here: the inputs the tests share - edge geometry, and lights of any lobe count (synthetic, fitted, adversarial)."""
import math

import numpy as np
import torch

FLOOR_VALUE, FLOOR_GRAD, CAP, FACTOR = 2e-6, 2e-5, 5e-4, 4.0


def rel_l2_64(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def rel_err_64(a, b, tiny=1e-30):
    """pointwise relative error in double"""
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return (a - b).abs() / (b.abs() + tiny)


class Judge:
    """Collects every comparison of one test, prints the table and fails once at the end with every bound that does
    not hold (so one run shows all figures)."""

    def __init__(self, what):
        self.what, self.rows, self.bad = what, [], []

    def close(self, name, got, ref64, ref32, floor=FLOOR_VALUE, cap=CAP, factor=FACTOR):
        e, e32 = rel_l2_64(got, ref64), rel_l2_64(ref32, ref64)
        bound = min(cap, max(factor * e32, floor))
        self._row(name, 'rel_l2', e, e32, bound)

    def quantiles(self, name, got, ref64, ref32, qs=((0.5, 2e-6, 1e-4), (0.99, 2e-4, 2e-3)), factor=FACTOR):
        """qs: (quantile, floor, cap) of the pointwise relative error"""
        r, r32 = rel_err_64(got, ref64), rel_err_64(ref32, ref64)
        for q, floor, cap in qs:
            e, e32 = r.quantile(q).item(), r32.quantile(q).item()
            self._row(name, 'q%g' % q, e, e32, min(cap, max(factor * e32, floor)))

    def require(self, name, ok, info):
        self.rows.append('%-34s %s' % (name, info))
        if not ok:
            self.bad.append('%s: %s' % (name, info))

    def _row(self, name, kind, e, e32, bound):
        ok = e <= bound          # NaN fails
        self.rows.append('%-34s %-7s gpu %.3e  fp32-oracle %.3e  bound %.3e %s' % (name, kind, e, e32, bound,
                                                                                    '' if ok else '  <-- FAIL'))
        if not ok:
            self.bad.append('%s %s: %.3e > %.3e (fp32 oracle %.3e)' % (name, kind, e, bound, e32))

    def done(self):
        print('\n[%s]\n  ' % self.what + '\n  '.join(self.rows))
        assert not self.bad, '%s: %s' % (self.what, '; '.join(self.bad))


def gate_flips(got, ref64):
    """elements where a clamp gate max(x, 0) opened on one side and not on the other"""
    return (got.detach().cpu() > 0) != (ref64.detach().cpu() > 0)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def edge_geometry(n, seed):
    """normal / view [n, 3] float32 (unit): random front-facing points plus, cycled in at the front, the cases where
    the shading kernels branch or lose digits - view == normal, exactly grazing (v.n = 0), barely front- and
    back-facing, fully back-facing, n.x > 0.9 (to_world's other up vector), axis-aligned normals."""
    g = torch.Generator().manual_seed(seed)
    nrm = _unit(torch.randn(n, 3, generator=g, dtype=torch.float64))
    view = _unit(nrm + 0.8 * torch.randn(n, 3, generator=g, dtype=torch.float64))
    s = 1 / math.sqrt(2.)
    edge = [
        ((0., 0., 1.), (0., 0., 1.)),                 # view == normal
        ((0.6, 0., 0.8), (0.6, 0., 0.8)),
        ((0., 0., 1.), (1., 0., 0.)),                 # exactly grazing: vn = 0 -> w_lam = b_lam / 1e-6
        ((0., 1., 0.), (s, 0., s)),                   # grazing, off-axis
        ((0., 0., 1.), (1., 0., 1e-4)),               # barely front-facing
        ((0., 0., 1.), (1., 0., -1e-4)),              # barely back-facing
        ((0., 0., 1.), (0.3, 0.2, -0.9)),             # back-facing
        ((1., 0., 0.), (0.2, 0.4, 0.9)),              # n.x = 1 > 0.9
        ((0.95, 0.3, 0.), (0.9, -0.1, 0.4)),          # n.x > 0.9
        ((0.901, 0.433, 0.02), (0.5, 0.5, 0.7)),
        ((-1., 0., 0.), (-0.6, 0.8, 0.)),
        ((0., -1., 0.), (0.1, -0.99, 0.1)),
    ]
    for i in range(min(n, len(edge))):
        nrm[i] = _unit(torch.tensor(edge[i][0], dtype=torch.float64))
        view[i] = _unit(torch.tensor(edge[i][1], dtype=torch.float64))
    return nrm.float(), view.float()


def synthetic_light(M, seed=3):
    """the synthetic initial light of nefii_amd.synthetic for M lobes (fibonacci axes, lambda 20..~300, mu > 0)"""
    g = np.random.default_rng(seed)
    lgt = g.normal(size=(M, 7))
    lgt[:, -2:] = lgt[:, -3:-2]
    lgt[:, 3:4] = 20. + np.abs(lgt[:, 3:4] * 100.)
    energy = np.abs(lgt[:, 4:]) * 2.0 * math.pi / lgt[:, 3:4] * (1.0 - np.exp(-2.0 * lgt[:, 3:4]))
    lgt[:, 4:] = np.abs(lgt[:, 4:]) / energy.sum(0, keepdims=True) * 2. * math.pi
    from nefii_amd.synthetic import fibonacci_sphere
    lgt[:, :3] = fibonacci_sphere(M) if M > 1 else (0., 0., 1.)      # (fibonacci_sphere(1) divides by 0)
    return torch.from_numpy(lgt).float()


def adversarial_light(M, seed=11):
    """M lobes with what fitted lights bring and the initial light never has: negative lambda and mu, exact zeros in
    mu (the sign(0) = 0 gradient paths), unnormalised axes of length 1e-3 and 50, sharpness from 0.5 to
    ~1200 (the sharpest lobe of a shipped fit is 1222).  No lambda is 0: the closed form divides by it (the reference
    gives NaN there too)"""
    g = torch.Generator().manual_seed(seed)
    lgt = torch.empty(M, 7, dtype=torch.float64)
    lgt[:, :3] = _unit(torch.randn(M, 3, generator=g, dtype=torch.float64))
    scale = torch.tensor([1., 1e-3, 50., 1., 3.], dtype=torch.float64)
    lgt[:, :3] *= scale[torch.arange(M) % 5].reshape(-1, 1)
    lam = torch.exp(torch.empty(M, dtype=torch.float64).uniform_(math.log(0.5), math.log(1200.), generator=g))
    sgn = torch.where(torch.rand(M, generator=g, dtype=torch.float64) < 0.3, -1., 1.)
    lgt[:, 3] = lam * sgn
    mu = torch.rand(M, 3, generator=g, dtype=torch.float64) * 2. / math.sqrt(M)
    mu = torch.where(torch.rand(M, 3, generator=g, dtype=torch.float64) < 0.3, -mu, mu)
    lgt[:, 4:] = mu
    lgt[1::7, 4] = 0.
    lgt[2::11, 4:] = 0.
    return lgt.float()


def tile_light(lgt, M):
    """the first M lobes of lgt repeated (a fitted light of another lobe count, with the same statistics)"""
    reps = (M + lgt.shape[0] - 1) // lgt.shape[0]
    return lgt.repeat(reps, 1)[:M].contiguous()
