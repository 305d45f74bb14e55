"""The SDF interval grid for the tracer's staged searches under frozen geometry, restated in torch and held to the full
searches on the CPU (csrc/nefii_sdf.hip: grid_cells_kernel; csrc/nefii_tracer.hip: begin_grid_bracket, grid_audit; tests/test_gpu_bound_grid.py holds
the kernels to this restatement).  tools/bound_grid_model.py runs the same rule on a bench workload's own rays; the tracer reads
the grid for the bracket searches of eval-mode traces only - profiles/bound_grid/README.md has the prediction that decided that.

The grid: the cube [-radius, radius]^3 cut into G^3 cells of edge h = 2 radius / G; g = the single-pass SDF at the (G+1)^3
vertices (|g - sdf| <= tau).  Per cell, two fp16:
  lo = min_k g_k - tau - L_cell h sqrt(3)/2   (rounded down),      hi = max_k g_k + tau + L_cell h sqrt(3)/2   (rounded up),
  L_cell = max(L_floor, safety x the largest finite-difference slope over the edges of the 3x3x3 block of cells around it)
(k: the cell's 8 corners; every point of a cell lies within h sqrt(3)/2 of its nearest corner).  A point outside the cube has
no bound: lo = -inf, hi = +inf, and its sample is evaluated.

The walk: a search that would evaluate a first stage of its own (a quarter of its samples) reads (lo_i, hi_i) of the cells
its ns samples fall into instead, and evaluates only the samples the bounds do not decide:
  bracket search (first negative sample `ind`, its bracket (ind - 1, ind), the argmin where somebody reads it):
    j1 = the first sample with hi < -tau (surely negative); front_only = in the object mask, j1 exists, lo_0 > 0 - the
    search ends at or before j1 and only signs matter: samples behind j1 are not needed, one in front is skipped when
    lo > 0.  Sign-only searches without j1 (nobody reads the argmin: unread misses) skip on lo > 0 over the whole row;
    the others skip on lo > max(0, min_i hi_i + tau): positive and not the argmin.
  min-SDF search (the argmin): skipped when lo > min_i hi_i + tau.
  (Comparisons carry the tracer's 1e-6, as staged_walk's.)  A skipped sample reads +inf: positive, never a minimum.
  More than CREF_CAP survivors: the whole row, as today.  One skipped sample per search is evaluated after all (the probe).
The audit: every evaluated sample is held against both ends of its cell's interval, max(lo - tau - v, v - hi - tau) over
the evaluated samples; positive = a bound that did not hold where it could be checked."""
import numpy as np
import torch
import torch.nn.functional as F

from nefii_amd import ops, synthetic as syn
from oracle import nets

import test_minsdf_share_cpu as share

NS = 100
TAU = share.TAU
CREF_CAP = 76          # csrc/nefii_tracer.hip
L_FLOOR = 1.0
SAFETY = 1.5           # ops.LIPSCHITZ_SAFETY: finite differences over an edge understate the steepest slope along it
INF = float('inf')


def fp16_toward(x, up):
    """x (float32) -> the nearest fp16 that is >= x (up) or <= x (down); finite inputs within the fp16 range"""
    hv = x.half()
    wrong = (hv.float() < x) if up else (hv.float() > x)
    bits = hv.view(torch.int16).clone()
    # one ulp away from zero when the move and the sign agree, towards zero otherwise; zero steps to the smallest subnormal
    pos = bits >= 0           # (sign bit clear: +0 and positives)
    mag = bits & 0x7FFF
    away = pos if up else ~pos
    stepped = torch.where(away, bits + 1, bits - 1)
    zero = mag == 0
    stepped = torch.where(zero, torch.full_like(bits, 0x0001 if up else -0x7FFF), stepped)      # (-0x7FFF = 0x8001)
    return torch.where(wrong, stepped, bits).view(torch.float16)


def grid_vertices(G, radius, device='cpu'):
    """[(G+1)^3, 3] float32, x slowest: vertex (i, j, k) = -radius + (i, j, k) h"""
    a = -radius + torch.arange(G + 1, device=device, dtype=torch.float32) * (2.0 * radius / G)
    return torch.stack(torch.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3)


def build_cells(g, radius, tau, l_floor, safety=SAFETY):
    """g [(G+1)]^3 float32 vertex values -> (lo, hi) fp16 [G, G, G], L_cell float32 [G, G, G]"""
    G = g.shape[0] - 1
    h = float(np.float32(2.0 * radius / G))                 # (the kernel's operands, rounded where it rounds them)
    reach = float(np.float32(h * 0.8660254037844386))       # h sqrt(3) / 2
    x = g[None, None]
    cmin = -F.max_pool3d(-x, 2, 1)[0, 0]
    cmax = F.max_pool3d(x, 2, 1)[0, 0]
    slope = None
    for ax in range(3):
        s = (g.narrow(ax, 1, G) - g.narrow(ax, 0, G)).abs() / h          # edges along ax: G x (G+1) x (G+1), permuted
        k = [4, 4, 4]
        k[ax] = 3       # edges ax-1 .. ax+1 of the block's 4 x 4 vertex columns across
        m = F.max_pool3d(s[None, None], tuple(k), 1, padding=1)[0, 0]
        slope = m if slope is None else torch.maximum(slope, m)
    lcell = torch.clamp(safety * slope, min=l_floor)
    slack = tau + lcell * reach
    return fp16_toward(cmin - slack, False), fp16_toward(cmax + slack, True), lcell


def gather(lo, hi, pts, radius):
    """per point [..., 3]: (lo, hi) float32 of its cell; (-inf, +inf) outside the cube"""
    G = lo.shape[0]
    c = torch.floor((pts.float() + radius) * (G / (2.0 * radius))).long()
    inside = ((c >= 0) & (c < G)).all(-1)
    c = c.clamp(0, G - 1)
    flat = (c[..., 0] * G + c[..., 1]) * G + c[..., 2]
    lo_s = torch.where(inside, lo.reshape(-1)[flat].float(), torch.full_like(flat, -INF, dtype=torch.float32))
    hi_s = torch.where(inside, hi.reshape(-1)[flat].float(), torch.full_like(flat, INF, dtype=torch.float32))
    return lo_s, hi_s


def _first(mask):
    """first True per row, the row's length where there is none"""
    ns = mask.shape[1]
    idx = torch.arange(ns, device=mask.device).expand_as(mask)
    return torch.where(mask, idx, torch.full_like(idx, ns)).min(1).values


def bracket_walk(lo, hi, obj, miss_argmin, tau):
    """lo, hi [n, ns]; obj bool [n] -> keep bool [n, ns]: the samples a bracket search evaluates"""
    ns = lo.shape[1]
    idx = torch.arange(ns, device=lo.device).expand_as(lo)
    j1 = _first(hi < -tau)
    front_only = obj & (j1 < ns) & (lo[:, 0] > 0)
    sign_only = front_only | (not miss_argmin)
    lim = torch.where(sign_only, torch.zeros_like(j1, dtype=lo.dtype), torch.clamp(hi.min(1).values + tau, min=0.0))
    last = torch.where(front_only, j1, torch.full_like(j1, ns - 1))
    return ~(lo - 1e-6 > lim[:, None]) & (idx <= last[:, None])


def minsdf_walk(lo, hi, tau):
    return ~(lo - 1e-6 > (hi.min(1).values + tau)[:, None])


def evaluations(keep):
    """single-pass evaluations per search: survivors, one probe when anything was skipped; past CREF_CAP the whole row"""
    ns = keep.shape[1]
    k = keep.sum(1)
    k = k + (k < ns).long()
    return torch.where(k > CREF_CAP, torch.full_like(k, ns), k)


def decide_bracket(v):
    """sampler_exact's reading of a row: (first negative sample or -1, argmin)"""
    ns = v.shape[1]
    ind = _first(v < 0)
    return torch.where(ind < ns, ind, torch.full_like(ind, -1)), v.argmin(1)


def audit(v, keep, lo, hi, tau):
    bad = torch.maximum(lo - tau - v, v - hi - tau)
    return float(torch.where(keep, bad, torch.full_like(bad, -INF)).max().clamp(min=0.0))


def staged_today(v, depth, llen, lim_of, last=None, tau=TAU):
    """The evaluated first stage the grid replaces (staged_walk with the global slope bound), rows already in SORTED order of
    depth [n, ns]: -> keep.  lim_of(best) -> the search's limit from the lowest first-stage value; last [n]: samples behind it
    are not needed (None: all are)."""
    n, ns = v.shape
    pos = share.stage1_pos(ns)
    keep = torch.zeros_like(v, dtype=torch.bool)
    keep[:, pos] = True
    lim = lim_of(v[:, pos].min(1).values)
    for ja in range(len(pos) - 1):
        a, b = pos[ja], pos[ja + 1]
        for kk in range(a + 1, b):
            lb = torch.maximum(v[:, a] - llen * (depth[:, kk] - depth[:, a]), v[:, b] - llen * (depth[:, b] - depth[:, kk])) - tau
            keep[:, kk] = ~(lb - 1e-6 > lim)
    if last is not None:
        idx = torch.arange(ns, device=v.device).expand_as(v)
        keep &= (idx <= last[:, None]) | keep.new_tensor([i in pos for i in range(ns)])[None]
    return keep


# ---- the checks -------------------------------------------------------------------------------------------------------

def _spheres(x):
    return torch.from_numpy(share.union_of_spheres(x.double().numpy())).float()


def _field_cases():
    yield 'union of spheres', _spheres, 1.0
    mc = syn.model_conf('physg', hidden=64)
    sd = {k: v.double() for k, v in syn.make_state_dict(mc, seed=0, bumpy=0.03).items()}
    cfg = mc['implicit_network']
    lip = ops.calibrate_lipschitz(lambda x: nets.sdf_gradient(sd, cfg, x.double()), 'cpu')

    def net(x):
        with torch.no_grad():
            return nets.sdf_forward(sd, cfg, x.double())[:, 0].float()
    yield 'tracer_bumpy_h64', net, lip


_FIELDS = {}


def _field(i):
    if not _FIELDS:
        for k, case in enumerate(_field_cases()):
            _FIELDS[k] = case
    return _FIELDS[i]


def _grid(sdf, l_floor, G=64, radius=1.0):
    g = sdf(grid_vertices(G, radius)).reshape(G + 1, G + 1, G + 1)
    return build_cells(g, radius, TAU, l_floor)


def _rays():
    o, d = share.bundles(8, 3)
    t0, t1, ok = share.sphere_stretch(o, d)
    o, d, t0, t1 = (torch.from_numpy(a[ok]).float() for a in (o, d, t0, t1))
    return o, d, t0, t1


def _rows(sdf, o, d, t0, t1, frac):
    t = t0[:, None] + frac[None, :] * (t1 - t0)[:, None]
    pts = o[:, None, :] + t[:, :, None] * d[:, None, :]
    return pts, sdf(pts.reshape(-1, 3)).reshape(pts.shape[:2])


def test_fp16_rounding_is_outward():
    x = torch.cat([torch.randn(4096) * 0.3, torch.tensor([0.0, 1e-9, -1e-9, 0.5, -0.5, 6.1e-5, -6.1e-5])])
    dn, up = fp16_toward(x, False).float(), fp16_toward(x, True).float()
    assert (dn <= x).all() and (up >= x).all()
    assert (up - dn <= 2.0 ** -10 * x.abs().clamp(min=2.0 ** -14)).all()      # at most one fp16 step apart


def _check_field(i):
    what, sdf, lip = _field(i)
    # the floor is a unit slope - what a distance function has - and not the global bound: the steep spots raise L_cell
    # where they are, through the finite differences around the cell
    lo, hi, lcell = _grid(sdf, L_FLOOR)
    assert float(lcell.max()) <= max(L_FLOOR, SAFETY * lip * 1.0001), (what, float(lcell.max()))
    g = torch.Generator().manual_seed(5)
    x = torch.rand(100000, 3, generator=g) * 2.0 - 1.0
    lo_s, hi_s = gather(lo, hi, x, 1.0)
    v = sdf(x)
    assert (lo_s <= v).all() and (v <= hi_s).all(), (what, float((lo_s - v).max()), float((v - hi_s).max()))
    # the searches: the grid's decisions against the full rows'
    o, d, t0, t1 = _rays()
    lin = torch.linspace(0, 1, NS)
    draws = torch.rand(NS, generator=g)
    report = []
    for kind, frac in (('bracket', lin), ('min-sdf', draws)):
        pts, v = _rows(sdf, o, d, t0, t1, frac)
        lo_s, hi_s = gather(lo, hi, pts, 1.0)
        for obj_all in (True, False):
            obj = torch.full((v.shape[0],), obj_all)
            for miss_argmin in (True, False):
                if kind == 'min-sdf':
                    keep = minsdf_walk(lo_s, hi_s, TAU)
                else:
                    keep = bracket_walk(lo_s, hi_s, obj, miss_argmin, TAU)
                masked = torch.where(keep, v, torch.full_like(v, INF))
                ind, amin = decide_bracket(v)
                ind_g, amin_g = decide_bracket(masked)
                if kind == 'min-sdf':
                    assert (amin == amin_g).all(), (what, kind)
                else:
                    assert (ind == ind_g).all(), (what, kind, obj_all, miss_argmin)
                    # the bracket partner's sign (ind - 1; ind = 0 pairs with the last sample)
                    has = ind >= 0
                    im = torch.where(ind > 0, ind - 1, torch.full_like(ind, NS - 1))
                    r = torch.arange(v.shape[0])
                    assert ((v[r, im] > 0) == (masked[r, im] > 0))[has].all(), (what, kind, 'bracket partner')
                    # the argmin is read unless the ray lies inside the mask and has its negative sample
                    reads = ~(obj & has) if miss_argmin else torch.zeros_like(has)
                    assert (amin == amin_g)[reads].all(), (what, kind, obj_all, 'argmin')
                assert audit(v, keep, lo_s, hi_s, TAU) == 0.0
                report.append('%s%s%s %.1f' % (kind, ' in-mask' if obj_all else ' out-of-mask', '' if miss_argmin else ' unread',
                                               evaluations(keep).float().mean()))
    print('[bound grid model, %s] global L %.3f, L_cell %.2f .. %.2f, G 64: evaluations per search of %d: %s' % (
        what, lip, float(lcell.min()), float(lcell.max()), NS, '; '.join(report)))
    assert evaluations(keep).float().mean() < NS
    # an understated slope bound: the audit must see it
    lo_u, hi_u, _ = build_cells(sdf(grid_vertices(64, 1.0)).reshape(65, 65, 65), 1.0, 0.0, 0.02, safety=0.02)
    pts, v = _rows(sdf, o, d, t0, t1, lin)
    lo_s, hi_s = gather(lo_u, hi_u, pts, 1.0)
    assert audit(v, torch.ones_like(v, dtype=torch.bool), lo_s, hi_s, 0.0) > 0.0, what


def test_bound_grid_on_union_of_spheres():
    _check_field(0)


def test_bound_grid_on_golden_net():
    _check_field(1)


def test_outside_the_cube_is_evaluated():
    lo = torch.full((4, 4, 4), 0.5).half()
    hi = torch.full((4, 4, 4), 0.6).half()
    x = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-1.0000001, 0.2, 0.2], [0.999999, 0.999999, -1.0]])
    lo_s, hi_s = gather(lo, hi, x, 1.0)
    assert lo_s.tolist() == [0.5, -INF, -INF, 0.5] and hi_s[1] == INF
    keep = minsdf_walk(lo_s[None], hi_s[None], TAU)
    assert keep[0, 1] and keep[0, 2]
