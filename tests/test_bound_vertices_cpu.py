"""Bounds from a cell's corners for the SDF interval grid, restated in torch and held to the full searches on the CPU
(csrc/nefii_sdf.hip: grid_cells_kernel's cell_l, grid_vertex_half_kernel; csrc/nefii_tracer.hip: grid_corner_bounds, the second pass of
begin_grid_bracket, grid_audit; tests/test_gpu_bound_vertices.py holds the kernels to this restatement).  The cell intervals,
their walk and the fields are tests/test_bound_grid_cpu.py's.

Beside the cells the build keeps, both as fp16,
  g16 = g at the (G+1)^3 vertices, rounded to nearest: |g - g16| <= e(g16) = 2^-11 |g16| + 2^-25 (half a step of a normal
        fp16, half the subnormal step),
  l16 = the slope bound of the G^3 cells, rounded up: L_c = max(L_floor, safety x sqrt(mx^2 + my^2 + mz^2)), m_a = s_a + (u_a - d_a),
        u_a / d_a the largest / least SIGNED finite-difference slope over the edges ALONG AXIS a of the 3x3x3 block of cells
        around the cell and s_a = max(|u_a|, |d_a|).  (L_cell of the cell intervals is safety x the largest s_a.  Differences along
        the axes measure the gradient's components, and its norm is up to sqrt(3) times the largest of them - more than the
        safety of 1.5 covers; and a difference is the mean slope over its edge: how far the slope inside may lie above it is
        measured by how much the means of neighbouring edges differ, u_a - d_a.  The cell interval's slack carries the corner
        spread beside it and has held; a bound that leans on the slope alone does not: with L_cell the golden net's corner
        bounds miss 8 of the 100 000 exact values below, by up to 4.5e-3, and without u_a - d_a the bounds miss inside a steep
        pocket little wider than a cell - tests/test_gpu_bound_vertices.py's dent.)
A point p of cell c, with the cell's 8 corners x_k and d_k = |p - x_k| + 1e-6 (the 1e-6: the rounding of p and x_k), has
  lo(p) = max_k (g16_k - e_k - l16_c d_k) - tau,      hi(p) = min_k (g16_k + e_k + l16_c d_k) + tau
- the measured quantities and the slope claim of the cell's interval, without its spread over the corners and with the
distance to each corner instead of the largest distance to the nearest.  Outside the cube: no bound.

The walk has two levels.  First test_bound_grid_cpu.bracket_walk on the cell intervals, one look-up per sample.  Then the
samples it keeps - the only ones whose bounds can still move j1, the least hi, the limit or the last sample - get
lo = max(lo_cell, lo_corner), hi = min(hi_cell, hi_corner), and bracket_walk decides once more on those.  lo only rises and hi only
falls, so j1 moves forward, the limit and the last sample fall and the survivors are a subset of the first level's.
The audit holds every evaluated sample against the combined interval."""
import numpy as np
import torch
import torch.nn.functional as F

import test_bound_grid_cpu as cells

NS, TAU, INF = cells.NS, cells.TAU, cells.INF
DIST_EPS = 1e-6


def encode_vertices(g):
    """float32 vertex values -> fp16, to nearest"""
    return g.half()


def vertex_error(g16):
    """what the rounding to fp16 can have moved a vertex value by (float32 arithmetic, as the kernel's)"""
    return g16.float().abs() * 2.0 ** -11 + 2.0 ** -25


def encode_slopes(lcell):
    return cells.fp16_toward(lcell, True)


def sqrt32(x):
    """float32 square root, correctly rounded as the kernel's sqrtf is (torch's own float32 sqrt is not on every CPU; a float64
    root rounded to float32 is: 53 bits are more than twice 24 plus 2)"""
    return torch.sqrt(x.double()).float()


def corner_slopes(g, radius, l_floor, safety=cells.SAFETY):
    """g [(G+1)]^3 float32 -> L_c float32 [G, G, G] (the operands rounded where the kernel rounds them, as build_cells')"""
    G = g.shape[0] - 1
    h = float(np.float32(2.0 * radius / G))
    sq = None
    for ax in range(3):
        s = (g.narrow(ax, 1, G) - g.narrow(ax, 0, G)) / h                 # signed
        k = [4, 4, 4]
        k[ax] = 3
        up = F.max_pool3d(s[None, None], tuple(k), 1, padding=1)[0, 0]
        dn = -F.max_pool3d(-s[None, None], tuple(k), 1, padding=1)[0, 0]
        m = torch.maximum(up.abs(), dn.abs()) + (up - dn)
        sq = m * m if sq is None else sq + m * m
    return torch.clamp(safety * sqrt32(sq), min=l_floor)


def build(g, radius, tau, l_floor, safety=cells.SAFETY):
    """g [(G+1)]^3 float32 -> (lo, hi) fp16 [G, G, G] (build_cells'), g16 fp16 [(G+1)]^3, l16 fp16 [G, G, G]"""
    lo, hi, lcell = cells.build_cells(g, radius, tau, l_floor, safety)
    lc = corner_slopes(g, radius, l_floor, safety)
    assert (lc >= lcell).all()
    return lo, hi, encode_vertices(g), encode_slopes(lc)


def corner_gather(g16, l16, pts, radius, tau):
    """per point [..., 3]: (lo, hi) float32 from the corners of its cell; (-inf, +inf) outside the cube"""
    G = l16.shape[0]
    V = G + 1
    p = pts.float()
    h = torch.tensor(2.0 * radius / G, dtype=torch.float32, device=p.device)
    c = torch.floor((p + radius) * (G / (2.0 * radius))).long()
    inside = ((c >= 0) & (c < G)).all(-1)
    c = c.clamp(0, G - 1)
    L = l16.reshape(-1)[(c[..., 0] * G + c[..., 1]) * G + c[..., 2]].float()
    gv = g16.reshape(-1)
    lo = torch.full(p.shape[:-1], -INF, device=p.device)
    hi = torch.full(p.shape[:-1], INF, device=p.device)
    e2 = [((p - (-radius + (c + a).float() * h)) ** 2) for a in (0, 1)]      # squared offsets per axis to the low / high corner
    for k in range(8):
        a, b, d = k >> 2, (k >> 1) & 1, k & 1
        v = gv[((c[..., 0] + a) * V + c[..., 1] + b) * V + c[..., 2] + d].float()
        dist = sqrt32(e2[a][..., 0] + e2[b][..., 1] + e2[d][..., 2]) + DIST_EPS
        reach = L * dist + vertex_error(v)
        lo = torch.maximum(lo, v - reach)
        hi = torch.minimum(hi, v + reach)
    lo, hi = lo - tau, hi + tau
    return torch.where(inside, lo, torch.full_like(lo, -INF)), torch.where(inside, hi, torch.full_like(hi, INF))


def combine(lo_cell, hi_cell, lo_c, hi_c, which=None):
    """the combined interval of the samples in `which` (None: all), the cell's own for the others"""
    lo, hi = torch.maximum(lo_cell, lo_c), torch.minimum(hi_cell, hi_c)
    if which is None:
        return lo, hi
    return torch.where(which, lo, lo_cell), torch.where(which, hi, hi_cell)


def minsdf_walk(lo_cell, hi_cell, lo_c, hi_c, tau):
    """the same two levels for a min-SDF search (tools/bound_vertices_model.py reports it; the tracer does not run it)"""
    first = cells.minsdf_walk(lo_cell, hi_cell, tau)
    lo, hi = combine(lo_cell, hi_cell, lo_c, hi_c, first)
    return cells.minsdf_walk(lo, hi, tau), first


def bracket_walk(lo_cell, hi_cell, lo_c, hi_c, obj, miss_argmin, tau):
    """-> (keep of the two-level walk, keep of the cell intervals alone, corner look-ups per search)"""
    first = cells.bracket_walk(lo_cell, hi_cell, obj, miss_argmin, tau)
    lo, hi = combine(lo_cell, hi_cell, lo_c, hi_c, first)
    return cells.bracket_walk(lo, hi, obj, miss_argmin, tau), first, first.sum(1)


# ---- the checks -------------------------------------------------------------------------------------------------------

_BUILT = {}


def _built(i, G=64):
    if i not in _BUILT:
        what, sdf, lip = cells._field(i)
        g = sdf(cells.grid_vertices(G, 1.0)).reshape(G + 1, G + 1, G + 1)
        _BUILT[i] = (what, sdf, g) + build(g, 1.0, TAU, cells.L_FLOOR)
    return _BUILT[i]


def test_fp16_encodings_are_outward_safe():
    g = torch.Generator().manual_seed(11)
    x = torch.cat([torch.randn(8192, generator=g) * 0.3, torch.randn(4096, generator=g) * 1e-6, torch.randn(4096, generator=g) * 3e-8,
                   torch.tensor([0.0, -0.0, 1e-9, -1e-9, 2.0 ** -25, -2.0 ** -25, 2.0 ** -24, 5.96e-8, 6.1e-5, -6.1e-5, 6.10352e-5,
                                 0.5, -0.5, 1.0, 1.7320508, 1.0 - 2.0 ** -12, 0.1])])
    g16 = encode_vertices(x)
    err = (g16.double() - x.double()).abs()
    assert (err <= vertex_error(g16).double()).all(), float((err - vertex_error(g16).double()).max())
    # ... and the allowance is no more than a step of the format
    assert (vertex_error(g16) <= 2.0 ** -10 * g16.float().abs().clamp(min=2.0 ** -14)).all()
    lc = x.abs() * 20.0 + 1e-8
    l16 = encode_slopes(lc).float()
    assert (l16 >= lc).all() and (l16 - lc <= 2.0 ** -10 * lc.clamp(min=2.0 ** -14)).all()


def _check_field(i):
    what, sdf, g, lo, hi, g16, l16 = _built(i)
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(100000, 3, generator=gen) * 2.0 - 1.0
    v = sdf(x)
    lo_cell, hi_cell = cells.gather(lo, hi, x, 1.0)
    lo_c, hi_c = corner_gather(g16, l16, x, 1.0, TAU)
    lo_s, hi_s = combine(lo_cell, hi_cell, lo_c, hi_c)
    assert (lo_s <= v).all() and (v <= hi_s).all(), (what, float((lo_s - v).max()), float((v - hi_s).max()))
    assert (lo_c <= v).all() and (v <= hi_c).all(), what
    print('[bound vertices, %s] G 64: mean half-width cells %.4f, corners %.4f, combined %.4f; tightest margins lo %.2e, hi %.2e' % (
        what, float((hi_cell - lo_cell).mean() / 2), float((hi_c - lo_c).mean() / 2), float((hi_s - lo_s).mean() / 2),
        float((v - lo_s).min()), float((hi_s - v).min())))
    assert (hi_s - lo_s).mean() < (hi_cell - lo_cell).mean(), what
    # the searches
    o, d, t0, t1 = cells._rays()
    pts, v = cells._rows(sdf, o, d, t0, t1, torch.linspace(0, 1, NS))
    lo_cell, hi_cell = cells.gather(lo, hi, pts, 1.0)
    lo_c, hi_c = corner_gather(g16, l16, pts, 1.0, TAU)
    lo_s, hi_s = combine(lo_cell, hi_cell, lo_c, hi_c)
    assert (lo_s <= v).all() and (v <= hi_s).all(), what
    report = []
    for obj_all in (True, False):
        obj = torch.full((v.shape[0],), obj_all)
        for miss_argmin in (True, False):
            keep, first, lookups = bracket_walk(lo_cell, hi_cell, lo_c, hi_c, obj, miss_argmin, TAU)
            case = (what, obj_all, miss_argmin)
            assert not (keep & ~first).any(), case + ('a survivor the cell intervals had skipped',)
            masked = torch.where(keep, v, torch.full_like(v, INF))
            ind, amin = cells.decide_bracket(v)
            ind_g, amin_g = cells.decide_bracket(masked)
            assert (ind == ind_g).all(), case
            has = ind >= 0
            im = torch.where(ind > 0, ind - 1, torch.full_like(ind, NS - 1))
            r = torch.arange(v.shape[0])
            assert ((v[r, im] > 0) == (masked[r, im] > 0))[has].all(), case + ('bracket partner',)
            reads = ~(obj & has) if miss_argmin else torch.zeros_like(has)
            assert (amin == amin_g)[reads].all(), case + ('argmin',)
            assert cells.audit(v, keep, lo_s, hi_s, TAU) == 0.0, case
            e0, e1 = cells.evaluations(first).float().mean(), cells.evaluations(keep).float().mean()
            assert (cells.evaluations(keep) <= cells.evaluations(first)).all(), case
            assert e1 < e0, case + (float(e0), float(e1))
            report.append('%s%s %.1f -> %.1f (%.1f corner look-ups)' % ('in-mask' if obj_all else 'out-of-mask', '' if miss_argmin else ' unread',
                                                                         e0, e1, lookups.float().mean()))
    print('[bound vertices, %s] G 64, %d searches: evaluations per search of %d, cells -> cells + corners: %s' % (
        what, v.shape[0], NS, '; '.join(report)))
    # an understated slope bound: the audit must see it through the combined interval too
    lo_u, hi_u, g16_u, l16_u = build(g, 1.0, 0.0, 0.02, safety=0.02)
    a, b = cells.gather(lo_u, hi_u, pts, 1.0)
    lo_s, hi_s = combine(a, b, *corner_gather(g16_u, l16_u, pts, 1.0, 0.0))
    assert cells.audit(v, torch.ones_like(v, dtype=torch.bool), lo_s, hi_s, 0.0) > 0.0, what


def test_bound_vertices_on_union_of_spheres():
    _check_field(0)


def test_bound_vertices_on_golden_net():
    _check_field(1)


def test_outside_the_cube_has_no_bound():
    g16 = torch.full((5, 5, 5), 0.5).half()
    l16 = torch.ones(4, 4, 4).half()
    x = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-1.0000001, 0.2, 0.2], [0.999999, 0.999999, -1.0]])
    lo_c, hi_c = corner_gather(g16, l16, x, 1.0, TAU)
    assert lo_c[1] == -INF and hi_c[1] == INF and lo_c[2] == -INF and hi_c[2] == INF
    assert torch.isfinite(lo_c[[0, 3]]).all() and torch.isfinite(hi_c[[0, 3]]).all()
    # at a vertex the bound is the vertex's own: value -+ (rounding allowance + L 1e-6 + tau)
    assert abs(float(lo_c[0]) - (0.5 - TAU)) < 3e-4 and abs(float(hi_c[0]) - (0.5 + TAU)) < 3e-4
    lo_cell, hi_cell = cells.gather(torch.full((4, 4, 4), 0.4).half(), torch.full((4, 4, 4), 0.6).half(), x, 1.0)
    keep, first, _ = bracket_walk(lo_cell[None], hi_cell[None], lo_c[None], hi_c[None], torch.ones(1, dtype=torch.bool), True, TAU)
    assert keep[0, 1] and keep[0, 2]
