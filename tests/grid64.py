"""fp64 yardstick of the SDF interval grid (tests/test_grid64_cpu.py, tests/test_gpu_grid_fp64.py): the claim every reader of the
grid rests on - lo <= sdf <= hi over a cell, and the corner bounds of a point - held against the network's SDF in float64, on
points chosen where a bound is tightest.

Reference.  The SDF evaluated in float64 on the fp32 EFFECTIVE weights the kernels pack (trace64.make_net), on the fp32 points.

Look-ups.  The restatements' (test_bound_grid_cpu.gather, test_bound_vertices_cpu.corner_gather): they decide a point's cell in
fp32 as the kernels do, with the radius, the cell edge and tau rounded to fp32 where the library rounds them (`Grid`).

The rules (`judge`), every comparison formed in float64 with ZERO tolerance - tau already pays for the evaluator's error:
  1  |float(vert_g[v]) - sdf64(x_v)| <= tau + 2^-11 |vert_g[v]| + 2^-25 at the grid's vertices, x_v formed as grid_points_kernel
     forms it (fp32 -radius + i h, h rounded to fp32): the tau claim, over the whole cube and not only the ball it is measured in;
  2  lo_cell <= sdf64(p) <= hi_cell;
  3  lo(p) <= sdf64(p) <= hi(p) from the 8 corners of p's cell, and the combined interval (max of the lower, min of the upper ends);
  4  the slope claim rule 3 uses: |sdf64(p) - sdf64(x_k)| <= L_c (|p - x_k| + 1e-6) for the 8 corners x_k of p's cell;
  5  a point inside the cube has a finite interval, a point at or past a face has none.  (The look-up rounds p + radius and its
     product with the cells per unit length to fp32: a point within 4 ulp of the UPPER face may round onto it - 1 - 2^-24 does,
     at radius 1 - and is then evaluated, which is safe.  Such points may go either way and are counted; a bound they do get
     is held to rules 2 and 3 like any other.)
  Printed, not asserted: the least margins of rules 2 to 4, the largest fp64 |grad| of a subsample against the L_c of its cell,
  the mean half-widths.  Tightness needs no assertion: the builds are pinned bit for bit to the restatements elsewhere.

Points (`points`).  Uniform points almost never land where a bound is tightest, so the set holds, per chosen cell, the centre
(farthest from every corner: the cell interval's reach) and a point 0.001 h inside each of the 8 corners (the corner bound rests
on tau alone there); points on the cube's faces, one ulp inside and one ulp past them; and uniform points.  Every cell is
chosen up to G = 64; above, a sample that always holds the 8 corner cells of the cube, cells of the outermost layer (their
3x3x3 block is clipped), the k cells with the steepest slope bound and the k cells with the least |vertex value|.
`search` then walks downhill from the 256 points of least margin, as ops.calibrate_lipschitz does for the gradient."""
import types

import numpy as np
import torch
import torch.nn.functional as F

import test_bound_grid_cpu as cells_model
import test_bound_vertices_cpu as verts_model
import trace64

ALL_CELLS_G = 64          # every cell is sampled up to this size
INF = float('inf')
KINDS = ('centre', 'corner', 'face', 'uniform')


def f32(v):
    return float(np.float32(v))


def sdf64_of(net, chunk=32768):
    """points [n, 3] (any float dtype, any device) -> float64 SDF [n] of trace64.NETS[net], in chunks, without autograd.  The
    values of the last large tensor are kept (by identity: several builds of one net are judged on one point set)."""
    f = trace64.make_net(net)[3]
    last = [None, None]

    def run(x):
        if last[0] is x:
            return last[1]
        xd = x.double()
        if xd.shape[0] == 0:
            return xd.new_zeros(0)
        with torch.no_grad():
            out = torch.cat([f(xd[i:i + chunk]) for i in range(0, xd.shape[0], chunk)])
        if x.shape[0] >= 100000:
            last[0], last[1] = x, out
        return out
    run.raw = f
    return run


def grad64_norm(sdf64, x, chunk=16384):
    """|grad sdf64| at x, by autograd through the float64 network"""
    out = []
    for i in range(0, x.shape[0], chunk):
        with torch.enable_grad():
            xr = x[i:i + chunk].double().detach().clone().requires_grad_(True)
            g = torch.autograd.grad(sdf64.raw(xr).sum(), xr)[0]
        out.append(g.norm(dim=1))
    return torch.cat(out) if out else x.new_zeros(0, dtype=torch.float64)


def unpack(words):
    """build_bound_grid's int32 words -> (lo, hi) fp16"""
    lo = (words & 0xFFFF).to(torch.int16).view(torch.float16)
    hi = ((words >> 16) & 0xFFFF).to(torch.int16).view(torch.float16)
    return lo, hi


class Grid:
    """The arrays of one build and the fp64 SDF they claim to bound.  radius, h and tau are kept as the library rounds them."""

    def __init__(self, sdf64, G, radius, tau, lo, hi, vert_g=None, cell_l=None):
        self.sdf64, self.G, self.V = sdf64, int(G), int(G) + 1
        self.radius, self.tau = f32(radius), f32(tau)
        self.h = f32(2.0 * self.radius / G)
        self.lo, self.hi, self.vert_g, self.cell_l = lo, hi, vert_g, cell_l
        self.device = lo.device
        assert tuple(lo.shape) == (G,) * 3 and lo.dtype == torch.float16 and hi.dtype == torch.float16
        if vert_g is not None:
            assert tuple(vert_g.shape) == (G + 1,) * 3 and tuple(cell_l.shape) == (G,) * 3
        self._table = None

    def vertex_points(self, ids):
        """flat vertex ids -> fp32 positions, as grid_points_kernel forms them"""
        V = self.V
        ijk = torch.stack([ids // (V * V), (ids // V) % V, ids % V], -1)
        return -self.radius + ijk.float() * self.h

    def vertex64(self, ids):
        """fp64 SDF at the vertices `ids` (any shape): from a table of all of them up to ALL_CELLS_G, else at the distinct ones"""
        if self.G <= ALL_CELLS_G:
            if self._table is None:
                self._table = self.sdf64(self.vertex_points(torch.arange(self.V ** 3, device=self.device)))
            return self._table[ids]
        uniq, inv = torch.unique(ids.reshape(-1), return_inverse=True)
        return self.sdf64(self.vertex_points(uniq))[inv].reshape(ids.shape)


def cell_of(x, G, radius):
    """(cell [n, 3] clamped into the grid, inside) - the line of test_bound_grid_cpu.gather that decides it, in fp32"""
    c = torch.floor((x.float() + radius) * (G / (2.0 * radius))).long()
    return c.clamp(0, G - 1), ((c >= 0) & (c < G)).all(-1)


# ---- the points ------------------------------------------------------------------------------------------------------------
def points(G, radius, seed=0, budget=400000, cell_l=None, vert_g=None, k=64, n_uniform=None, n_face=128, device='cpu'):
    """A deterministic fp32 point set for a grid -> namespace(x [n, 3], kind uint8 [n] (index into KINDS), cells [m, 3] the
    chosen cells, strata: name -> rows of `cells`).  cell_l, vert_g (the build's arrays, optional): the steepest and the
    nearest-to-the-surface cells are stratified from them."""
    radius = f32(radius)
    h = 2.0 * radius / G
    gen = torch.Generator().manual_seed(seed)
    n_uniform = min(100000, budget // 4) if n_uniform is None else n_uniform
    strata, chosen = {}, []

    def add(name, c):
        strata[name] = torch.arange(sum(t.shape[0] for t in chosen), sum(t.shape[0] for t in chosen) + c.shape[0])
        chosen.append(c.cpu().long())

    ends = torch.tensor([0, G - 1])
    add('corner_cells', torch.stack(torch.meshgrid(ends, ends, ends, indexing='ij'), -1).reshape(-1, 3))
    unravel = lambda flat: torch.stack([flat // (G * G), (flat // G) % G, flat % G], -1)
    if cell_l is not None:
        add('steepest', unravel(torch.topk(cell_l.reshape(-1).float(), min(k, G ** 3)).indices))
    if vert_g is not None:
        least = -F.max_pool3d(-vert_g.float().abs()[None, None], 2, 1)[0, 0]         # the least |corner value| of each cell
        add('near_surface', unravel(torch.topk(-least.reshape(-1), min(k, G ** 3)).indices))
    if G <= ALL_CELLS_G:
        a = torch.arange(G)
        every = torch.stack(torch.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3)
        outer = ((every == 0) | (every == G - 1)).any(-1)
        add('outer', every[outer])
        add('inner', every[~outer])
    else:
        m = max(budget - n_uniform - 3 * (4 * n_face + 2 * max(n_face // 8, 1)) - 8, 0) // 9
        n_outer = m // 4
        c = torch.randint(0, G, (n_outer, 3), generator=gen)
        ax = torch.randint(0, 3, (n_outer,), generator=gen)
        side = torch.randint(0, 2, (n_outer,), generator=gen) * (G - 1)
        c[torch.arange(n_outer), ax] = side
        add('outer', c)
        add('inner', torch.randint(1, G - 1, (max(m - sum(t.shape[0] for t in chosen), 0), 3), generator=gen))
    cells = torch.cat(chosen)
    # per cell: the centre, and a point 0.001 h inside each of its 8 corners (formed in float64, rounded once)
    base = -radius + cells.double() * h
    per = [base + 0.5 * h]
    for q in range(8):
        off = torch.tensor([q >> 2, (q >> 1) & 1, q & 1], dtype=torch.float64)
        per.append(base + off * h + (1.0 - 2.0 * off) * (0.001 * h))
    cell_pts = torch.stack(per, 1).reshape(-1, 3).float()
    kind = torch.cat([torch.tensor([0] + [1] * 8, dtype=torch.uint8).repeat(cells.shape[0])])
    # the faces: one coordinate ON a face, one ulp inside it and one ulp past it, the others uniform in the cube; and the 8 corners
    r = np.float32(radius)
    special = [float(v) for v in (-r, r, np.nextafter(r, np.float32(0)), np.nextafter(-r, np.float32(0)), np.nextafter(-r, np.float32(-2) * r),
                                  np.nextafter(r, np.float32(2) * r))]
    face = []
    for ax in range(3):
        for v in special[:4]:
            p = (torch.rand(n_face, 3, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * radius
            p[:, ax] = v
            face.append(p)
        for v in special[4:]:
            p = (torch.rand(max(n_face // 8, 1), 3, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * radius
            p[:, ax] = v
            face.append(p)
    cube = torch.tensor([-radius, float(np.nextafter(r, np.float32(0)))], dtype=torch.float64)
    face.append(torch.stack(torch.meshgrid(cube, cube, cube, indexing='ij'), -1).reshape(-1, 3))
    face = torch.cat(face).float()
    uni = ((torch.rand(n_uniform, 3, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * radius).float()
    x = torch.cat([cell_pts, face, uni])
    kind = torch.cat([kind, torch.full((face.shape[0],), 2, dtype=torch.uint8), torch.full((uni.shape[0],), 3, dtype=torch.uint8)])
    return types.SimpleNamespace(x=x.contiguous().to(device), kind=kind.to(device), cells=cells, strata=strata)


def vertex_sample(G, n_random=200000, seed=0):
    """flat ids of the three central vertex planes and n_random random vertices (the sample of rule 1 above ALL_CELLS_G)"""
    V = G + 1
    a = torch.arange(V)
    mid = torch.full((V * V,), V // 2)
    jj, kk = torch.meshgrid(a, a, indexing='ij')
    jj, kk = jj.reshape(-1), kk.reshape(-1)
    planes = [(mid * V + jj) * V + kk, (jj * V + mid) * V + kk, (jj * V + kk) * V + mid]
    rnd = torch.randint(0, V ** 3, (n_random,), generator=torch.Generator().manual_seed(seed))
    return torch.unique(torch.cat(planes + [rnd]))


# ---- the search ------------------------------------------------------------------------------------------------------------
def search(margin_fn, x, h, radius=1.0, seed=0, rounds=3, margins=None):
    """ops.calibrate_lipschitz's scheme, downhill: `rounds` rounds around the 256 points of least margin, 255 Gaussian
    perturbations each with sigma h / 2, halved every round, clamped inside the cube.  margin_fn: fp32 points [n, 3] -> margins
    [n] (margins: those of x, if already known).  -> (the last round's points, their margins)."""
    radius = f32(radius)
    top_face = float(np.nextafter(np.float32(radius), np.float32(0)))
    gen = torch.Generator().manual_seed(seed)
    m = margin_fn(x) if margins is None else margins
    sigma = 0.5 * h
    for _ in range(rounds):
        top = torch.topk(-m, min(256, m.numel())).indices
        seeds, best = x[top], m[top]
        pert = (torch.randn(seeds.shape[0], 255, 3, generator=gen) * sigma).to(x.device)
        cand = (seeds.unsqueeze(1) + pert).reshape(-1, 3).clamp(-radius, top_face).float()
        x = torch.cat([seeds, cand])
        m = torch.cat([best, margin_fn(cand)])
        sigma *= 0.5
    return x, m


# ---- the judge -------------------------------------------------------------------------------------------------------------
def rules_at(grid, x):
    """The margins of rules 2 to 4 (float64, +inf where a point has no bound; negative = violated) and the flags of rule 5 at
    the fp32 points x [n, 3] on the grid's device."""
    G, r, tau = grid.G, grid.radius, grid.tau
    s = grid.sdf64(x)
    lo_c, hi_c = cells_model.gather(grid.lo, grid.hi, x, r)
    out = {'sdf': s, 'lo_cell': lo_c, 'hi_cell': hi_c}
    out['m2'] = torch.minimum(s - lo_c.double(), hi_c.double() - s)
    has = torch.isfinite(lo_c) & torch.isfinite(hi_c)
    nan = torch.isnan(lo_c) | torch.isnan(hi_c)
    c, inside = cell_of(x, G, r)
    if grid.vert_g is not None:
        lo_k, hi_k = verts_model.corner_gather(grid.vert_g, grid.cell_l, x, r, tau)
        lo_b, hi_b = verts_model.combine(lo_c, hi_c, lo_k, hi_k)
        out['m3'] = torch.minimum(s - lo_k.double(), hi_k.double() - s)
        out['m3c'] = torch.minimum(s - lo_b.double(), hi_b.double() - s)
        out['half_corner'], out['half_both'] = (hi_k - lo_k) / 2, (hi_b - lo_b) / 2
        has &= torch.isfinite(lo_k) & torch.isfinite(hi_k)
        nan |= torch.isnan(lo_k) | torch.isnan(hi_k)
        # rule 4, differences in float64
        V = grid.V
        L = grid.cell_l.reshape(-1)[(c[:, 0] * G + c[:, 1]) * G + c[:, 2]].float().double()
        ids = torch.stack([((c[:, 0] + (q >> 2)) * V + c[:, 1] + ((q >> 1) & 1)) * V + c[:, 2] + (q & 1) for q in range(8)], 1)      # [n, 8]
        xk = grid.vertex_points(ids.reshape(-1)).double().reshape(-1, 8, 3)
        dist = (x.double().unsqueeze(1) - xk).norm(dim=-1) + 1e-6
        head = L.unsqueeze(1) * dist - (s.unsqueeze(1) - grid.vertex64(ids)).abs()
        out['m4'] = torch.where(inside, head.min(1).values, torch.full_like(s, INF))
        cover = (L.unsqueeze(1) * dist / (s.unsqueeze(1) - grid.vertex64(ids)).abs().clamp_min(1e-300)).min(1).values
        out['cover'] = torch.where(inside, cover, torch.full_like(s, INF))
        out['L'] = L
    out['half_cell'] = (hi_c - lo_c) / 2
    xf = x.float()
    geo_in = ((xf >= -r) & (xf < r)).all(-1)
    safely_in = geo_in & (xf.max(-1).values <= r * (1.0 - 2.0 ** -21))
    out['inside'], out['has'] = inside, has
    out['bad5'] = (~geo_in & has) | (safely_in & ~has) | nan | (inside != has)
    out['either'] = geo_in & ~safely_in
    m = out['m2']
    for key in ('m3', 'm3c', 'm4'):
        if key in out:
            m = torch.minimum(m, out[key])
    out['margin'] = m
    return out


def judge(what, grid, x, vertex_ids=None, check=True, search_seed=0, rounds=3, grad_sample=50000):
    """Hold a build to rules 1 to 5 on the points x (fp32 [n, 3]) and on what `rounds` rounds of `search` find from them.
    vertex_ids: the vertices of rule 1 (None: all of them).  Prints the figures; check: asserts the hard ones.  -> the figures,
    with figures['violations'][rule] the number of points (vertices) that break a rule."""
    dev = grid.device
    x = x.to(dev).float().contiguous()
    fig = {'violations': {}}
    viol = fig['violations']
    # rule 1
    if grid.vert_g is not None:
        ids = torch.arange(grid.V ** 3, device=dev) if vertex_ids is None else vertex_ids.to(dev)
        xv = grid.vertex_points(ids)
        g = grid.vert_g.reshape(-1)[ids].float().double()
        err = (g - grid.vertex64(ids)).abs()
        allowed = grid.tau + 2.0 ** -11 * g.abs() + 2.0 ** -25
        viol[1] = int((err > allowed).sum())
        ball = xv.double().norm(dim=1) <= grid.radius
        part = lambda msk, t: float(t[msk].max()) if msk.any() else 0.0
        # what is left for tau to cover once the rounding to fp16 is paid for: a lower bound on |single-pass - sdf64| there
        need = (err - (allowed - grid.tau)).clamp_min(0.0)
        fig.update(vertices=int(ids.numel()), err_in=part(ball, err), err_out=part(~ball, err), need_in=part(ball, need),
                   need_out=part(~ball, need), over_in=part(ball, err - allowed), over_out=part(~ball, err - allowed))
        print('[grid64 %s] rule 1, %d vertices: largest |g16 - sdf64| inside the ball %.3e, outside %.3e; left for tau after the fp16 '
              'allowance: inside %.3e, outside %.3e, against tau %.3e; least headroom to tau + 2^-11 |g| + 2^-25: inside %.3e, outside '
              '%.3e; violations %d' % (what, fig['vertices'], fig['err_in'], fig['err_out'], fig['need_in'], fig['need_out'], grid.tau,
                                       -fig['over_in'], -fig['over_out'], viol[1]))
    # rules 2 to 5 on the sample, then downhill from its worst points
    first = rules_at(grid, x)
    keys = [k for k in ('m2', 'm3', 'm3c', 'm4') if k in first]
    least = {k: float(first[k].min()) for k in keys}
    count = {k: int((first[k] < 0).sum()) for k in keys}
    bad5, either = int(first['bad5'].sum()), int(first['either'].sum())
    cover = float(first['cover'].min()) if 'cover' in first else INF

    def margin_fn(p):
        got = rules_at(grid, p)
        nonlocal bad5, cover
        if 'cover' in got:
            cover = min(cover, float(got['cover'].min()))
        for k in keys:
            least[k] = min(least[k], float(got[k].min()))
            count[k] += int((got[k] < 0).sum())
        bad5 += int(got['bad5'].sum())
        return got['margin']

    sample_least = dict(least)
    search(margin_fn, x, grid.h, grid.radius, search_seed, rounds, margins=first['margin'])
    viol[2] = count['m2']
    if 'm3' in count:
        viol[3], viol['3 combined'], viol[4] = count['m3'], count['m3c'], count['m4']
    viol[5] = bad5
    has = first['has']
    fig.update(points=int(x.shape[0]), bounded=int(has.sum()), either=either, least=least, sample_least=sample_least, cover=cover,
               half_cell=float(first['half_cell'][has].mean()) if has.any() else 0.0)
    names = {'m2': 'cell (rule 2)', 'm3': 'corner (rule 3)', 'm3c': 'combined (rule 3)', 'm4': 'slope headroom (rule 4)'}
    print('[grid64 %s] %d points, %d with a bound (%d within 4 ulp of the upper face, either way); least margins, sample -> after the search: %s; '
          'violations %s' % (what, fig['points'], fig['bounded'], either,
                             '; '.join('%s %.3e -> %.3e' % (names[k], sample_least[k], least[k]) for k in keys), viol))
    if 'm3' in first:
        print('[grid64 %s] rule 4 as a ratio: least L_c (|p - x_k| + 1e-6) / |sdf64(p) - sdf64(x_k)| %.3f' % (what, cover))
        fig.update(half_corner=float(first['half_corner'][has].mean()), half_both=float(first['half_both'][has].mean()))
        sub = torch.nonzero(has).flatten()
        sub = sub[torch.randperm(sub.numel(), generator=torch.Generator().manual_seed(search_seed))[:max(grad_sample, 1)].to(dev)]
        gn = grad64_norm(grid.sdf64, x[sub])
        L = first['L'][sub]
        i = int(gn.argmax())
        ball = x[sub].double().norm(dim=1) <= grid.radius
        fig.update(grad_max=float(gn[i]), L_there=float(L[i]), grad_max_ball=float(gn[ball].max()) if ball.any() else 0.0,
                   least_L_over_grad=float((L / gn.clamp_min(1e-12)).min()))
        print('[grid64 %s] mean half-width: cells %.4f, corners %.4f, combined %.4f; largest fp64 |grad| of %d sampled points %.3f '
              '(in the ball %.3f) under L_c %.3f; least L_c / |grad| %.3f' % (
                  what, fig['half_cell'], fig['half_corner'], fig['half_both'], int(sub.numel()), fig['grad_max'], fig['grad_max_ball'],
                  fig['L_there'], fig['least_L_over_grad']))
    else:
        print('[grid64 %s] mean half-width: cells %.4f' % (what, fig['half_cell']))
    fig['first'] = first
    if check:
        hold(what, fig)
    return fig


def hold(what, fig):
    """the hard figures: no vertex and no point breaks a rule"""
    for rule, n in fig['violations'].items():
        assert n == 0, (what, 'rule %s' % rule, n, fig['least'])
    assert fig['bounded'] > 0, (what, 'no point had a bound')
