"""The two certificates of the tracer over the SDF interval grid (csrc/nefii_sdf.hip: grid_blocks_kernel; csrc/nefii_tracer.hip: chord_block_step,
certify_crossing; chord_free, certify_free_stretch; DESIGN section 4h, "certificates") restated in NumPy and held to the reference's
recurrences in oracle.tracer on the CPU.

The block level: the least `lo` of every block of B^3 cells of the SDF interval grid.  The CROSSING rule, for a training-mode ray
with the bounding-sphere stretch [t0, t1]: a_0 = t0, b_0 = t1; per step a walk over EVERY block j the chord [a_k, b_k] crosses,
which the chord is in from depth in_j to out_j; s_j = lo_j - tau - margin; give up unless s_j > sdf_threshold in every block;
a_k+1 = min_j (max(a_k, in_j) + s_j), b_k+1 = max_j (min(b_k, out_j) - s_j) - each front moves at least by the bound of the block
it stands in, so both move by at least m_k - tau - margin, m_k the least lo of the chord; certified when a_k >= b_k for some
k <= sphere_tracing_iters.  A certified ray must be one whose two fronts the reference's sphere tracing reports as crossed
(no front left for the bracket search, t_s >= t_e).  The FREE-STRETCH rule, for an eval-mode ray whose misses nobody reads, is
stated further down; a ray it ends must be one the reference's trace reports as a miss.  Both on an analytic SDF with exact
intervals and on the golden net with the grid's own formula, with rays that graze within one cell of the surface among them;
the crossing rule also on chords whose bound runs out only at k = sphere_tracing_iters."""
import numpy as np
import torch

from oracle import tracer as oracle_tracer

import test_bound_grid_cpu as cells
import test_minsdf_share_cpu as share

B = 4                 # NEFII_BOUND_GRID_BLOCK
MARGIN = 1e-4         # NEFII_CERTIFY_MARGIN
G = 64
P = dict(oracle_tracer.DEFAULT_TRACER)
ITERS = P['sphere_tracing_iters']
THR = P['sdf_threshold']


def block_minima(lo, b=B):
    """lo [G, G, G] -> [ceil(G / b)]^3: the least lo of each block (the last block of an axis is short where b does not divide G)"""
    g = lo.shape[0]
    gb = -(-g // b)
    pad = np.full((gb * b,) * 3, np.inf, dtype=np.float64)
    pad[:g, :g, :g] = lo
    return pad.reshape(gb, b, gb, b, gb, b).min(axis=(1, 3, 5))


def chord_blocks(o, d, a, b, g, n_blocks, radius=1.0, blk=B):
    """the blocks the chord o + t d, a <= t <= b, crosses, in order, each with the depths behind a at which the chord enters and
    leaves it: a walk through the faces it leaves by; None where it leaves the cube"""
    hb = blk * 2.0 * radius / g
    ext = g / blk
    f = (o + a * d + radius) / hb
    if not ((f >= 0).all() and (f < ext).all()):
        return None
    idx = np.floor(f).astype(int)
    with np.errstate(divide='ignore', invalid='ignore'):
        step = np.where(d != 0, hb / np.abs(d), np.inf)
        t = np.where(d > 0, (idx + 1 - f) * step, np.where(d < 0, (f - idx) * step, np.inf))
    u = np.where(d > 0, 1, -1)
    out, t_in = [], 0.0
    while True:
        ax = int(np.argmin(t))
        out.append((tuple(idx), t_in, min(t[ax], b - a)))
        if not t[ax] < b - a:
            return out
        t_in = t[ax]
        idx[ax] += u[ax]
        t[ax] += step[ax]
        if idx[ax] < 0 or idx[ax] >= n_blocks:
            return None


def certify(o, d, t0, t1, blocks, g, tau, thr=THR, iters=ITERS, margin=MARGIN, radius=1.0):
    """-> (certified, k: the steps the bounds took, block look-ups)"""
    off = tau + margin
    a, b, looks = t0, t1, 0
    for k in range(iters + 1):
        if a >= b:
            return True, k, looks
        if k == iters:
            break
        walk = chord_blocks(o, d, a, b, g, blocks.shape[0], radius)
        if walk is None:
            break
        looks += len(walk)
        if not min(blocks[c] for c, _, _ in walk) > thr + off:
            break
        a, b = (min(a + t_in + blocks[c] - off for c, t_in, _ in walk),
                max(a + t_out - (blocks[c] - off) for c, _, t_out in walk))
    return False, k, looks


def oracle_crossed(sdf, o, d):
    """per ray: the reference's sphere tracing left no front for the bracket search and its fronts have crossed"""
    o, d = torch.from_numpy(o).float(), torch.from_numpy(d).float()
    t_io, hit = oracle_tracer.sphere_intersection(o, d)
    live, t_s, t_e, _, _ = oracle_tracer.sphere_trace(sdf, o, d, hit, t_io, P, oracle_tracer.Counters())
    return (hit & ~live & (t_s >= t_e)).numpy(), hit.numpy()


def _rays(n, seed):
    """unit rays from cameras about 2 away, aimed at a disc of radius 1.1 around the origin: hits, misses of every width, rays
    outside the sphere"""
    g = np.random.default_rng(seed)
    cam = g.normal(size=(n, 3))
    cam *= g.uniform(1.6, 2.4, size=(n, 1)) / np.linalg.norm(cam, axis=1, keepdims=True)
    tgt = g.normal(size=(n, 3))
    tgt *= (1.1 * g.uniform(size=(n, 1)) ** 0.5) / np.linalg.norm(tgt, axis=1, keepdims=True)
    d = tgt - cam
    return cam, d / np.linalg.norm(d, axis=1, keepdims=True)


def _profile_min(sdf, o, d, t0, t1, n=256):
    t = t0[:, None] + np.linspace(0.0, 1.0, n)[None] * (t1 - t0)[:, None]
    pts = o[:, None, :] + t[:, :, None] * d[:, None, :]
    return sdf(torch.from_numpy(pts.reshape(-1, 3)).float()).reshape(len(o), n).double().numpy().min(1)


def _suite(sdf, seed, n_keep=320):
    """rays with a stretch: every ray of 4000 that grazes (least SDF along it within one cell of 0, above it) and others up to
    n_keep"""
    o, d = _rays(4000, seed)
    t0, t1, ok = share.sphere_stretch(o, d)
    o, d, t0, t1 = o[ok], d[ok], t0[ok], t1[ok]
    least = _profile_min(sdf, o, d, t0, t1)
    graze = (least > 0) & (least < 2.0 / G)
    pick = np.nonzero(graze)[0][:n_keep // 2]
    rest = np.setdiff1d(np.arange(len(o)), pick)[:n_keep - len(pick)]
    sel = np.concatenate([pick, rest])
    return o[sel], d[sel], t0[sel], t1[sel], graze[sel]


def _check(what, sdf, lo, tau, seed):
    o, d, t0, t1, graze = _suite(sdf, seed)
    assert graze.sum() >= 20, (what, 'too few rays graze within one cell of the surface', int(graze.sum()))
    blocks = block_minima(lo)
    crossed, _ = oracle_crossed(sdf, o, d)
    n_cert = wrong = looks = graze_cert = 0
    for r in range(len(o)):
        ok, _, n = certify(o[r], d[r], t0[r], t1[r], blocks, G, tau)
        looks += n
        if ok:
            n_cert += 1
            graze_cert += int(graze[r])
            wrong += int(not crossed[r])
    print('[grid certify model, %s] %d rays (%d graze within one cell), %d cross; certified %d (%d of the grazing ones), wrong %d; '
          '%.1f block look-ups per ray' % (what, len(o), graze.sum(), crossed.sum(), n_cert, graze_cert, wrong, looks / len(o)))
    assert wrong == 0, what
    assert 0 < n_cert <= crossed.sum(), what


def _spheres(x):
    return torch.from_numpy(share.union_of_spheres(x.double().numpy())).float()


def test_certificate_on_union_of_spheres_with_exact_intervals():
    """a distance function (slope 1): its value at a cell's centre less the half diagonal bounds it over the cell, no tau"""
    h = 2.0 / G
    c = -1.0 + (np.arange(G) + 0.5) * h
    ctr = np.stack(np.meshgrid(c, c, c, indexing='ij'), -1).reshape(-1, 3)
    lo = share.union_of_spheres(ctr).reshape(G, G, G) - h * np.sqrt(3.0) / 2.0
    _check('union of spheres', _spheres, lo, 0.0, 11)


def test_certificate_on_golden_net_with_the_grids_formula():
    what, sdf, _ = cells._field(1)
    lo, _, _ = cells._grid(sdf, cells.L_FLOOR, G)
    _check(what, sdf, lo.double().numpy(), cells.TAU, 12)


def test_walk_covers_every_block_the_chord_crosses():
    """densely sampled points of a chord fall into blocks of the walk only; the walk's blocks are neighbours through a face"""
    o, d = _rays(200, 5)
    t0, t1, ok = share.sphere_stretch(o, d)
    hb = B * 2.0 / G
    for r in np.nonzero(ok)[0]:
        walk = chord_blocks(o[r], d[r], t0[r], t1[r], G, G // B)
        if walk is None:
            continue
        t = np.linspace(t0[r], t1[r], 4000)
        pts = o[r] + t[:, None] * d[r]
        seen = set(map(tuple, np.floor((pts + 1.0) / hb).astype(int)))
        ids = [c for c, _, _ in walk]
        assert seen <= set(ids), (r, seen - set(ids))
        assert all(sum(abs(p - q) for p, q in zip(a, b)) == 1 for a, b in zip(ids, ids[1:]))
        # ... and the depths at which it enters and leaves them tile the chord
        assert walk[0][1] == 0.0 and abs(walk[-1][2] - (t1[r] - t0[r])) < 1e-12
        assert all(x[2] == y[1] for x, y in zip(walk, walk[1:]))
        for c, t_in, t_out in walk:
            mid = o[r] + (t0[r] + 0.5 * (t_in + t_out)) * d[r]
            assert t_out < t_in + 1e-12 or tuple(np.floor((mid + 1.0) / hb).astype(int)) == c


def test_short_last_block_and_outside():
    lo = np.arange(6 ** 3, dtype=np.float64).reshape(6, 6, 6)
    bm = block_minima(lo)
    assert bm.shape == (2, 2, 2) and bm[0, 0, 0] == 0 and bm[1, 1, 1] == lo[4, 4, 4] and bm[1, 0, 1] == lo[4, 0, 4]
    # a chord that starts outside the cube has no bound
    assert chord_blocks(np.array([1.5, 0.0, 0.0]), np.array([-1.0, 0.0, 0.0]), 0.01, 1.0, G, G // B) is None
    assert not certify(np.array([1.5, 0.0, 0.0]), np.array([-1.0, 0.0, 0.0]), 0.01, 1.0, np.full((16,) * 3, 0.5), G, 0.0)[0]


def test_bound_runs_out_only_at_the_last_iteration():
    """a constant field c over a chord of length 2 through the centre: the reference's fronts move by c a step, the bounds by
    c - margin.  c with 2 ITERS (c - margin) >= 2: certified, at k = ITERS exactly, and the reference has crossed.  c a little
    lower, 2 ITERS c >= 2 > 2 ITERS (c - margin): the bound fails at k = ITERS only - not certified - while the reference still
    crosses (the rule is allowed to lose such a ray).  Lower still, 2 ITERS c < 2: not certified, and the reference does not
    cross within the iterations."""
    o, d = np.array([[0.0, 0.0, -2.0]]), np.array([[0.0, 0.0, 1.0]])
    t0, t1, _ = share.sphere_stretch(o, d)
    length = float(t1[0] - t0[0])
    for c, want_cert, want_cross in ((length / (2 * ITERS) + MARGIN + 1e-6, True, True),
                                     (length / (2 * ITERS) + 0.5 * MARGIN, False, True),
                                     (length / (2 * ITERS) - 1e-4, False, False)):
        blocks = np.full((G // B,) * 3, c)
        ok, k, _ = certify(o[0], d[0], t0[0], t1[0], blocks, G, 0.0)
        crossed, _ = oracle_crossed(lambda x, c=c: torch.full((x.shape[0],), c, dtype=x.dtype), o, d)
        assert ok == want_cert and k == ITERS, (c, ok, k)
        assert bool(crossed[0]) == want_cross, (c, crossed)
        assert not ok or crossed[0]


# ---- the free-stretch rule (certify_free_stretch, chord_free, end_free) -------------------------------------------------------
# An eval-mode ray whose misses nobody reads ends as a miss when every cell of the stretch [t_s, t_max] - from its start front to
# where it leaves the bounding sphere - has lo - tau - margin > sdf_threshold: asked before the first evaluation, and at every
# iteration behind the step, before the new points are evaluated.  One look-up at t_s's own cell first; then a walk by blocks, a
# block that is not free walked again by its cells over the depths the chord is in it.

def stretch_free(o, d, t_s, t_max, lo, blocks, tau, thr=THR, margin=MARGIN, radius=1.0):
    g = lo.shape[0]
    stop = thr + tau + margin
    c = np.floor((o + t_s * d + radius) * (g / (2.0 * radius))).astype(int)
    if (c < 0).any() or (c >= g).any() or not lo[tuple(c)] > stop or not t_s < t_max:
        return False
    walk = chord_blocks(o, d, t_s, t_max, g, blocks.shape[0], radius)
    if walk is None:
        return False
    for blk, t_in, t_out in walk:
        if blocks[blk] > stop:
            continue
        inner = chord_blocks(o, d, t_s + t_in, t_s + t_out, g, g, radius, blk=1)
        if inner is None or not all(lo[cell] > stop for cell, _, _ in inner):
            return False
    return True


def sphere_trace_with_rule(sdf, o, d, ended_at):
    """oracle.tracer.sphere_trace restated statement by statement (eval-mode rays, every ray inside or through the sphere), with
    ended_at(iteration, live_s, t_s, t_e) called where the tracer asks the rule.  Returns what the oracle's returns."""
    t_io, hit = oracle_tracer.sphere_intersection(o, d)
    thr, zero = P['sdf_threshold'], torch.zeros(())
    f = lambda t, m: torch.where(m, sdf(o + t[:, None] * d), zero)
    t_s, t_e = torch.where(hit, t_io[:, 0], zero), torch.where(hit, t_io[:, 1], zero)
    live_s, live_e = hit.clone(), hit.clone()
    t_min, t_max = t_s.clone(), t_e.clone()
    ended_at(0, live_s, t_s, t_e)
    nxt_s, nxt_e = f(t_s, live_s), f(t_e, live_e)
    it = 0
    while True:
        cur_s = torch.where(live_s, nxt_s, zero)
        cur_s = torch.where(cur_s <= thr, zero, cur_s)
        cur_e = torch.where(live_e, nxt_e, zero)
        cur_e = torch.where(cur_e <= thr, zero, cur_e)
        live_s, live_e = live_s & (cur_s > thr), live_e & (cur_e > thr)
        if it == ITERS or not (live_s.any() or live_e.any()):
            break
        it += 1
        t_s, t_e = t_s + cur_s, t_e - cur_e
        ended_at(it, live_s, t_s, t_e)
        nxt_s, nxt_e = f(t_s, live_s), f(t_e, live_e)
        bad_s, bad_e = nxt_s < 0, nxt_e < 0
        k = 0
        while (bad_s.any() or bad_e.any()) and k < P['line_step_iters']:
            back = (1 - P['line_search_step']) / (2 ** k)
            t_s = torch.where(bad_s, t_s - back * cur_s, t_s)
            t_e = torch.where(bad_e, t_e + back * cur_e, t_e)
            nxt_s = torch.where(bad_s, sdf(o + t_s[:, None] * d), nxt_s)
            nxt_e = torch.where(bad_e, sdf(o + t_e[:, None] * d), nxt_e)
            bad_s, bad_e = nxt_s < 0, nxt_e < 0
            k += 1
        live_s, live_e = live_s & (t_s < t_e), live_e & (t_s < t_e)
    return live_s, t_s, t_e, t_min, t_max


def _secondary_suite(sdf, seed, n_keep=300):
    """rays started 0.01 off the surface into the hemisphere of its normal, from the hit points of primary rays; every one of
    them that then grazes the surface again within one cell (least SDF behind depth 0.1 in (0, h)), and others up to n_keep"""
    o, d = _rays(3000, seed)
    o, d = torch.from_numpy(o).float(), torch.from_numpy(d).float()
    first = oracle_tracer.trace(sdf, o, d, torch.ones(len(o), dtype=torch.bool), P, False)
    p = first['points'][first['hit']]
    e = 1e-3 * torch.eye(3)
    grad = torch.stack([sdf(p + e[k]) - sdf(p - e[k]) for k in range(3)], 1)
    g = torch.Generator().manual_seed(seed)
    w = torch.nn.functional.normalize(torch.randn(len(p), 3, generator=g), dim=1)
    # (a third of them flattened over the surface: those graze)
    nrm = torch.nn.functional.normalize(grad, dim=1)
    flat = torch.nn.functional.normalize(w - 0.8 * (w * nrm).sum(1, keepdim=True) * nrm, dim=1)
    steep = torch.nn.functional.normalize(nrm + 0.3 * w, dim=1)               # (... a third close to the normal: those get away)
    w = torch.where((torch.arange(len(p)) % 3 == 0)[:, None], flat, torch.where((torch.arange(len(p)) % 3 == 1)[:, None], steep, w))
    w = torch.where((w * grad).sum(1, keepdim=True) < 0, -w, w)
    o2 = (p + 0.01 * w).double().numpy()
    d2 = w.double().numpy()
    t0, t1, ok = share.sphere_stretch(o2, d2)
    o2, d2, t0, t1 = o2[ok], d2[ok], t0[ok], t1[ok]
    least = _profile_min(sdf, o2, d2, np.maximum(t0, 0.1), t1)
    graze = (least > 0) & (least < 2.0 / G)
    pick = np.nonzero(graze)[0][:n_keep // 2]
    rest = np.setdiff1d(np.arange(len(o2)), pick)[:n_keep - len(pick)]
    sel = np.concatenate([pick, rest])
    return o2[sel], d2[sel], graze[sel]


def _check_free(what, sdf, lo, tau, seed):
    o, d, graze = _secondary_suite(sdf, seed)
    assert graze.sum() >= 20, (what, 'too few rays graze within one cell of the surface', int(graze.sum()))
    blocks = block_minima(lo)
    n = len(o)
    ended = np.zeros(n, dtype=bool)
    at = np.full(n, -1)
    ot, dt = torch.from_numpy(o).float(), torch.from_numpy(d).float()
    _, sph = oracle_tracer.sphere_intersection(ot, dt)
    t_max = oracle_tracer.sphere_intersection(ot, dt)[0][:, 1].double().numpy()

    def ended_at(it, live_s, t_s, t_e):
        for r in np.nonzero((live_s & (t_s < t_e)).numpy() & ~ended)[0]:
            if stretch_free(o[r], d[r], float(t_s[r]), t_max[r], lo, blocks, tau):
                ended[r], at[r] = True, it

    mine = sphere_trace_with_rule(sdf, ot, dt, ended_at)
    ref = oracle_tracer.sphere_trace(sdf, ot, dt, sph, oracle_tracer.sphere_intersection(ot, dt)[0], P, oracle_tracer.Counters())
    for a, b in zip(mine, ref):
        assert torch.equal(a, b), 'the restated recurrence is not the oracle\'s'
    full = oracle_tracer.trace(sdf, ot, dt, torch.ones(n, dtype=torch.bool), P, False)
    hit = full['hit'].numpy()
    wrong = int((ended & hit).sum())
    print('[grid certify model, free stretch, %s] %d rays started 0.01 off the surface (%d graze within one cell), %d miss; ended %d '
          '(%d of the grazing ones; %d before the first evaluation, the others at iterations up to %d), ended rays that hit %d' % (
              what, n, graze.sum(), (~hit).sum(), ended.sum(), (ended & graze).sum(), (at == 0).sum(), at.max(), wrong))
    assert wrong == 0, what
    assert 0 < ended.sum() <= (~hit).sum(), what
    assert (at > 0).any(), (what, 'no ray was ended behind a step: the per-iteration rule is not exercised')


def test_free_stretch_on_union_of_spheres_with_exact_intervals():
    h = 2.0 / G
    c = -1.0 + (np.arange(G) + 0.5) * h
    ctr = np.stack(np.meshgrid(c, c, c, indexing='ij'), -1).reshape(-1, 3)
    lo = share.union_of_spheres(ctr).reshape(G, G, G) - h * np.sqrt(3.0) / 2.0
    _check_free('union of spheres', _spheres, lo, 0.0, 21)


def test_free_stretch_on_golden_net_with_the_grids_formula():
    what, sdf, _ = cells._field(1)
    lo, _, _ = cells._grid(sdf, cells.L_FLOOR, G)
    _check_free(what, sdf, lo.double().numpy(), cells.TAU, 22)


def test_free_stretch_walk_descends_to_the_cells():
    """a block whose minimum fails while the cells the chord crosses in it are free does not stop the rule; one cell on the chord
    that is not free does; so does t_s's own cell"""
    lo = np.full((G, G, G), 0.5)
    o, d = np.array([0.01, 0.013, -0.9]), np.array([0.0, 0.0, 1.0])
    lo[40, 40, 20] = -1.0                       # in a block the chord crosses (cells 32.. of x and y), off the chord
    assert stretch_free(o, d, 0.0, 1.8, lo, block_minima(lo), 0.0)
    lo[32, 32, 20] = 0.0                        # on the chord
    assert not stretch_free(o, d, 0.0, 1.8, lo, block_minima(lo), 0.0)
    assert stretch_free(o, d, 0.7, 1.8, lo, block_minima(lo), 0.0)         # ... and behind the start front it no longer matters
    lo[32, 32, 25] = 0.0
    assert not stretch_free(o, d, 0.7, 1.8, lo, block_minima(lo), 0.0)     # t_s's own cell (z = -0.2: cell 25)
