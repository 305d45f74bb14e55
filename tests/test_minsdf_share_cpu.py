"""The shared first stage of the tracer's staged min-SDF search (csrc/nefii_tracer.hip: minsdf_share / shared_walk), restated
in NumPy and held to the brute-force search on the CPU.

The model: a ray's search is the argmin (first index of the minimum) of the SDF over n_steps = 100 depth fractions s_i of its
stretch [t_min, t_max], one row of fractions for all rays.  `own_search` is the two-stage search every ray runs without the
sharing (a quarter of the depths, spread over their sorted order, then whatever the slope bound L does not clear);
`shared_search` takes the bounds from a donor ray's evaluated depths instead:
  lo_i = v_c[i] - L d_i - tau,  up_i = v_c[i] + L d_i + tau,  d_i = |p_f(s_i) - p_c(s_i)|,  U = min up_i,
  between evaluated neighbours a < s < b: lb(s) = max(lo_a - L len (s - s_a), lo_b - L len (s_b - s)),
  skipped iff lb - 1e-6 > U; more than stage1_count depths left (the probe included): the ray's own search instead.
Coarse values are taken as exact (tau still widens every bound) and every search pays one probe when it skipped anything -
the kernel's near-miss probes (at most NEAR_PROBES more) are not modelled.  Counts are single-pass evaluations per search."""
import math

import numpy as np
import torch

from nefii_amd import ops, synthetic as syn
from oracle import nets

NS = 100
TAU = 1.2e-3          # a single-pass error bound of the size ops.calibrate_coarse_tau measures on the 512-wide nets


def stage1_count(ns):
    return (ns + 3) // 4


def stage1_pos(ns):
    n1 = stage1_count(ns)
    return [(j * (ns - 1)) // (n1 - 1) for j in range(n1)]


def own_search(v, s, order, llen, tau):
    """-> (evaluated mask, evaluations).  v: exact values [ns]; s: fractions; order: argsort of s; llen = L x stretch length."""
    ns = len(v)
    pos = stage1_pos(ns)
    ev = np.zeros(ns, bool)
    ev[order[pos]] = True
    lim = v[order[pos]].min() + tau
    skipped = 0
    for ja in range(len(pos) - 1):
        ia, ib = order[pos[ja]], order[pos[ja + 1]]
        for kk in range(pos[ja] + 1, pos[ja + 1]):
            i = order[kk]
            lb = max(v[ia] - llen * (s[i] - s[ia]), v[ib] - llen * (s[ib] - s[i])) - tau
            if not (lb - 1e-6 > lim):
                ev[i] = True
            else:
                skipped += 1
                assert v[i] >= lb, 'own search: a skipped depth lies below its bound'
    return ev, int(ev.sum()) + (1 if skipped else 0)


def shared_search(v_f, p_f, v_c, p_c, ev_c, s, order, lip, len_f, tau):
    """-> (evaluated mask, evaluations) or None when the ray falls back to its own search.  p_x: points [ns, 3] of the two
    rays at the fractions s; ev_c: the donor's evaluated depths."""
    ns = len(s)
    delta = np.linalg.norm(p_f - p_c, axis=1)
    lo = np.where(ev_c, v_c - lip * delta - tau, -np.inf)
    up = np.where(ev_c, v_c + lip * delta + tau, np.inf)
    U = up.min()
    known = [k for k in range(ns) if ev_c[order[k]]]
    ev = np.zeros(ns, bool)
    skipped = 0
    for kk in range(ns):
        i = order[kk]
        if ev_c[i]:
            lb = lo[i]
        else:
            a = max((k for k in known if k < kk), default=None)
            b = min((k for k in known if k > kk), default=None)
            lb = -np.inf
            if a is not None:
                lb = max(lb, lo[order[a]] - lip * len_f * (s[i] - s[order[a]]))
            if b is not None:
                lb = max(lb, lo[order[b]] - lip * len_f * (s[order[b]] - s[i]))
        if not (lb - 1e-6 > U):
            ev[i] = True
        else:
            skipped += 1
            assert v_f[i] >= lb, 'shared search: a skipped depth lies below its bound (%g < %g)' % (v_f[i], lb)
    n = int(ev.sum()) + (1 if skipped else 0)
    if n > stage1_count(ns):
        return None
    return ev, n


def sphere_stretch(o, d, radius=1.0):
    """the bounding-sphere stretch of each ray (t_min, t_max clamped at 0.01 as the tracer does), and which rays have one"""
    b = (o * d).sum(1)
    under = b * b - ((o * o).sum(1) - radius * radius)
    ok = under > 0
    sq = np.sqrt(np.where(ok, under, 0.0))
    return np.maximum(-sq - b, 0.01), np.maximum(sq - b, 0.01), ok


def run_waves(sdf, o, d, s, lip, tau=TAU, wave=64, searches=None):
    """Every ray with a stretch searches (searches: a function of the rows of values -> which of them do).  Per wave of `wave` consecutive rays the first one leads (its own search), the
    others take its row.  -> per ray: (own evaluations, shared evaluations, fell back), with the asserts of the rule."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = o.shape[0]
    order = np.argsort(s, kind='stable')
    t0, t1, ok = sphere_stretch(o, d)
    pts = o[:, None, :] + (t0[:, None] + s[None, :] * (t1 - t0)[:, None])[:, :, None] * d[:, None, :]
    vals = sdf(pts.reshape(-1, 3)).reshape(n, len(s))
    if searches is not None:
        ok = ok & searches(vals)
    own_n, shared_n, fell = np.zeros(n, int), np.zeros(n, int), np.zeros(n, bool)
    for w0 in range(0, n, wave):
        lead = None
        for r in range(w0, min(n, w0 + wave)):
            if not ok[r]:
                continue
            brute = int(np.argmin(vals[r]))
            llen = lip * (t1[r] - t0[r])
            ev, own_n[r] = own_search(vals[r], s, order, llen, tau)
            assert int(np.argmin(np.where(ev, vals[r], np.inf))) == brute, ('own search', r)
            if lead is None:
                lead, ev_lead = r, ev
                shared_n[r] = own_n[r]
                continue
            got = shared_search(vals[r], pts[r], vals[lead], pts[lead], ev_lead, s, order, lip, t1[r] - t0[r], tau)
            if got is None:
                fell[r] = True
                shared_n[r] = own_n[r]
            else:
                ev, shared_n[r] = got
                assert int(np.argmin(np.where(ev, vals[r], np.inf))) == brute, ('shared search', r)
            assert shared_n[r] <= own_n[r], (r, shared_n[r], own_n[r])
    return own_n[ok], shared_n[ok], fell[ok], ok


def bundles(n_pixels, seed, cam=(0.2, 0.1, 2.0), ring=(0.35, 0.95), jitter=0.003, n_random=64):
    """64 jittered rays through each of n_pixels points of the plane through the origin that faces the camera - neighbours are
    millimetres apart, as the sub-pixel rays of one pixel are - then n_random unrelated rays."""
    g = np.random.default_rng(seed)
    cam = np.asarray(cam, np.float64)
    z = -cam / np.linalg.norm(cam)
    x = np.cross(z, [0.0, 1.0, 0.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    o, d = [], []
    for k in range(n_pixels):
        rad = ring[0] + (ring[1] - ring[0]) * k / max(n_pixels - 1, 1)
        ang = 2.0 * math.pi * g.uniform()
        tgt = rad * (math.cos(ang) * x + math.sin(ang) * y)
        jit = g.uniform(-jitter, jitter, size=(64, 2))
        t = tgt[None] + jit[:, :1] * x[None] + jit[:, 1:] * y[None]
        dd = t - cam[None]
        o.append(np.repeat(cam[None], 64, 0))
        d.append(dd / np.linalg.norm(dd, axis=1, keepdims=True))
    if n_random:
        oo = g.normal(size=(n_random, 3))
        oo = oo / np.linalg.norm(oo, axis=1, keepdims=True) * (1.5 + g.uniform(size=(n_random, 1)))
        dd = g.normal(size=(n_random, 3)) * 0.45 - oo
        o.append(oo)
        d.append(dd / np.linalg.norm(dd, axis=1, keepdims=True))
    return np.concatenate(o), np.concatenate(d)


def union_of_spheres(x):
    """min_k |x - c_k| - r_k: |grad| = 1 wherever it is differentiable, so L = 1 bounds the slope in every direction"""
    c = np.array([[0.0, 0.0, 0.0], [0.35, 0.2, -0.1], [-0.3, -0.25, 0.2], [0.1, -0.45, 0.05]])
    r = np.array([0.45, 0.22, 0.18, 0.12])
    return (np.linalg.norm(x[:, None, :] - c[None], axis=2) - r[None]).min(1)


def check(sdf, lip, what, seed=3):
    o, d = bundles(8, seed)
    s = np.random.default_rng(seed + 100).uniform(size=NS)
    own, shared, fell, ok = run_waves(sdf, o, d, s, lip)
    px = np.cumsum(ok)[8 * 64 - 1]          # searches of the pixel bundles come first
    print('[minsdf share model, %s] L %.3f: pixel bundles %d searches, %.1f -> %.1f evaluations per search (%d fell back); '
          'unrelated rays %d searches, %.1f -> %.1f (%d fell back)' % (
              what, lip, px, own[:px].mean(), shared[:px].mean(), fell[:px].sum(), len(own) - px, own[px:].mean(),
              shared[px:].mean(), fell[px:].sum()))
    assert px == 8 * 64          # every pixel ray crosses the bounding sphere
    assert (shared <= own).all()
    assert shared[:px].sum() < own[:px].sum()
    return own, shared


def test_share_rule_on_union_of_spheres():
    check(union_of_spheres, 1.0, 'union of spheres')


def test_share_rule_on_golden_net():
    """The 64-wide net of tests/golden/tracer_bumpy_h64.npz (physg, seed 0, bumpy 0.03), L as ops.calibrate_lipschitz finds it."""
    mc = syn.model_conf('physg', hidden=64)
    sd = {k: v.double() for k, v in syn.make_state_dict(mc, seed=0, bumpy=0.03).items()}
    cfg = mc['implicit_network']
    lip = ops.calibrate_lipschitz(lambda x: nets.sdf_gradient(sd, cfg, x.double()), 'cpu')
    assert 1.0 <= lip < 50.0, lip

    def sdf(x):
        with torch.no_grad():
            return nets.sdf_forward(sd, cfg, torch.from_numpy(x))[:, 0].numpy()
    check(sdf, lip, 'tracer_bumpy_h64')
