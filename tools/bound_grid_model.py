"""SDF interval grid for the staged searches: what the rule (tests/test_bound_grid_cpu.py) predicts on a bench workload's own
scene and rays - single-pass evaluations per dense search today against the grid, by search kind, for several grid sizes.

    python tools/bound_grid_model.py [workload=cfg3] [G,G,...=128,256,384] [L_floor=1.0] [safety=1.5]

Needs the GPU: one training-mode forward of the model supplies the rays of its tracer calls (the primary trace and the
Monte-Carlo renderer's secondary trace) and, from the kept workspaces, the stretch each dense search ran over; the SDF values
of the rows and of the grid vertices come from the tracer's own single-pass evaluator.  Every grid size is reported with the
cell intervals alone and with the bounds from the cells' corners on top ("+ corners": tests/test_bound_vertices_cpu.py; the
tracer runs those for the eval-mode bracket searches and the training-mode ones inside the object mask, the other kinds are
report-only).  What is modelled per search:
  eval-mode bracket search (secondary rays): today's quarter-row windows, the opt-in evaluated first stage with the global
    slope bound (bracket_staged_eval), and the grid's walk;
  training-mode bracket search outside the object mask and min-SDF searches that evaluate a first stage of their own (leaders
    and fall-backs of the shared first stage): today's evaluated first stage against the grid's walk;
  training-mode bracket search inside the object mask: the quarter-row windows (what NEFII_BOUND_GRID_TRAINING=0 leaves) against
    the grid's walk as built - the argmin read, the leading exact chunk in front;
  followers of a shared first stage are counted and left as they are.
Not modelled: the searches the leading exact chunk settles are left out of both sides by their coarse values (first negative
sample among samples 1..5); near-miss probes; the split-precision refinement, which both sides pay alike.

Rays ended before they are traced ("certificates"), on the library's own grid at the first size given: the
training-mode calls are traced again with and without the crossing certificate (nefii_trace_grid.certify) - rays
certified, of how many whose fronts cross, sphere-tracing evaluations saved, block look-ups per ray, and WRONG certificates
(certified rays whose fronts the uncertified trace did not see cross; must be 0) - and the eval-mode call whose misses nobody
reads with and without the free-stretch certificate: rays ended, evaluations saved, look-ups per ray, ended rays that hit (must
be 0).  These two lines MEASURE the built kernels against the uncertified trace; they are not a prediction."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from nefii_amd import _lib, conf, ops, synthetic as syn                             # noqa: E402
from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork           # noqa: E402
import test_bound_grid_cpu as model                                                 # noqa: E402
import test_bound_vertices_cpu as corners                                           # noqa: E402

F_SPH, F_SAMP, F_HIT, F_OWN = 1 << 8, 1 << 9, 1 << 10, 1 << 11      # csrc/nefii_tracer.hip, flags layout
F_CERT = 1 << 7                                                     # (behind sphere tracing: the certificate ended the ray)
CHUNK = 6


def ws_array(ws, n, k):
    stride = (4 * n + 255) // 256 * 256
    return ws[k * stride:k * stride + 4 * n]


def grid_values(pm, G, radius, dev):
    """single-pass SDF at the (G+1)^3 vertices, slab by slab -> [(G+1)]^3, seconds"""
    torch.cuda.synchronize()
    t = time.time()
    a = -radius + torch.arange(G + 1, device=dev, dtype=torch.float32) * (2.0 * radius / G)
    out = torch.empty(G + 1, G + 1, G + 1, device=dev)
    yz = torch.stack(torch.meshgrid(a, a, indexing='ij'), -1).reshape(-1, 2)
    for i0 in range(0, G + 1, 16):
        xs = a[i0:i0 + 16]
        pts = torch.cat([xs[:, None, None].expand(-1, yz.shape[0], 1), yz[None].expand(xs.numel(), -1, -1)], -1)
        out[i0:i0 + 16] = ops.sdf_eval(pm, pts.reshape(-1, 3).contiguous(), coarse=True).reshape(xs.numel(), G + 1, G + 1)
    torch.cuda.synchronize()
    return out, time.time() - t


def rows_of(pm, o, d, t0, t1, frac):
    """points [n, ns, 3] and single-pass values [n, ns] of the rays' samples at t0 + frac (t1 - t0)"""
    t = t0[:, None] + frac[None, :] * (t1 - t0)[:, None]
    pts = o[:, None, :] + t[:, :, None] * d[:, None, :]
    v = torch.cat([ops.sdf_eval(pm, c.reshape(-1, 3).contiguous(), coarse=True) for c in pts.split(1 << 14)]).reshape(t.shape)
    return pts, v


def windows_today(v, obj, tau, windowed):
    """today's default for a bracket search: quarter rows until a surely negative sample (in the mask), else the whole row"""
    ns = v.shape[1]
    cw = (ns + 3) // 4
    i0, i1 = model._first(v < tau), model._first(v < -tau)
    quarters = torch.clamp((i1 // cw + 1) * cw, max=ns)
    cost = torch.where((i1 < ns) & (i0 > 0), quarters, torch.full_like(i1, ns))
    return torch.where(obj, cost, torch.full_like(cost, ns)) if windowed else torch.full_like(i1, ns)


def followers_on_sparser_rows(pm, c, kf, leaders, s_sorted, t_min, t_max, lip, tau, grid, radius, G, n_waves=48):
    """Report only: the followers of a shared first stage re-modelled on a donor row that holds what the corner bounds leave of it
    instead of an evaluated first stage and its survivors (shared_walk bounds a follower from the donor's EVALUATED samples, so a
    sparser row bounds less).  A sample of waves; the donor of a wave is taken to be its lowest ray with a search of its own;
    the rule is tests/test_minsdf_share_cpu.py's shared_search (fall-back: the ray's own search - today's evaluated first stage,
    or the corner walk)."""
    import numpy as np
    import test_minsdf_share_cpu as share_rule
    lead_k = leaders['k'].cpu().numpy()
    donor_row = {}
    for row, r in enumerate(lead_k):
        donor_row.setdefault(int(r) // 64, row)
    kf_np = kf.cpu().numpy()
    waves = sorted({int(r) // 64 for r in kf_np} & set(donor_row))
    if not waves:
        return
    waves = waves[::max(1, len(waves) // n_waves)][:n_waves]
    s = s_sorted.cpu().numpy().astype(np.float64)
    order = np.arange(len(s))
    tot = dict(today=0, new=0, fell_today=0, fell_new=0, broke_today=0, broke_new=0, n=0, lead_today=0, lead_new=0)
    for wv in waves:
        row = donor_row[wv]
        rays = torch.tensor([int(r) for r in kf_np if int(r) // 64 == wv], device=kf.device)
        pts, v = rows_of(pm, c['o'][rays], c['d'][rays], t_min[rays], t_max[rays], s_sorted)
        lo_s, hi_s = model.gather(grid[0], grid[1], pts, radius)
        lo_c, hi_c = corners.corner_gather(grid[2], grid[3], pts, radius, tau)
        own_new = model.evaluations(corners.minsdf_walk(lo_s, hi_s, lo_c, hi_c, tau)[0]).cpu().numpy()
        v_c, p_c = leaders['v'][row].cpu().numpy().astype(np.float64), leaders['pts'][row].cpu().numpy().astype(np.float64)
        ev_today, ev_new = leaders['keep_today'][row].cpu().numpy(), leaders['keep_new'][row].cpu().numpy()
        tot['lead_today'] += int(ev_today.sum())
        tot['lead_new'] += int(ev_new.sum())
        length = (t_max - t_min)[rays].cpu().numpy().astype(np.float64)
        vf, pf = v.cpu().numpy().astype(np.float64), pts.cpu().numpy().astype(np.float64)
        for j in range(rays.numel()):
            for key, ev_c in (('today', ev_today), ('new', ev_new)):
                try:
                    got = share_rule.shared_search(vf[j], pf[j], v_c, p_c, ev_c, s, order, lip, length[j], tau)
                except AssertionError:
                    # the rule's own check "a skipped depth lies above its bound" failed.  Single-pass values stand in for exact
                    # ones here, so a bound missed by < tau is the stand-in's; counted on its own, NOT as a fall-back, and the
                    # ray priced at its own search
                    got = None
                    tot['broke_' + key] += 1
                    tot['fell_' + key] -= 1
                if got is None:
                    tot['fell_' + key] += 1
                    tot[key] += share_rule.own_search(vf[j], s, order, lip * length[j], tau)[1] if key == 'today' else int(own_new[j])
                else:
                    tot[key] += got[1]
            tot['n'] += 1
    n, w = max(tot['n'], 1), len(waves)
    print('  %-58s %7d followers of %d sampled waves at G %d: evaluations per follower %.2f on today\'s donor rows (%.1f evaluated '
          'samples each; %d fall back, %d broke the rule\'s check) -> %.2f on the rows the corner bounds leave (%.1f; %d fall back, %d broke '
          'the check): report only' % (
              'min-SDF, followers re-modelled on the leaders\' new rows', tot['n'], w, G, tot['today'] / n, tot['lead_today'] / w,
              tot['fell_today'], tot['broke_today'], tot['new'] / n, tot['lead_new'] / w, tot['fell_new'], tot['broke_new']))


def certified_crossings(net, pm, c, radius, G):
    """one training-mode call traced with the certificate off and on, on the library's grid of G cells per edge"""
    cells, verts = net.bound_grid(radius, G, vertices=True)
    if cells is None:
        print('  certified crossings: no grid for this network')
        return
    blocks = net.bound_grid_blocks(radius, G)
    n = c['o'].shape[0]
    res = {}
    for on in (False, True):
        kept, cnt = [], torch.zeros(ops.CERTIFY_COUNTS, device=c['o'].device, dtype=torch.int32)
        out = ops.trace_rays(pm, c['params'], c['o'], c['d'], c['obj'], c['lin'], c['steps'], want_counters=True, bound_grid=cells,
                             bound_vertices=verts, bound_grid_training=True, bound_grid_certify=blocks if on else None,
                             certify_counts=cnt, keep_workspace=kept)
        flags = ws_array(kept[0][0], n, _lib.TRACE_WS_FLOAT_ARRAYS).view(torch.int32).clone()
        res[on] = (out, flags, cnt.cpu().tolist())
    (off, f0, _), (on, f1, cnt) = res[False], res[True]
    same = all(torch.equal(a, b) for a, b in zip(off[:3], on[:3]))
    crossed = ((f0 & F_SPH) != 0) & ((f0 & F_SAMP) == 0) & ((f0 & F_HIT) == 0)
    cert = (f1 & F_CERT) != 0
    q = lambda t: int(t[3][:, _lib.CNT_SINGLES].sum() + t[3][:, _lib.CNT_COARSE_SINGLES].sum())
    sp = lambda t: [int(x.sum()) for x in ops.executed_evals(t[3], c['lin'].numel())]
    audit = on[3][:, _lib.CNT_LIP_AUDIT].cpu().contiguous().view(torch.float32).max().item()
    print('  certified crossings, G %d, blocks of %d cells: %d rays, %d miss, the fronts of %d cross; certified %d (%.1f %% of the crossed), '
          'WRONG certificates %d; sphere-tracing evaluations %d -> %d (saved %d, %.2f per certified ray); executed split / single-pass '
          '%s -> %s; block look-ups %.1f per ray; outputs %s; audit %.1e' % (
              G, ops.BOUND_GRID_BLOCK, n, int((~off[1]).sum()), int(crossed.sum()), cnt[0], 100.0 * cnt[0] / max(int(crossed.sum()), 1),
              int((cert & ~crossed).sum()), q(off), q(on), q(off) - q(on), (q(off) - q(on)) / max(cnt[0], 1), sp(off), sp(on),
              cnt[1] / n, 'bit-identical' if same else 'DIFFER', audit))


def freed_misses(net, pm, c, radius, G):
    """one eval-mode call whose misses nobody reads, traced with the free-stretch certificate off and on, on the library's grid"""
    cells, verts = net.bound_grid(radius, G, vertices=True)
    if cells is None:
        print('  eval-mode misses ended as free: no grid for this network')
        return
    blocks = net.bound_grid_blocks(radius, G)
    n = c['o'].shape[0]
    res = {}
    for on in (False, True):
        kept, cnt = [], torch.zeros(ops.CERTIFY_COUNTS, device=c['o'].device, dtype=torch.int32)
        out = ops.trace_rays(pm, c['params'], c['o'], c['d'], c['obj'], c['lin'], c['steps'], want_counters=True, bound_grid=cells,
                             bound_vertices=verts, bound_grid_certify=blocks if on else None, certify_counts=cnt, certify_parts=2,
                             keep_workspace=kept)
        flags = ws_array(kept[0][0], n, _lib.TRACE_WS_FLOAT_ARRAYS).view(torch.int32).clone()
        res[on] = (out, flags, cnt.cpu().tolist())
    (off, _, _), (on, f1, cnt) = res[False], res[True]
    hit = off[1]
    same = torch.equal(on[1], hit) and torch.equal(on[0][hit], off[0][hit]) and torch.equal(on[2][hit], off[2][hit])
    freed = (f1 & F_CERT) != 0
    q = lambda t: int(t[3][:, _lib.CNT_SINGLES].sum() + t[3][:, _lib.CNT_COARSE_SINGLES].sum())
    sp = lambda t: [int(x.sum()) for x in ops.executed_evals(t[3], c['lin'].numel())]
    audit = on[3][:, _lib.CNT_LIP_AUDIT].cpu().contiguous().view(torch.float32).max().item()
    print('  eval-mode misses ended as free, G %d: %d rays, %d miss; ended %d (%.1f %% of the misses), WRONG (ended rays that hit) %d; '
          'sphere-tracing evaluations %d -> %d (saved %d); executed split / single-pass %s -> %s; look-ups %.1f per ray; probes %d -> %d; '
          'hit mask and hit outputs %s; audit %.1e' % (
              G, n, int((~hit).sum()), cnt[2], 100.0 * cnt[2] / max(int((~hit).sum()), 1), int((freed & hit).sum()), q(off), q(on),
              q(off) - q(on), sp(off), sp(on), cnt[3] / n, int(off[3][:, _lib.CNT_PROBES].sum()), int(on[3][:, _lib.CNT_PROBES].sum()),
              'bit-identical' if same else 'DIFFER', audit))


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else 'cfg3'
    sizes = [int(x) for x in (sys.argv[2] if len(sys.argv) > 2 else '128,256,384').split(',')]
    l_floor = float(sys.argv[3]) if len(sys.argv) > 3 else model.L_FLOOR
    safety = float(sys.argv[4]) if len(sys.argv) > 4 else model.SAFETY
    w = dict(syn.WORKLOADS[name])
    mc = syn.model_conf(w['model'])
    sd = syn.make_state_dict(mc, seed=0, scene=w.get('scene'))
    dev = torch.device('cuda:0')
    m = IDRNetwork(conf.from_dict(mc))
    m.load_state_dict(sd)
    m = m.to(dev)
    m.freeze_geometry()
    m.ray_tracer.trace_tier = os.environ.get('NEFII_TRACE_TIER', '1') != '0'        # as bench.py runs the workload
    m.train()
    inp, _ = syn.make_inputs(w['num_pixels'], w['image_hw'], w['focal'], w['cam_pos'], w['num_rays'], seed=1)
    inp = {k: v.to(dev) for k, v in inp.items()}

    calls = []
    inner = ops.trace_rays

    def recording(pm_sdf, params, origins, dirs, object_mask, lin_steps, minsdf_steps=None, **kw):
        kept = []
        kw['keep_workspace'] = kept
        res = inner(pm_sdf, params, origins, dirs, object_mask, lin_steps, minsdf_steps, **kw)
        calls.append(dict(training=bool(params.training), unread=bool(params.unread_misses), o=origins, d=dirs,
                          obj=object_mask.reshape(-1).bool(), lin=lin_steps, steps=minsdf_steps, kept=kept,
                          tau=float(params.coarse_tau), lip=float(params.minsdf_lipschitz), params=params))
        return res
    ops.trace_rays = recording
    m.ray_tracer.adaptive_rounds = False
    with torch.no_grad():
        m(inp)
    torch.cuda.synchronize()
    ops.trace_rays = inner

    net = m.implicit_network
    radius = float(m.ray_tracer.object_bounding_sphere)
    pm = net.packed(f16x3=True)
    tau = net.coarse_tau(radius)
    lip = net.minsdf_lipschitz(radius)
    print('%s: %d tracer calls; tau %.6f, global L %.3f, L_floor %.2f, safety %.2f' % (name, len(calls), tau, lip, l_floor, safety))

    grids = {}
    for G in sizes:
        g, sec = grid_values(pm, G, radius, dev)
        torch.cuda.synchronize()
        t = time.time()
        lo, hi, lcell = model.build_cells(g, radius, tau, l_floor, safety)
        torch.cuda.synchronize()
        # the arrays behind the corner bounds (tests/test_bound_vertices_cpu.py): fp16 vertex values, fp16 slope bound per cell
        grids[G] = (lo, hi, corners.encode_vertices(g), corners.encode_slopes(corners.corner_slopes(g, radius, l_floor, safety)))
        print('G %3d: %.1f M vertices evaluated in %.3f s (torch cells %.3f s), %.1f MB of cells; L_cell median %.2f, 99th pct %.2f, '
              'max %.2f; slack tau + L_cell h sqrt(3)/2: median %.4f' % (
                  G, (G + 1) ** 3 / 1e6, sec, time.time() - t, 4 * G ** 3 / 1e6, float(lcell.median()),
                  float(lcell.flatten()[::7].float().quantile(0.99)), float(lcell.max()),
                  tau + float(lcell.median()) * 2 * radius / G * 0.8660254))
        del g, lcell

    total_today = 0
    total_grid = {G: 0 for G in sizes}
    total_corner = {G: 0 for G in sizes}

    def report(what, n, today, staged, per_grid, aud, per_corner, aud_corner):
        nonlocal total_today
        if n == 0:
            print('  %-58s none' % what)
            return
        total_today += int(today.sum())
        line = '  %-58s %7d searches, evaluations per search: today %6.2f' % (what, n, today.float().mean())
        if staged is not None:
            line += ', evaluated first stage (global L) %6.2f' % staged.float().mean()
        for G in sizes:
            total_grid[G] += int(per_grid[G].sum())
            line += ' | G %d: %6.2f (audit %.1e)' % (G, per_grid[G].float().mean(), aud[G])
            total_corner[G] += int(per_corner[G].sum())
            line += ', + corners %6.2f (audit %.1e)' % (per_corner[G].float().mean(), aud_corner[G])
        print(line)

    for ci, c in enumerate(calls):
        ws, _lo0, n = c['kept'][0]
        assert len(c['kept']) == 1 and n == c['o'].shape[0]
        f32 = lambda k: ws_array(ws, n, k).view(torch.float32)
        flags = ws_array(ws, n, _lib.TRACE_WS_FLOAT_ARRAYS).view(torch.int32)
        t_s, t_e, t_min, t_max = f32(0), f32(1), f32(6), f32(7)
        obj, training = c['obj'], c['training']
        sph, samp, hit, own = ((flags & b) != 0 for b in (F_SPH, F_SAMP, F_HIT, F_OWN))
        print('call %d: %s mode, %d rays%s' % (ci, 'training' if training else 'eval', n, ', misses unread' if c['unread'] else ''))
        windowed = n >= 32768
        # ---- bracket searches
        sel = samp.nonzero().flatten()
        pts, v = rows_of(pm, c['o'][sel], c['d'][sel], t_s[sel], t_e[sel], c['lin'])
        so = obj[sel]
        length = (t_e - t_s)[sel]
        coarse = 0.5 * (v[:, 0].clamp(min=0) + v[:, -1].clamp(min=0) + length) > 3.0 * tau
        gate = so & (v[:, 0] <= 1.0 * (CHUNK - 1) * length / (v.shape[1] - 1))
        ind = model._first(v < 0)
        in_chunk = gate & (ind >= 1) & (ind < CHUNK)
        print('  bracket searches: %d, of them %d settled by the leading exact chunk and %d too short for the coarse pass (left out)' % (
            sel.numel(), int((in_chunk & coarse).sum()), int((~coarse).sum())))
        live = coarse & ~in_chunk
        miss_argmin = not (c['unread'] and not training)
        for what, pick, inside in (('bracket, inside the mask', live & so, True), ('bracket, outside the mask', live & ~so, False)):
            k = pick.nonzero().flatten()
            if k.numel() == 0:
                continue
            vk, ok = v[k], so[k]
            today = windows_today(vk, ok, tau, windowed)
            lim_of = (lambda best: torch.clamp(best + tau, min=0.0)) if miss_argmin else (lambda best: torch.zeros_like(best))
            # (front_only of the evaluated first stage: a surely negative first-stage sample inside the mask)
            pos = torch.tensor(model.share.stage1_pos(vk.shape[1]), device=dev)
            neg1 = vk[:, pos] < -tau
            j1 = torch.where(neg1.any(1), pos[neg1.float().argmax(1)], torch.full_like(k, vk.shape[1] - 1))
            front = ok & neg1.any(1) & ~(vk[:, 0] < tau)
            lim_rows = lambda best: torch.where(front, torch.zeros_like(best), lim_of(best))
            depth = c['lin'][None, :] * (t_e - t_s)[sel][k][:, None]
            keep = model.staged_today(vk, depth, lip, lim_rows, torch.where(front, j1, torch.full_like(j1, vk.shape[1] - 1)), tau)
            staged = model.evaluations(keep)
            if training and inside:
                # built (nefii_trace_grid.training): the argmin is read (miss_argmin), the leading chunk stays in front;
                # `today` is what NEFII_BOUND_GRID_TRAINING=0 leaves - the quarter-row windows
                what += ' (training: from the grid)'
            elif training:
                today = staged          # out-of-mask training rays run the evaluated first stage, and keep it: report only
                what += ' (training: report only)'
            per, aud, per_c, aud_c = {}, {}, {}, {}
            for G in sizes:
                lo_s, hi_s = model.gather(grids[G][0], grids[G][1], pts[k], radius)
                lo_c, hi_c = corners.corner_gather(grids[G][2], grids[G][3], pts[k], radius, tau)
                keep_c, keep, looked = corners.bracket_walk(lo_s, hi_s, lo_c, hi_c, ok, miss_argmin, tau)
                per_c[G] = model.evaluations(keep_c) - torch.where(gate[k], keep_c[:, :CHUNK].sum(1), torch.zeros_like(k))
                aud_c[G] = model.audit(vk, keep_c, *corners.combine(lo_s, hi_s, lo_c, hi_c), tau)
                masked = torch.where(keep_c, vk, torch.full_like(vk, model.INF))
                assert (model._first(masked < -tau) == model._first(vk < -tau)).all(), 'a surely negative first sample moved (corners)'
                print('      G %d: corner look-ups per search %.1f' % (G, looked.float().mean()))
                del lo_c, hi_c
                # leading exact samples of chunk rays are not evaluated again
                per[G] = model.evaluations(keep) - torch.where(gate[k], keep[:, :CHUNK].sum(1), torch.zeros_like(k))
                aud[G] = model.audit(vk, keep, lo_s, hi_s, tau)
                masked = torch.where(keep, vk, torch.full_like(vk, model.INF))
                assert (model._first(masked < -tau) == model._first(vk < -tau)).all(), 'a surely negative first sample moved'
            report(what, k.numel(), today, staged, per, aud, per_c, aud_c)
        del pts, v
        # ---- min-SDF searches
        if training and c['steps'] is not None:
            searching = sph & ~samp & (~obj | ~hit)
            steps = c['steps'].reshape(-1)[:c['lin'].numel()].to(dev)
            order = torch.argsort(steps, stable=True)
            leaders = None
            for what, pick in (('min-SDF, own first stage (leaders, fall-backs)', searching & own), ('min-SDF, followers (keep the donor\'s row)', searching & ~own)):
                k = pick.nonzero().flatten()
                if k.numel() == 0:
                    continue
                if 'followers' in what:
                    print('  %-58s %7d searches, unchanged' % (what, k.numel()))
                    if leaders is not None:
                        followers_on_sparser_rows(pm, c, k, leaders, steps[order], t_min, t_max, lip, tau, grids[max(sizes)], radius, max(sizes))
                    continue
                pts, v = rows_of(pm, c['o'][k], c['d'][k], t_min[k], t_max[k], steps[order])
                depth = steps[order][None, :] * (t_max - t_min)[k][:, None]
                keep_today = model.staged_today(v, depth, lip, lambda best: best + tau, None, tau)
                today = model.evaluations(keep_today)
                per, aud, per_c, aud_c = {}, {}, {}, {}
                for G in sizes:
                    lo_s, hi_s = model.gather(grids[G][0], grids[G][1], pts, radius)
                    lo_c, hi_c = corners.corner_gather(grids[G][2], grids[G][3], pts, radius, tau)
                    keep_c, _ = corners.minsdf_walk(lo_s, hi_s, lo_c, hi_c, tau)
                    per_c[G] = model.evaluations(keep_c)
                    aud_c[G] = model.audit(v, keep_c, *corners.combine(lo_s, hi_s, lo_c, hi_c), tau)
                    masked = torch.where(keep_c, v, torch.full_like(v, model.INF))
                    assert ((masked.min(1).values - v.min(1).values).abs() <= 0).all(), 'the minimum was skipped (corners)'
                    del lo_c, hi_c
                    keep = model.minsdf_walk(lo_s, hi_s, tau)
                    per[G] = model.evaluations(keep)
                    aud[G] = model.audit(v, keep, lo_s, hi_s, tau)
                    masked = torch.where(keep, v, torch.full_like(v, model.INF))
                    assert ((masked.min(1).values - v.min(1).values).abs() <= 0).all(), 'the minimum was skipped'
                report(what, k.numel(), today, None, per, aud, per_c, aud_c)
                leaders = dict(k=k, v=v, pts=pts, keep_today=keep_today, keep_new=keep_c)       # (keep_c: the largest grid's, with corners)
    print('rays ended before they are traced:')
    for ci, c in enumerate(calls):
        if c['training']:
            print('call %d:' % ci)
            certified_crossings(net, pm, c, radius, sizes[0])
        elif c['unread']:
            print('call %d:' % ci)
            freed_misses(net, pm, c, radius, sizes[0])
    print('per step, the searches above: %.2f M single-pass evaluations today' % (total_today / 1e6))
    for G in sizes:
        print('  G %3d: %.2f M, saved %.2f M (%.0f %%)' % (G, total_grid[G] / 1e6, (total_today - total_grid[G]) / 1e6,
                                                         100.0 * (total_today - total_grid[G]) / max(total_today, 1)))
        print('         with the corner bounds %.2f M, saved %.2f M (%.0f %%)' % (
            total_corner[G] / 1e6, (total_today - total_corner[G]) / 1e6, 100.0 * (total_today - total_corner[G]) / max(total_today, 1)))


if __name__ == '__main__':
    main()
