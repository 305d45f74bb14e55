"""Bounds from a cell's corners for the SDF interval grid (include/nefii_amd.h: nefii_sdf_bound_grid_build_vertices,
nefii_trace_grid.vertex_g / .cell_l) on the GPU: the build against its torch restatement
(tests/test_bound_vertices_cpu.py) and against exact SDF values, and the eval-mode traces that bound the samples their cell
intervals leave from the corners - points, hit mask and depths bit-identical to the trace with the cells alone, without the grid
and without any staging, no more single-pass evaluations, a silent audit; on the batches of tests/test_gpu_bound_grid.py."""
import functools

import pytest
import torch

from nefii_amd import _lib, ops, synthetic as syn
from trace_cmp import build_sdf

import test_bound_grid_cpu as cells_model
import test_bound_vertices_cpu as model
import test_gpu_bound_grid as grid
import test_gpu_minsdf_share as share

pytestmark = pytest.mark.gpu

DEV = grid.DEV
G = 64


def _trace(mc, pm, o, d, om, training, steps, tau, lip, tier=0, cells=None, verts=None, group=0):
    tp = ops.make_tracer_params(mc['ray_tracer'], training, 'f16x3w', coarse_tau=tau, minsdf_lipschitz=lip, trace_tier=tier,
                                minsdf_group=group)
    lin = torch.linspace(0, 1, steps=tp.n_steps).to(DEV)
    return ops.trace_rays(pm, tp, o.to(DEV).contiguous(), d.to(DEV).contiguous(), om.to(DEV), lin, steps.to(DEV),
                          want_counters=True, bound_grid=cells, bound_vertices=verts)


@functools.lru_cache(maxsize=None)
def _bowl():
    """test_gpu_bound_grid's trained bowl and its cells at G = 64, with the vertex arrays of the same build"""
    mc, pm, tau, lip, cells_only = grid._bowl()
    cells, verts = ops.build_bound_grid(pm, 1.0, tau, G, vertices=True)
    assert torch.equal(cells, cells_only), 'the cells of the two build entry points differ'
    return mc, pm, tau, lip, cells, verts


def _evals(c):
    return ops.executed_evals(c, 100)[1].sum().item()


def test_build_matches_the_restatement_and_bounds_the_sdf():
    mc, pm, tau, lip, cells, (vert_g, cell_l) = _bowl()
    assert vert_g.shape == (G + 1,) * 3 and vert_g.dtype == torch.float16 and cell_l.shape == (G,) * 3 and cell_l.dtype == torch.float16
    g = ops.sdf_eval(pm, cells_model.grid_vertices(G, 1.0, DEV).contiguous(), coarse=True).cpu().reshape(G + 1, G + 1, G + 1)
    lo, hi, g16, l16 = model.build(g, 1.0, tau, ops.BOUND_GRID_L_FLOOR, ops.BOUND_GRID_SAFETY)
    vg, cl = vert_g.cpu(), cell_l.cpu()
    dg = int((vg.view(torch.int16) != g16.view(torch.int16)).sum())
    dl = int((cl.view(torch.int16) != l16.view(torch.int16)).sum())
    print('[bound vertices build] G %d, tau %.2e: slope bounds %.2f .. %.2f; entries that differ from the restatement: values %d, slopes %d' % (
        G, tau, float(cl.float().min()), float(cl.float().max()), dg, dl))
    assert dg == 0 and dl == 0
    x = (torch.rand(20000, 3, generator=torch.Generator().manual_seed(4)) * 2.0 - 1.0)
    exact = ops.sdf_eval(pm, x.to(DEV).contiguous()).cpu()
    words = cells.cpu()
    lo_k = (words & 0xFFFF).to(torch.int16).view(torch.float16)
    hi_k = ((words >> 16) & 0xFFFF).to(torch.int16).view(torch.float16)
    lo_s, hi_s = model.combine(*cells_model.gather(lo_k, hi_k, x, 1.0), *model.corner_gather(vg, cl, x, 1.0, tau))
    print('[bound vertices build] 20000 exact values: tightest margins lo %.3e, hi %.3e; mean half-width %.4f' % (
        float((exact - lo_s).min()), float((hi_s - exact).min()), float((hi_s - lo_s).mean() / 2)))
    assert (lo_s <= exact).all() and (exact <= hi_s).all()


def _check_modes(what, o, d, om, steps, group=0, must_fall=False):
    """corners / cells only / no grid / no staging at all: the same outputs; -> single-pass evaluations (cells only, corners)
    of the eval-mode traces"""
    mc, pm, tau, lip, cells, verts = _bowl()
    fell = []
    for training in (False, True):
        for tier in (0, 1):
            plain = _trace(mc, pm, o, d, om, training, steps, tau, 0.0, tier, group=group)
            off = _trace(mc, pm, o, d, om, training, steps, tau, lip if training else 0.0, tier, group=group)
            only = _trace(mc, pm, o, d, om, training, steps, tau, lip, tier, cells=cells, group=group)
            got = _trace(mc, pm, o, d, om, training, steps, tau, lip, tier, cells=cells, verts=verts, group=group)
            for k, out in enumerate(('points', 'hit mask', 'depths')):
                assert torch.equal(got[k], only[k]), (what, training, tier, out, 'against the cells alone')
                assert torch.equal(got[k], off[k]), (what, training, tier, out, 'against the trace without the grid')
                assert torch.equal(got[k], plain[k]), (what, training, tier, out, 'against the unstaged trace')
            assert grid._audit(got[3]) == 0.0, (what, training, tier, grid._audit(got[3]))
            c0, c1 = only[3].cpu().long(), got[3].cpu().long()
            if training:      # training-mode traces do not read the grid: nothing changes
                assert torch.equal(c0, c1), (what, tier)
                continue
            e0, e1 = _evals(c0), _evals(c1)
            print('[bound vertices %s eval tier=%d] %d rays, %d bracket searches: single-pass evaluations %d -> %d, survivors %d -> %d, '
                  'probes %d -> %d' % (what, tier, o.shape[0], c0[:, _lib.CNT_SEARCHES].sum().item(), e0, e1,
                                       c0[:, _lib.CNT_COARSE_SAMPLES].sum().item(), c1[:, _lib.CNT_COARSE_SAMPLES].sum().item(),
                                       c0[:, _lib.CNT_PROBES].sum().item(), c1[:, _lib.CNT_PROBES].sum().item()))
            assert c1[:, _lib.CNT_SEARCHES].sum() == c0[:, _lib.CNT_SEARCHES].sum()
            assert e1 <= e0, (what, tier, e0, e1)
            fell.append((e0, e1))
    if must_fall:
        assert all(e1 < e0 for e0, e1 in fell), fell
    return fell


def test_corners_change_no_output_on_the_share_cases():
    for name, (o, d, om, steps, group, _) in share._cases().items():
        if name == 'copies64':
            continue
        _check_modes(name, o, d, om, steps, group)


def test_corners_change_no_output_on_secondary_rays():
    o, d = grid._secondary()
    _check_modes('secondary', o, d, torch.ones(o.shape[0], dtype=torch.bool), torch.rand(100), must_fall=True)


@pytest.mark.parametrize('n', [1, 255, 256, 257])
def test_corners_change_no_output_around_a_block_of_rays(n):
    """one ray, and one ray less than, exactly and one more than advance_kernel's block of 256"""
    o, d = grid._secondary()
    _check_modes('secondary[:%d]' % n, o[7:7 + n], d[7:7 + n], torch.ones(n, dtype=torch.bool), torch.rand(100))


def test_ray_leaving_the_cube_by_rounding():
    """test_gpu_bound_grid's rays along the cube's faces: samples on and past the faces have no corner bound either"""
    o, d = [], []
    for ax in range(3):
        for sign in (1.0, -1.0):
            for t in range(2):
                p = torch.zeros(3)
                p[ax] = sign * 0.99999994
                q = torch.zeros(3)
                q[(ax + 1 + t) % 3] = 1.0
                o.append(p - 0.5 * q * 1e-3)
                d.append(q)
    ro, rd = share._random(52, 3)
    o, d = torch.cat([torch.stack(o), ro]), torch.cat([torch.stack(d), rd])
    _check_modes('cube faces', o, d, torch.ones(o.shape[0], dtype=torch.bool), torch.rand(100))


def test_corners_on_the_dent():
    """test_grid_on_the_dent's pocket, bundles, tau and L at G = 256 with the corner bounds on: every bundle bit-identical to the
    full search, no bundle size missing silently.  The pocket (radius 0.01) is little wider than a cell (7.8 mm): the differences
    over the edges around it understate the slope inside (they are means over an edge), and what makes the cell's slope bound
    cover it is the term u_a - d_a - how much the means of neighbouring edges differ (tests/test_bound_vertices_cpu.py); without
    it the audit fired in 25 of these 170 traces."""
    from test_gpu_kernels import _bundle_through, _dent_scene
    mc, sd, c = _dent_scene()
    pm, pm32 = build_sdf(mc, sd, f16x3=True), build_sdf(mc, sd)
    tau = ops.calibrate_coarse_tau(pm)
    lip = ops.calibrate_lipschitz(lambda x: ops.sdf_value_grad(pm32, x)[2], DEV)
    cells, verts = ops.build_bound_grid(pm, 1.0, tau, 256, l_floor=lip, vertices=True)
    cd = c.to(DEV)
    steps = torch.rand(100)
    table = []
    for n, reps in ((4096, 2), (256, 8), (64, 16), (16, 32), (4, 48), (1, 64)):
        silent = detected = same = differing = pocket = 0
        for rep in range(reps):
            o, d = _bundle_through(c, n, 100 * n + rep)
            om = torch.ones(n, dtype=torch.bool)
            base = _trace(mc, pm, o, d, om, False, steps, tau, 0.0)
            got = _trace(mc, pm, o, d, om, False, steps, tau, lip, cells=cells, verts=verts)
            viol = grid._audit(got[3])
            diff = int(((got[2] != base[2]) | (got[1] != base[1])).sum())
            pocket += int(((base[0] - cd).abs().sum(1) < 0.012).sum())
            differing += diff
            if diff == 0:
                same += 1
            elif viol > 0:
                detected += 1
            else:
                silent += 1
        table.append((n, reps, same, detected, silent, differing, pocket))
        print('[bound vertices dent] bundles of %4d rays x %2d: bit-identical %2d, audit fired %2d, SILENT miss %2d (rays that differ %d, '
              'rays the full search ends in the pocket %d)' % table[-1])
    assert table[0][6] > 0.1 * 4096 * 2, table
    assert all(t[4] == 0 for t in table), table
    assert all(t[2] == t[1] for t in table), table


def test_model_bounds_from_the_corners_by_default(monkeypatch):
    """RayTracing.forward in eval mode under frozen geometry: both arrays are built with the cells, kept with the packed weights
    and read by default; NEFII_BOUND_GRID_VERTICES=0 leaves the cells alone; the outputs do not change."""
    from nefii_amd import conf
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    mc = syn.model_conf('conf')
    sd = syn.make_state_dict(mc, seed=2, scene='bowl_trained')
    o, d = grid._secondary()
    n = o.shape[0]
    res = {}
    for mode in ('corners', 'cells'):
        monkeypatch.setenv('NEFII_BOUND_GRID_VERTICES', '1' if mode == 'corners' else '0')
        m = IDRNetwork(conf.from_dict(mc))
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV)
        m.freeze_geometry()
        m.eval()
        rt = m.ray_tracer
        assert rt.bound_grid_vertices == (mode == 'corners')
        rt.bound_grid_size = G
        rt.collect_counters = True

        def run():
            with torch.no_grad():
                return rt(sdf=m.implicit_network, cam_loc=o.to(DEV), object_mask=torch.ones(n, dtype=torch.bool, device=DEV),
                          ray_directions=d.to(DEV).reshape(n, 1, 3))
        res[mode] = run()
        kept = m.implicit_network._grid
        assert kept is not None and (kept[5] is not None) == (mode == 'corners'), mode
        assert rt.retraced_calls == 0 and not m.implicit_network.coarse_audit_events
        res[mode] += (rt.last_counters.cpu().long(),)
        run()
        again = m.implicit_network._grid
        assert again[4] is kept[4] and again[5] is kept[5], 'the grid was rebuilt for unchanged weights'
        if mode == 'corners':
            with pytest.warns(UserWarning):
                m.implicit_network.note_lipschitz_audit(1.0, m.implicit_network.minsdf_lipschitz(1.0))
            assert m.implicit_network._grid is None, 'a failed slope audit keeps the arrays'
    for k in range(3):
        assert torch.equal(res['corners'][k], res['cells'][k]), k
    e = {mode: _evals(res[mode][3]) for mode in res}
    print('[bound vertices model] single-pass evaluations: corners %d, NEFII_BOUND_GRID_VERTICES=0 %d' % (e['corners'], e['cells']))
    assert e['corners'] < e['cells']
