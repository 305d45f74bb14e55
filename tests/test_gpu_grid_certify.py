"""Rays the SDF interval grid proves to miss, ended before they are traced (include/nefii_amd.h: nefii_sdf_bound_grid_blocks,
nefii_trace_grid.certify; DESIGN section 4h, "certificates") on the GPU.  A training-mode ray whose two fronts the
grid's block level proves to cross within sphere_tracing_iters goes to its min-SDF search in round 0: points, hit mask and
depths bit-identical with the flag on and off, fewer sphere-tracing queries, a certified count above 0 and below the misses,
a silent audit.  An eval-mode trace with unread misses ends the rays whose remaining stretch the grid proves free: the hit mask
and every hit output identical; one whose misses are read is not changed: every output and every counter.  Intervals that do
not hold make the audit fire and the model re-trace.  On the adversarial dent no
bundle may differ from the uncertified trace without the audit having fired.  The block build against a torch min-pool bit
for bit.  On the model level: RayTracing.bound_grid_certify / NEFII_BOUND_GRID_CERTIFY, grouped traces, and a TrainStep run under
the protocol of tests/test_gpu_grid_training.py.  tests/test_grid_certify_cpu.py holds the rule itself to the reference's
sphere tracing."""
import functools

import pytest
import torch

from nefii_amd import _lib, conf, ops, synthetic as syn
from trace_cmp import build_sdf

import test_gpu_bound_grid as grid
import test_gpu_bound_vertices as vertices
import test_gpu_grid_training as gt
import test_gpu_minsdf_share as share

pytestmark = pytest.mark.gpu

DEV = grid.DEV
G = vertices.G
SIZES = [1, 63, 64, 65, 257, 4096]
F_CERT = 1 << 7          # csrc/nefii_tracer.hip: the flag word's bit of a ray the certificate ended


def _trace(mc, pm, o, d, om, steps, tau, lip, tier=0, cells=None, verts=None, blocks=None, training=True, unread_misses=0,
           n_steps=None, keep=None, parts=3):
    """-> (points, hit, depths, counters, [certified rays, block look-ups])"""
    cfg = dict(mc['ray_tracer'])
    if n_steps:
        cfg['n_steps'] = n_steps
    tp = ops.make_tracer_params(cfg, training, 'f16x3w', coarse_tau=tau, minsdf_lipschitz=lip, trace_tier=tier,
                                unread_misses=unread_misses)
    lin = torch.linspace(0, 1, steps=tp.n_steps).to(DEV)
    counts = torch.zeros(ops.CERTIFY_COUNTS, device=DEV, dtype=torch.int32)
    out = ops.trace_rays(pm, tp, o.to(DEV).contiguous(), d.to(DEV).contiguous(), om.to(DEV), lin, steps.to(DEV),
                         want_counters=True, bound_grid=cells, bound_vertices=verts, bound_grid_training=training and cells is not None,
                         bound_grid_certify=blocks, certify_counts=counts, keep_workspace=keep, certify_parts=parts)
    return out + (counts.cpu().tolist(),)


@functools.lru_cache(maxsize=None)
def _bowl():
    mc, pm, tau, lip, cells, verts = vertices._bowl()
    return mc, pm, tau, lip, cells, verts, ops.build_bound_grid_blocks(cells)


def _certified_mask(kept):
    out = []
    for ws, _lo, n in kept:
        stride = (4 * n + 255) // 256 * 256
        begin = _lib.TRACE_WS_FLOAT_ARRAYS * stride
        out.append((ws[begin:begin + 4 * n].view(torch.int32) & F_CERT) != 0)
    return torch.cat(out).cpu()


@functools.lru_cache(maxsize=None)
def _rays():
    """4096 rays from outside the bounding sphere aimed around the bowl (it ends inside radius 0.6): hits, misses that graze it,
    wide misses, rays that miss the sphere; 15 % outside the object mask.  Ray 0 is one the certificate ends (the batch of one ray
    then checks something), ray 1 one that misses without being certified."""
    mc, pm, tau, lip, cells, verts, blocks = _bowl()
    o, d = share._random(4096, 51, spread=0.8)
    g = torch.Generator().manual_seed(52)
    om, steps = torch.rand(4096, generator=g) < 0.85, torch.rand(100, generator=g)
    kept = []
    res = _trace(mc, pm, o, d, om, steps, tau, lip, 0, cells, verts, blocks, keep=kept)
    cert = _certified_mask(kept)
    assert int(cert.sum()) == res[4][0] > 0, (int(cert.sum()), res[4])
    plain_miss = ~cert & ~res[1].cpu()
    order = torch.arange(4096)
    first = int(torch.nonzero(cert).flatten()[0])
    order[[0, first]] = order[[first, 0]]
    other = 1 + int(torch.nonzero(plain_miss[order][1:]).flatten()[0])
    order[[1, other]] = order[[other, 1]]
    return o[order], d[order], om[order], steps


def _queries(c):
    """sphere-tracing queries of both evaluators"""
    c = c.cpu().long()
    return int(c[:, _lib.CNT_COARSE_SINGLES].sum() + c[:, _lib.CNT_SINGLES].sum())


@pytest.mark.parametrize('n_steps', [100, 40])
@pytest.mark.parametrize('tier', [0, 1])
@pytest.mark.parametrize('n', SIZES)
def test_training_traces_do_not_move_by_a_bit(n, tier, n_steps):
    """the first n of the 4096 rays.  0 < certified < misses wherever a batch can satisfy it; the batch of one ray is ray 0,
    which the certificate ends: certified == misses == 1 there"""
    mc, pm, tau, lip, cells, verts, blocks = _bowl()
    o, d, om, steps = _rays()
    o, d, om, steps = o[:n], d[:n], om[:n], steps[:n_steps]
    off = _trace(mc, pm, o, d, om, steps, tau, lip, tier, cells, verts, None, n_steps=n_steps)
    on = _trace(mc, pm, o, d, om, steps, tau, lip, tier, cells, verts, blocks, n_steps=n_steps)
    for k, out in enumerate(('points', 'hit mask', 'depths')):
        assert torch.equal(on[k], off[k]), out
    misses = int((~off[1]).sum())
    print('[grid certify n=%d tier=%d n_steps=%d] misses %d, certified %d, block look-ups %d; sphere-tracing queries %d -> %d' % (
        n, tier, n_steps, misses, on[4][0], on[4][1], _queries(off[3]), _queries(on[3])))
    assert off[4] == [0] * ops.CERTIFY_COUNTS
    assert grid._audit(on[3]) == 0.0, grid._audit(on[3])
    assert _queries(on[3]) < _queries(off[3])
    if n == 1:
        assert on[4][0] == misses == 1
    else:
        assert 0 < on[4][0] < misses, (on[4], misses)


@pytest.mark.parametrize('unread', [1, 0])
def test_eval_mode_traces(unread):
    """eval-mode traces with rays started 0.01 off the surface.  Misses unread (the secondary trace): the free-stretch
    certificate ends rays - the hit mask identical, points and depths identical wherever hit, everything finite, fewer
    sphere-tracing queries, a silent audit with probes sent.  Misses read (renders): the flag changes no output and no counter"""
    mc, pm, tau, lip, cells, verts, blocks = _bowl()
    so, sd = grid._secondary()
    so = so + 0.01 * sd
    om = torch.ones(so.shape[0], dtype=torch.bool)
    steps = torch.rand(100, generator=torch.Generator().manual_seed(3))
    off = _trace(mc, pm, so, sd, om, steps, tau, lip, 0, cells, verts, None, training=False, unread_misses=unread)
    on = _trace(mc, pm, so, sd, om, steps, tau, lip, 0, cells, verts, blocks, training=False, unread_misses=unread)
    assert torch.isfinite(on[0]).all() and torch.isfinite(on[2]).all()
    if unread:
        hit = off[1]
        assert torch.equal(on[1], hit) and torch.equal(on[0][hit], off[0][hit]) and torch.equal(on[2][hit], off[2][hit])
        print('[grid certify eval] %d rays, %d miss; ended as free %d, look-ups %d; sphere-tracing queries %d -> %d; probes %d -> %d' % (
            hit.numel(), int((~hit).sum()), on[4][2], on[4][3], _queries(off[3]), _queries(on[3]),
            int(off[3][:, _lib.CNT_PROBES].sum()), int(on[3][:, _lib.CNT_PROBES].sum())))
        assert on[4][:2] == [0, 0] and 0 < on[4][2] <= int((~hit).sum())
        assert _queries(on[3]) < _queries(off[3])
        assert grid._audit(on[3]) == 0.0
        only_cross = _trace(mc, pm, so, sd, om, steps, tau, lip, 0, cells, verts, blocks, training=False, unread_misses=1, parts=1)
        assert torch.equal(only_cross[3], off[3]) and only_cross[4] == [0] * ops.CERTIFY_COUNTS
    else:
        for k in range(4):
            assert torch.equal(on[k], off[k]), k
        assert on[4] == [0] * ops.CERTIFY_COUNTS


def _min_pool(cells, b=ops.BOUND_GRID_BLOCK):
    g = cells.shape[0]
    gb = -(-g // b)
    lo = (cells & 0xFFFF).to(torch.int16).view(torch.float16).float()
    pad = torch.full((gb * b,) * 3, float('inf'), device=cells.device)
    pad[:g, :g, :g] = lo
    return pad.reshape(gb, b, gb, b, gb, b).amin(dim=(1, 3, 5)).half()


@pytest.mark.parametrize('g', [64, 66, 10, 5])
def test_block_build_is_the_min_pool(g):
    """the bowl's cells at G = 64, and random cells at sizes the block does and does not divide"""
    if g == G:
        cells = _bowl()[4]
    else:
        gen = torch.Generator().manual_seed(g)
        lo = (torch.randn(g, g, g, generator=gen) * 0.3).half().view(torch.int16).int() & 0xFFFF
        hi = (torch.randn(g, g, g, generator=gen) * 0.3 + 1.0).half().view(torch.int16).int() & 0xFFFF
        cells = (lo | (hi << 16)).to(torch.int32).to(DEV)
    blocks = ops.build_bound_grid_blocks(cells)
    want = _min_pool(cells)
    assert blocks.shape == want.shape == (-(-g // ops.BOUND_GRID_BLOCK),) * 3 and blocks.dtype == torch.float16
    assert torch.equal(blocks.view(torch.int16), want.view(torch.int16))


def _past_the_pocket(c, n, seed, jitter=0.003):
    """rays through the pocket ACROSS the line from the object's centre: most of them pass the pocket and miss the object"""
    g = torch.Generator().manual_seed(seed)
    p = c[None] + torch.randn(n, 3, generator=g) * jitter
    t = torch.linalg.cross(c[None].expand(n, 3), torch.randn(n, 3, generator=g))
    t = t / t.norm(dim=1, keepdim=True)
    return p - 1.8 * t, t


@pytest.mark.parametrize('scene', ['scaled', 'unscaled'])
def test_on_the_dent(scene):
    """test_grid_on_the_dent's pocket, tau, L and grid (G = 256): bundles aimed through the pocket at the object, bundles that
    pass through it across the object and bundles that pass up to 0.15 beside it, training mode and eval mode with unread
    misses.  Every trace equals the uncertified one or has raised the audit; a difference with a silent audit is counted, and
    there is none.  'scaled' is that test's field as it is: an under-estimated distance (|grad| 0.3), on which only rays far
    from the object cross in ten iterations.  'unscaled' keeps the distance (|grad| 1) and deepens the pocket to 0.06, negative
    within 3 mm of its centre: rays beside it are certified, rays through it must not be."""
    from test_gpu_kernels import _bundle_through, _dent_scene
    mc, sd, c = _dent_scene() if scene == 'scaled' else _dent_scene(value_scale=1.0, depth=0.06)
    pm, pm32 = build_sdf(mc, sd, f16x3=True), build_sdf(mc, sd)
    tau = ops.calibrate_coarse_tau(pm)
    lip = ops.calibrate_lipschitz(lambda x: ops.sdf_value_grad(pm32, x)[2], DEV)
    cells, verts = ops.build_bound_grid(pm, 1.0, tau, 256, l_floor=lip, vertices=True)
    blocks = ops.build_bound_grid_blocks(cells)
    steps = torch.rand(100, generator=torch.Generator().manual_seed(2))
    table = []
    for training in (True, False):
        for n, reps in ((4096, 3), (256, 6), (64, 6), (16, 6), (4, 6), (1, 6)):
            silent = detected = same = certified = misses = 0
            for rep in range(reps):
                o, d = (_bundle_through(c, n, 100 * n + rep), _past_the_pocket(c, n, 100 * n + rep),
                        _past_the_pocket(c, n, 100 * n + rep, jitter=0.15))[rep % 3]
                om = torch.ones(n, dtype=torch.bool)
                kw = dict(training=training, unread_misses=0 if training else 1)
                base = _trace(mc, pm, o, d, om, steps, tau, lip, 0, cells, verts, None, **kw)
                got = _trace(mc, pm, o, d, om, steps, tau, lip, 0, cells, verts, blocks, **kw)
                if training:
                    diff = int(((got[2] != base[2]) | (got[1] != base[1]) | (got[0] != base[0]).any(1)).sum())
                else:       # nobody reads a miss of this trace
                    diff = int(((got[1] != base[1]) | ((got[2] != base[2]) & base[1])).sum())
                certified += got[4][0] + got[4][2]
                misses += int((~base[1]).sum())
                if diff == 0:
                    same += 1
                elif grid._audit(got[3]) > 0:
                    detected += 1
                else:
                    silent += 1
            table.append((training, n, reps, same, detected, silent, certified, misses))
            print('[grid certify dent, %s] training %d, bundles of %4d rays x %d: equal %d, audit fired %d, SILENT %d (certified %d of '
                  '%d misses)' % ((scene,) + table[-1]))
    assert all(t[5] == 0 for t in table), table
    assert table[6][6] > 0, 'no eval-mode ray was ended as free: the case checks nothing'
    assert table[0][6] > 0, 'no ray was certified: the case checks nothing'


def _model(monkeypatch, on):
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    # ('2': counted traces certify too - RayTracing leaves the certificate out of a trace whose counters are collected)
    monkeypatch.setenv('NEFII_BOUND_GRID_CERTIFY', '2' if on else '0')
    monkeypatch.setenv('NEFII_BOUND_GRID_CERTIFY_EVAL', '1' if on else '0')        # (the eval-mode part is off by default)
    mc = syn.model_conf('conf')
    sd = syn.make_state_dict(mc, seed=2, scene='bowl_trained')
    m = IDRNetwork(conf.from_dict(mc))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m.freeze_geometry()
    m.train()
    assert m.ray_tracer.bound_grid_certify and not m.ray_tracer.bound_grid_certify_eval and m.ray_tracer.bound_grid_training
    m.ray_tracer.bound_grid_size = G
    m.ray_tracer.collect_counters = True
    m.ray_tracer.certify_counts = torch.zeros(ops.CERTIFY_COUNTS, device=DEV, dtype=torch.int32)
    return m


@pytest.mark.parametrize('miss_search', [True, False])
def test_model_switch(miss_search, monkeypatch):
    """RayTracing.forward in training mode under frozen geometry certifies by default, NEFII_BOUND_GRID_CERTIFY=0 (read per
    call) leaves the traces as they were; with miss_search off (an eval-mode trace) the switch changes nothing"""
    o, d, om, steps = _rays()
    n = o.shape[0]
    res = {}
    for on in (True, False):
        m = _model(monkeypatch, on)
        rt = m.ray_tracer
        rt.miss_search = miss_search
        rt.minsdf_steps_override = steps
        with torch.no_grad():
            out = rt(sdf=m.implicit_network, cam_loc=o.to(DEV), object_mask=om.to(DEV), ray_directions=d.to(DEV).reshape(n, 1, 3))
        assert rt.retraced_calls == 0 and not m.implicit_network.coarse_audit_events
        res[on] = out + (rt.last_counters.cpu(), rt.certify_counts.cpu().tolist())
    hit = res[False][1]
    keep = torch.ones_like(hit) if miss_search else hit        # (miss_search off: nobody reads a miss)
    assert torch.equal(res[True][1], hit)
    for k in (0, 2):
        assert torch.equal(res[True][k][keep], res[False][k][keep]), k
        assert torch.isfinite(res[True][k]).all()
    assert grid._audit(res[True][3]) == 0.0 and res[False][4] == [0] * ops.CERTIFY_COUNTS
    assert _queries(res[True][3]) < _queries(res[False][3])
    if miss_search:
        assert res[True][4][0] > 0 and res[True][4][2] == 0
    else:
        assert res[True][4][0] == 0 and res[True][4][2] > 0
        # the part's own switch
        monkeypatch.setenv('NEFII_BOUND_GRID_CERTIFY_EVAL', '0')
        rt.certify_counts.zero_()
        with torch.no_grad():
            out = rt(sdf=m.implicit_network, cam_loc=o.to(DEV), object_mask=om.to(DEV), ray_directions=d.to(DEV).reshape(n, 1, 3))
        assert rt.certify_counts.cpu().tolist() == [0] * ops.CERTIFY_COUNTS and torch.equal(rt.last_counters.cpu(), res[False][3])
        assert all(torch.equal(out[k], res[False][k]) for k in range(3))


def test_counted_traces_trace_every_ray(monkeypatch):
    """the default (NEFII_BOUND_GRID_CERTIFY unset): a trace whose counters are collected is read as the reference's
    recurrences and certifies nothing - its counters are those of the switch off; the same trace without counters certifies;
    same outputs"""
    o, d, om, steps = _rays()
    n = o.shape[0]
    m = _model(monkeypatch, False)
    rt = m.ray_tracer
    rt.minsdf_steps_override = steps
    res = {}
    for mode, counted in (('0', True), (None, True), (None, False)):
        if mode is None:
            monkeypatch.delenv('NEFII_BOUND_GRID_CERTIFY', raising=False)
        else:
            monkeypatch.setenv('NEFII_BOUND_GRID_CERTIFY', mode)
        rt.collect_counters = counted
        rt.certify_counts.zero_()
        with torch.no_grad():
            out = rt(sdf=m.implicit_network, cam_loc=o.to(DEV), object_mask=om.to(DEV), ray_directions=d.to(DEV).reshape(n, 1, 3))
        res[(mode, counted)] = out + (rt.last_counters.cpu() if counted else None, rt.certify_counts.cpu().tolist())
    assert rt.retraced_calls == 0 and not m.implicit_network.coarse_audit_events
    for key in ((None, True), (None, False)):
        for k in range(3):
            assert torch.equal(res[key][k], res[('0', True)][k]), (key, k)
    assert torch.equal(res[(None, True)][3], res[('0', True)][3]) and res[(None, True)][4] == [0] * ops.CERTIFY_COUNTS
    assert res[(None, False)][4][0] > 0


def test_grouped_trace_equals_the_single_traces(monkeypatch):
    """two batches as one tracer call (RayTracing.steps_per_batch, TrainStep's grouped traces): each slice is that batch's own
    trace, certified rays in both"""
    _, _, om, _ = _rays()
    S = 1536
    m = _model(monkeypatch, True)
    rt = m.ray_tracer
    cams = torch.tensor([[0.2, 0.1, 2.0], [1.6, -0.3, 1.2]])
    dirs = torch.nn.functional.normalize(torch.randn(2, S, 3, generator=torch.Generator().manual_seed(5)) * 0.6 - cams[:, None], dim=-1)
    mask = om[:2 * S]

    def run(c, dd, mk, per_batch):
        torch.manual_seed(21)
        rt.steps_per_batch = per_batch
        try:
            with torch.no_grad():
                return rt(sdf=m.implicit_network, cam_loc=c.to(DEV), object_mask=mk.to(DEV), ray_directions=dd.to(DEV))
        finally:
            rt.steps_per_batch = False

    both = run(cams, dirs, mask, True)
    together = int(rt.certify_counts[0])
    assert together > 0, 'no ray was certified'
    torch.manual_seed(21)
    drawn = [torch.empty(100).uniform_(0.0, 1.0) for _ in range(2)]
    for b in range(2):
        rt.minsdf_steps_override = drawn[b]
        one = run(cams[b:b + 1], dirs[b:b + 1], mask[b * S:(b + 1) * S], False)
        for k in range(3):
            assert torch.equal(one[k], both[k][b * S:(b + 1) * S]), (b, k)
    rt.minsdf_steps_override = None
    assert int(rt.certify_counts[0]) == 2 * together, 'the single traces certify the rays the grouped trace did'
    assert rt.retraced_calls == 0 and not m.implicit_network.coarse_audit_events


def test_train_step_does_not_move_by_a_bit(monkeypatch):
    """tests/test_gpu_grid_training.py's TrainStep protocol (its docstring has the why) with NEFII_BOUND_GRID_CERTIFY: shrunk
    config 3, three steps with the next batch traced ahead; a run does not repeat itself bit for bit, so three runs with the
    switch off and one with it on.  Bit-identity between all four on every primary trace, the first secondary trace and the
    first loss; every parameter of the on run within 4 R of the nearest off run (R: the largest relative root-mean-square
    difference between two off runs on any tensor, not below that file's recorded 4.0e-5); the later losses within 4 x the
    off runs' own relative difference, not below 4 units in the last place."""
    from nefii_amd.training.step import TrainStep
    from test_gpu_configs import SHRUNK, build_model, to_dev
    w = syn.WORKLOADS['cfg3']
    lc = syn.loss_conf(w['model'])
    batches = [syn.make_inputs(SHRUNK['cfg3'], w['image_hw'], w['focal'], w['cam_pos'], w['num_rays'], seed=s) for s in (1, 2, 3)]
    n_primary = SHRUNK['cfg3'] * w['num_rays']
    res = {}
    for run in ('on',) + gt.OFF:
        monkeypatch.setenv('NEFII_BOUND_GRID_CERTIFY', '2' if run == 'on' else '0')
        monkeypatch.setenv('NEFII_BOUND_GRID_CERTIFY_EVAL', '1' if run == 'on' else '0')
        mc, sd = syn.workload_state_dict('cfg3', seed=0)
        m = build_model(mc, sd, True)
        assert m.ray_tracer.bound_grid_certify and not m.ray_tracer.trace_tier
        m.ray_tracer.bound_grid_size = G
        m.ray_tracer.collect_counters = True
        m.ray_tracer.certify_counts = torch.zeros(ops.CERTIFY_COUNTS, device=DEV, dtype=torch.int32)
        traces, tails, counters = [], [], []
        m.ray_tracer.register_forward_hook(lambda mod, args, out, traces=traces: traces.append(tuple(t.detach().clone() for t in out)))
        m.ray_tracer.register_forward_hook(lambda mod, args, out, counters=counters: counters.append(mod.last_counters))
        shade_tail = m.shade_tail

        def recording_tail(ctx, *a, shade_tail=shade_tail, tails=tails, **kw):
            tails.append((ctx['points'].detach().clone(), ctx['network_object_mask'].detach().clone()))
            return shade_tail(ctx, *a, **kw)
        m.shade_tail = recording_tail
        step = TrainStep(m, lc, secondary_train_interval=10, secondary_batch_size=1024, num_rays=w['num_rays'])
        torch.manual_seed(7)
        inputs = [to_dev(inp) for inp, _ in batches]
        losses = []
        for k in range(3):
            _, lo = step(inputs[k], {'rgb': batches[k][1].to(DEV)}, next_input=inputs[k + 1] if k < 2 else None)
            losses.append(lo['loss'].detach().clone())
        torch.cuda.synchronize()
        assert step.retraced_steps == 0 and not m.implicit_network.coarse_audit_events
        params = {k: v.detach().double().cpu() for k, v in m.state_dict().items() if v.dtype.is_floating_point}
        res[run] = (losses, tails + [t for t in traces if t[0].shape[0] != n_primary][:1], [c.cpu() for c in counters if c.shape[0] > 0],
                    params, m.ray_tracer.certify_counts.cpu().tolist())
    for other in gt.OFF:
        assert len(res['on'][1]) == 4 and len(res[other][1]) == 4, 'three primary traces and the first secondary one'
        for n, (a, b) in enumerate(zip(res['on'][1], res[other][1])):
            # (the secondary trace, the last entry: nothing reads its misses - its hit mask, and the rest under it)
            keep = a[1] if n == 3 else torch.ones_like(a[1] if len(a) > 2 else a[0][:, 0], dtype=torch.bool)
            for k in range(len(a)):
                assert a[k].shape == b[k].shape and torch.equal(a[k][keep] if n == 3 and k != 1 else a[k], b[k][keep] if n == 3 and k != 1 else b[k]), (other, n, k, a[k].shape)
        assert torch.equal(res['on'][0][0], res[other][0][0]), (other, res['on'][0][0].item(), res[other][0][0].item())
        assert res[other][4] == [0] * ops.CERTIFY_COUNTS
    p_on, p_off = res['on'][3], [res[r][3] for r in gt.OFF]
    pairs = [(a, b) for n, a in enumerate(p_off) for b in p_off[n + 1:]]
    rms = lambda x: float(x.pow(2).mean().sqrt())
    scale = {k: rms(p_off[0][k]) for k in p_on}
    spread = {k: max(rms(a[k] - b[k]) for a, b in pairs) for k in p_on}
    R_seen = max(spread[k] / scale[k] for k in p_on if scale[k] > 0)
    R = max(R_seen, gt.R_RECORDED)
    worst = (-1.0, '')
    for k in p_on:
        dist = min(rms(p_on[k] - q[k]) for q in p_off)
        if scale[k] > 0:
            worst = max(worst, (dist / scale[k], k))
        assert dist <= 4.0 * R * scale[k], (k, dist, spread[k], 4.0 * R * scale[k])
    l_on, l_off = [x.item() for x in res['on'][0]], [[x.item() for x in res[r][0]] for r in gt.OFF]
    r_loss = max(max(abs(a[k] - b[k]) / abs(a[k]) for k in range(3) for n, a in enumerate(l_off) for b in l_off[n + 1:]), 2.0 ** -23)
    for k in (1, 2):
        dist = min(abs(l_on[k] - q[k]) for q in l_off)
        assert dist <= 4.0 * r_loss * abs(l_off[0][k]), (k, l_on[k], [q[k] for q in l_off])
    assert all(grid._audit(c) == 0.0 for c in res['on'][2])
    q_on, q_off = (sum(_queries(c) for c in res[r][2]) for r in ('on', gt.OFF[0]))
    print('[grid certify step] 3 steps, losses on %s, off %s (bound: %.2e relative); largest relative rms difference between off runs '
          '%.3e (R not below %.1e), on against the nearest off run at most %.3e (%s), bound 4 R; certified rays %d, block look-ups %d; '
          'sphere-tracing queries of all traces %d -> %d' % (
              ['%.9g' % x for x in l_on], [['%.9g' % x for x in q] for q in l_off], 4.0 * r_loss, R_seen, gt.R_RECORDED, worst[0], worst[1],
              res['on'][4][0], res['on'][4][1], q_off, q_on))
    assert res['on'][4][0] > 0 and q_on < q_off, 'no training-mode trace certified a ray'


def _raised(cells, by):
    """the cells with every lo raised by `by`: intervals that do not hold"""
    lo = ((cells & 0xFFFF).to(torch.int16).view(torch.float16).float() + by).half().view(torch.int16).int() & 0xFFFF
    return ((cells.int() & ~0xFFFF) | lo).to(torch.int32)


def test_audit_fires_on_intervals_that_do_not_hold(monkeypatch):
    """lo raised by 0.1 in every cell: certificates are issued that the field does not back.  The min-SDF searches of the
    certified rays report it (NEFII_CNT_LIP_AUDIT > 0 in a trace whose every ray lies outside the mask and certifies or
    traces without a grid walk), and RayTracing.forward drops the grid and repeats the trace: retraced_calls == 1, outputs
    those of the uncertified trace"""
    mc, pm, tau, lip, cells, verts, blocks = _bowl()
    o, d, om, steps = _rays()
    bad = _raised(cells, 0.1)
    bad_blocks = ops.build_bound_grid_blocks(bad)
    miss = ~_trace(mc, pm, o, d, om, steps, tau, lip, 0, cells, verts, None)[1].cpu()
    oo, dd = o[miss], d[miss]
    outside = torch.zeros(int(miss.sum()), dtype=torch.bool)
    off = _trace(mc, pm, oo, dd, outside, steps, tau, lip, 0, bad, verts, None)
    on = _trace(mc, pm, oo, dd, outside, steps, tau, lip, 0, bad, verts, bad_blocks)
    assert grid._audit(off[3]) == 0.0, 'rays outside the mask do not read the cells without the certificate'
    assert on[4][0] > 0 and grid._audit(on[3]) > 0.0
    # the eval-mode part: the probes of the rays ended as free (one in 16) are held against the raised intervals
    so, sd = grid._secondary()
    so = so + 0.01 * sd
    ones = torch.ones(so.shape[0], dtype=torch.bool)
    kw = dict(training=False, unread_misses=1, parts=2)
    plain = _trace(mc, pm, so, sd, ones, steps, tau, lip, 0, bad, verts, None, **kw)
    probed = _trace(mc, pm, so, sd, ones, steps, tau, lip, 0, bad, verts, bad_blocks, **kw)
    # (the bracket searches of an eval-mode trace read the raised cells too: only what the certificate adds counts here)
    # rounds 0 and 1: no bracket search has started - the probes sent there are init_ray's, the audit there is theirs
    sent = int(probed[3][:2, _lib.CNT_PROBES].sum())
    assert probed[4][2] >= 64 and sent > 0 and int(plain[3][:2, _lib.CNT_PROBES].sum()) == 0, (probed[4], sent)
    assert grid._audit(probed[3][:2].clone()) > 0.0 and grid._audit(plain[3][:2].clone()) == 0.0
    # the model: the grid it built is replaced by the raised one behind its back
    m = _model(monkeypatch, False)
    rt = m.ray_tracer
    rt.collect_counters = False
    rt.minsdf_steps_override = steps
    n = o.shape[0]
    run = lambda: rt(sdf=m.implicit_network, cam_loc=o.to(DEV), object_mask=om.to(DEV), ray_directions=d.to(DEV).reshape(n, 1, 3))
    with torch.no_grad():
        want = run()
    monkeypatch.setenv('NEFII_BOUND_GRID_CERTIFY', '1')
    net = m.implicit_network
    net._grid[4].copy_(_raised(net._grid[4], 0.1))
    net._grid_blocks = None
    import warnings
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        got = run()
    assert rt.retraced_calls == 1 and any(kind == 'lipschitz_disabled' for kind, _, _ in net.coarse_audit_events)
    for k in range(3):
        assert torch.equal(got[k], want[k]), k
