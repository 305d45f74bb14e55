"""Training-mode traces that read the SDF interval grid (include/nefii_amd.h: nefii_trace_grid.training; DESIGN section
4h) on the GPU: the bracket searches of the rays INSIDE the object mask start from the grid - cell intervals, corner bounds,
probes and audit as in eval mode - in place of their windows; rays outside the mask and the min-SDF searches keep their
evaluated first stage.  Points, hit mask and depths are bit-identical with the grid, without it and without any staging; the
audit stays silent; the in-mask searches cost no more single-pass evaluations; out-of-mask rays see nothing change.  On the
adversarial dent of tests/test_gpu_bound_vertices.py no bundle size may differ from the full search without the audit having
fired.  On the model level: RayTracing.bound_grid_training / NEFII_BOUND_GRID_TRAINING, grouped traces, and a TrainStep run whose
traces and first loss do not move by a bit and whose later losses and parameters stay within what runs with the switch left alone
differ by among themselves (they do not repeat from run to run: see the test)."""
import functools

import pytest
import torch

from nefii_amd import _lib, conf, ops, synthetic as syn
from trace_cmp import build_sdf

import test_gpu_bound_grid as grid
import test_gpu_bound_vertices as vertices
import test_gpu_minsdf_share as share

pytestmark = pytest.mark.gpu

DEV = grid.DEV
G = vertices.G


def _trace(mc, pm, o, d, om, steps, tau, lip, tier=0, cells=None, verts=None, in_training=False, group=0, training=True,
           unread_misses=0):
    tp = ops.make_tracer_params(mc['ray_tracer'], training, 'f16x3w', coarse_tau=tau, minsdf_lipschitz=lip, trace_tier=tier,
                                minsdf_group=group, unread_misses=unread_misses)
    lin = torch.linspace(0, 1, steps=tp.n_steps).to(DEV)
    return ops.trace_rays(pm, tp, o.to(DEV).contiguous(), d.to(DEV).contiguous(), om.to(DEV), lin, steps.to(DEV),
                          want_counters=True, bound_grid=cells, bound_vertices=verts, bound_grid_training=in_training)


@functools.lru_cache(maxsize=None)
def _rays():
    """4096 rays: half started on the surface (most of their bracket searches find a crossing late or never), half from outside"""
    so, sd = grid._secondary()
    m = min(so.shape[0], 2048)
    po, pd = share._random(4096 - m, 41, spread=0.35)
    perm = torch.randperm(4096, generator=torch.Generator().manual_seed(12))
    g = torch.Generator().manual_seed(13)
    return torch.cat([so[:m], po])[perm], torch.cat([sd[:m], pd])[perm], torch.rand(4096, generator=g) < 0.6, torch.rand(100, generator=g)


def _bracket_evals(c):
    """single-pass evaluations of quarter rows and single samples (n_steps 100: 25 per quarter row)"""
    return int(c[:, _lib.CNT_COARSE_WINDOWS].sum() * 25 + c[:, _lib.CNT_COARSE_SAMPLES].sum())


@pytest.mark.parametrize('tier', [0, 1])
def test_grid_for_training_changes_no_output(tier):
    mc, pm, tau, lip, cells, verts = vertices._bowl()
    o, d, om, steps = _rays()
    plain = _trace(mc, pm, o, d, om, steps, tau, 0.0, tier)
    off = _trace(mc, pm, o, d, om, steps, tau, lip, tier, cells, verts, False)
    on = _trace(mc, pm, o, d, om, steps, tau, lip, tier, cells, verts, True)
    for k, out in enumerate(('points', 'hit mask', 'depths')):
        assert torch.equal(on[k], off[k]), (out, 'against the trace that ignores the grid')
        assert torch.equal(on[k], plain[k]), (out, 'against the unstaged trace')
    assert grid._audit(on[3]) == 0.0, grid._audit(on[3])
    assert torch.equal(off[3], _trace(mc, pm, o, d, om, steps, tau, lip, tier)[3]), 'a trace not asked to reads the grid'
    # the rays inside the mask alone: their searches' evaluations; the rays outside it alone: nothing changes
    inside, outside = torch.nonzero(om).flatten(), torch.nonzero(~om).flatten()
    res = {}
    for name, idx in (('inside', inside), ('outside', outside)):
        mask = om[idx]
        a = _trace(mc, pm, o[idx], d[idx], mask, steps, tau, lip, tier, cells, verts, False)
        b = _trace(mc, pm, o[idx], d[idx], mask, steps, tau, lip, tier, cells, verts, True)
        for k in range(3):
            assert torch.equal(a[k], b[k]), (name, k)
        res[name] = (a[3].cpu().long(), b[3].cpu().long())
    c0, c1 = res['inside']
    e0, e1 = _bracket_evals(c0), _bracket_evals(c1)
    print('[grid training tier=%d] %d rays inside the mask, %d searches: single-pass evaluations of quarter rows and samples %d -> %d '
          '(quarter rows %d -> %d, samples %d -> %d, probes %d -> %d)' % (
              tier, inside.numel(), c0[:, _lib.CNT_SEARCHES].sum(), e0, e1, c0[:, _lib.CNT_COARSE_WINDOWS].sum(),
              c1[:, _lib.CNT_COARSE_WINDOWS].sum(), c0[:, _lib.CNT_COARSE_SAMPLES].sum(), c1[:, _lib.CNT_COARSE_SAMPLES].sum(),
              c0[:, _lib.CNT_PROBES].sum(), c1[:, _lib.CNT_PROBES].sum()))
    assert c1[:, _lib.CNT_SEARCHES].sum() == c0[:, _lib.CNT_SEARCHES].sum()
    assert c1[:, _lib.CNT_COARSE_SAMPLES].sum() > c0[:, _lib.CNT_COARSE_SAMPLES].sum(), 'no search read the grid: the case checks nothing'
    assert e1 <= e0, (e0, e1)
    assert torch.equal(*res['outside']), 'rays outside the mask: counters differ'


def test_grid_for_training_against_the_windows(monkeypatch):
    """the same rays with the quarter-row windows the big batches take (NEFII_SAMPLER_WINDOW=3): what the grid replaces on the
    headline workload.  Outputs as before; the evaluations are printed (G = 64 here, 256 there)"""
    mc, pm, tau, lip, cells, verts = vertices._bowl()
    o, d, om, steps = _rays()
    inside = torch.nonzero(om).flatten()
    o, d, om = o[inside], d[inside], om[inside]
    monkeypatch.setenv('NEFII_SAMPLER_WINDOW', '3')
    off = _trace(mc, pm, o, d, om, steps, tau, lip, 0, cells, verts, False)
    on = _trace(mc, pm, o, d, om, steps, tau, lip, 0, cells, verts, True)
    for k in range(3):
        assert torch.equal(on[k], off[k]), k
    assert grid._audit(on[3]) == 0.0
    c0, c1 = off[3].cpu().long(), on[3].cpu().long()
    print('[grid training, windows] %d searches: single-pass evaluations of quarter rows and samples %d -> %d' % (
        c0[:, _lib.CNT_SEARCHES].sum(), _bracket_evals(c0), _bracket_evals(c1)))


def _model(monkeypatch, on):
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    monkeypatch.setenv('NEFII_BOUND_GRID_TRAINING', '1' if on else '0')
    mc = syn.model_conf('conf')
    sd = syn.make_state_dict(mc, seed=2, scene='bowl_trained')
    m = IDRNetwork(conf.from_dict(mc))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m.freeze_geometry()
    m.train()
    assert m.ray_tracer.bound_grid_training == on
    m.ray_tracer.bound_grid_size = G
    m.ray_tracer.collect_counters = True
    return m


@pytest.mark.parametrize('miss_search', [True, False])
def test_model_switch_and_miss_search(miss_search, monkeypatch):
    """RayTracing.forward in training mode under frozen geometry: the grid is built at the first trace and read by default,
    NEFII_BOUND_GRID_TRAINING=0 leaves the training-mode traces as they were; miss_search off (the secondary rays' schedule: an
    eval-mode trace) reads the grid either way"""
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
        assert (m.implicit_network._grid is not None) == (on or not miss_search)
        res[on] = out + (rt.last_counters.cpu(),)
    for k in range(3):
        assert torch.equal(res[True][k], res[False][k]), k
    assert grid._audit(res[True][3]) == 0.0
    if miss_search:
        assert _bracket_evals(res[True][3]) < _bracket_evals(res[False][3])
    else:
        assert torch.equal(res[True][3], res[False][3])


def test_grouped_trace_equals_the_single_traces(monkeypatch):
    """two batches as one tracer call (RayTracing.steps_per_batch, TrainStep's grouped traces): each slice is that batch's own
    trace, with the grid read in both"""
    o, d, om, _ = _rays()
    S = 1536
    m = _model(monkeypatch, True)
    rt = m.ray_tracer
    cams = torch.tensor([[0.2, 0.1, 2.0], [1.6, -0.3, 1.2]])
    dirs = torch.nn.functional.normalize(torch.randn(2, S, 3, generator=torch.Generator().manual_seed(5)) * 0.3 - cams[:, None], dim=-1)
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
    assert (rt.last_counters[:, _lib.CNT_PROBES].sum() > 0), 'no search read the grid'
    torch.manual_seed(21)
    drawn = [torch.empty(100).uniform_(0.0, 1.0) for _ in range(2)]
    for b in range(2):
        rt.minsdf_steps_override = drawn[b]
        one = run(cams[b:b + 1], dirs[b:b + 1], mask[b * S:(b + 1) * S], False)
        for k in range(3):
            assert torch.equal(one[k], both[k][b * S:(b + 1) * S]), (b, k)
    rt.minsdf_steps_override = None
    assert rt.retraced_calls == 0 and not m.implicit_network.coarse_audit_events


def test_training_rays_on_the_dent():
    """test_corners_on_the_dent's pocket, bundles, tau, L and grid (G = 256) with TRAINING-mode rays inside the mask aimed through
    the pocket: every trace is bit-identical to the full search or has raised the audit (the model then traces again without the
    staging: RayTracing.forward, TrainStep._take_prefetched); a difference with a silent audit is counted, and there is none"""
    from test_gpu_kernels import _bundle_through, _dent_scene
    mc, sd, c = _dent_scene()
    pm, pm32 = build_sdf(mc, sd, f16x3=True), build_sdf(mc, sd)
    tau = ops.calibrate_coarse_tau(pm)
    lip = ops.calibrate_lipschitz(lambda x: ops.sdf_value_grad(pm32, x)[2], DEV)
    cells, verts = ops.build_bound_grid(pm, 1.0, tau, 256, l_floor=lip, vertices=True)
    cd = c.to(DEV)
    steps = torch.rand(100, generator=torch.Generator().manual_seed(2))
    table = []
    for n, reps in ((4096, 2), (256, 8), (64, 16), (16, 32), (4, 48), (1, 64)):
        silent = detected = same = differing = pocket = walked = 0
        for rep in range(reps):
            o, d = _bundle_through(c, n, 100 * n + rep)
            om = torch.ones(n, dtype=torch.bool)
            base = _trace(mc, pm, o, d, om, steps, tau, 0.0)
            got = _trace(mc, pm, o, d, om, steps, tau, lip, 0, cells, verts, True)
            viol = grid._audit(got[3])
            diff = int(((got[2] != base[2]) | (got[1] != base[1])).sum())
            pocket += int(((base[0] - cd).abs().sum(1) < 0.012).sum())
            walked += int(got[3][:, _lib.CNT_PROBES].sum() > 0)
            differing += diff
            if diff == 0:
                same += 1
            elif viol > 0:
                detected += 1
            else:
                silent += 1
        table.append((n, reps, same, detected, silent, differing, pocket, walked))
        print('[grid training dent] bundles of %4d rays x %2d: bit-identical %2d, audit fired %2d, SILENT miss %2d (rays that differ %d, '
              'rays the full search ends in the pocket %d, traces with a probe %d)' % table[-1])
    assert table[0][6] > 0.1 * 4096 * 2, table
    assert table[0][7] == 2, table
    assert all(t[4] == 0 for t in table), table


OFF = ('off', 'off again', 'off once more')
R_RECORDED = 4.0e-5       # the largest R of nine measurements of runs with the switch off (the test's docstring)


def test_train_step_does_not_move_by_a_bit(monkeypatch):
    """TrainStep on config 3 shrunk in pixels (tests/test_gpu_configs.py's size), three steps with the next batch traced ahead,
    untiered, NEFII_BOUND_GRID_TRAINING on against off.

    A run of these three steps does not repeat ITSELF bit for bit: the training kernels' backward accumulates in an order that
    changes from run to run.  Measured on MI355X with the switch off both times: the losses of the three steps 16.4841347,
    7.23567629 / 7.23567581, 13.3558979 / 13.3558989 / 13.3558969, and 31 to 33 parameter tensors that differ (the rendering
    network's first), with and without the secondary step, with torch's deterministic algorithms on or off; the library has no
    deterministic reduction path.  So the test runs the switch off THREE TIMES and on once, and asserts
      bit-identity on everything a run does repeat: every primary trace (frozen geometry: no trained parameter reaches it), the
        one the step makes itself and the two enqueued ahead; the secondary trace and the loss of the first step, which see
        the initial parameters only - between all four runs;
      every parameter after the three steps, on against the nearest off run: the root-mean-square difference over the tensor
        within 4 x R x the tensor's root-mean-square value, where R is the largest such relative difference between two
        off runs on any tensor (root mean squares, because the largest single element's difference has a heavy tail - a
        near-zero gradient whose sign flips moves its element by a whole Adam step; R over all tensors, so that a tensor that
        happens to repeat between the off runs is not held to zero; the noise has a heavy tail - over nine
        measurements with the switch off R came out between 3.7e-6 and 4.0e-5, a single run now and then lying ten times
        further from the others than they lie from each other - so R is not taken below the largest of those, 4.0e-5, and three
        off runs are made, not two; 4: the on run is one more draw of the same noise if the
        switch changes nothing);
      the later losses likewise within 4 x the largest relative difference two off runs show on any step, and not below 4
        units in the last place of fp32 (2^-23 relative) for a pair that happens to agree.
    Both bounds are printed with what they bound."""
    from nefii_amd.training.step import TrainStep
    from test_gpu_configs import SHRUNK, build_model, to_dev
    w = syn.WORKLOADS['cfg3']
    lc = syn.loss_conf(w['model'])
    batches = [syn.make_inputs(SHRUNK['cfg3'], w['image_hw'], w['focal'], w['cam_pos'], w['num_rays'], seed=s) for s in (1, 2, 3)]
    n_primary = SHRUNK['cfg3'] * w['num_rays']
    res = {}
    for run in ('on',) + OFF:
        on = run == 'on'
        monkeypatch.setenv('NEFII_BOUND_GRID_TRAINING', '1' if on else '0')
        mc, sd = syn.workload_state_dict('cfg3', seed=0)
        m = build_model(mc, sd, True)
        assert m.ray_tracer.bound_grid_training == on and not m.ray_tracer.trace_tier
        m.ray_tracer.bound_grid_size = G
        m.ray_tracer.collect_counters = True
        # what each step's tail is handed (a trace enqueued ahead is complete only once TrainStep has settled it) and what
        # every synchronous trace returns (the secondary traces)
        traces, tails = [], []
        m.ray_tracer.register_forward_hook(lambda mod, args, out: traces.append(tuple(t.detach().clone() for t in out)))
        # (each trace's own counters, read once everything has run: RayTracing.counter_sum is combined on whichever stream the
        # trace was enqueued on)
        counters = []
        m.ray_tracer.register_forward_hook(lambda mod, args, out: counters.append(mod.last_counters))
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
                    params)
    # ---- what repeats: bit for bit between all four runs
    for other in OFF:
        assert len(res['on'][1]) == 4 and len(res[other][1]) == 4, 'three primary traces and the first secondary one'
        for n, (a, b) in enumerate(zip(res['on'][1], res[other][1])):
            for k in range(len(a)):
                assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (other, n, k, a[k].shape)
        assert torch.equal(res['on'][0][0], res[other][0][0]), (other, res['on'][0][0].item(), res[other][0][0].item())
    # ---- what does not: within the noise the off runs show among themselves
    p_on, p_off = res['on'][3], [res[r][3] for r in OFF]
    pairs = [(a, b) for n, a in enumerate(p_off) for b in p_off[n + 1:]]
    rms = lambda x: float(x.pow(2).mean().sqrt())
    scale = {k: rms(p_off[0][k]) for k in p_on}
    spread = {k: max(rms(a[k] - b[k]) for a, b in pairs) for k in p_on}
    R_seen = max(spread[k] / scale[k] for k in p_on if scale[k] > 0)
    R = max(R_seen, R_RECORDED)
    moved = [k for k in p_on if spread[k] > 0]
    worst = (-1.0, '')
    for k in p_on:
        dist = min(rms(p_on[k] - q[k]) for q in p_off)
        if scale[k] > 0:
            worst = max(worst, (dist / scale[k], k))
        assert dist <= 4.0 * R * scale[k], (k, dist, spread[k], 4.0 * R * scale[k])
    l_on, l_off = [x.item() for x in res['on'][0]], [[x.item() for x in res[r][0]] for r in OFF]
    r_loss = max(max(abs(a[k] - b[k]) / abs(a[k]) for k in range(3) for n, a in enumerate(l_off) for b in l_off[n + 1:]), 2.0 ** -23)
    for k in (1, 2):
        dist = min(abs(l_on[k] - q[k]) for q in l_off)
        assert dist <= 4.0 * r_loss * abs(l_off[0][k]), (k, l_on[k], [q[k] for q in l_off])
    assert all(grid._audit(c) == 0.0 for c in res['on'][2])
    e_on, e_off = (sum(_bracket_evals(c.long()) for c in res[r][2][:2]) for r in ('on', OFF[0]))
    print('[grid training step] 3 steps, losses on %s, off %s (bound: %.2e relative); parameters: %d of %d tensors differ between the '
          'off runs, largest relative rms difference %.3e (R not below %.1e); on against the nearest off run at most %.3e (%s), bound 4 R; single-pass '
          'evaluations of quarter rows and samples, the first two primary traces: %d -> %d' % (
              ['%.9g' % x for x in l_on], [['%.9g' % x for x in q] for q in l_off], 4.0 * r_loss, len(moved), len(p_on), R_seen, R_RECORDED,
              worst[0], worst[1], e_off, e_on))
    assert e_on != e_off, 'no training-mode trace read the grid'
