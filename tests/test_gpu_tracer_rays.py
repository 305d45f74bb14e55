"""The tracer per ray against fp64, off the shipped rays and parameters (yardstick, ray families, judge: tests/trace64.py).

Every case prints the decidable rays per class, the hit-mask flips on decidable rays (must be 0), the worst surface-depth
error and the worst certificate excess before it asserts.

Measured on an MI355X (95 tests, 65 s; the fp64 references of the 512- and 256-wide nets run on the GPU in torch): 0 hit-mask
flips on decidable rays in every case and arithmetic; worst surface-depth error 5.02e-5 of the 5.5e-5 allowed (sdf_threshold +
EPS_SDF: trace64's docstring says why not sdf_threshold; the median stays at 1e-6); certificate excess never above the fp32
oracle's own by more than 1e-6, distance from a candidate at most 0.17 of its fp32 rounding bound; evaluation counts within 1 % of
the oracle's with every n_steps; every schedule bit-identical on `inside`, `graze` and `away` with 16 / 37 / 100 / 128 samples; no
refusal wrote a byte.  No case found a wrong decision in the tracer.  Two forms of the bounds as first written did not hold
against a CORRECT tracer and were restated with their reasons (trace64's docstring: the depth bound, the candidates' rounding);
prepare_job admitted negative iteration counts, now refused."""
import ctypes

import pytest
import torch

import trace64
from nefii_amd import _lib, ops
from trace64 import Case
from trace_cmp import build_sdf, compare_trace, run_gpu_trace

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ARITHMETICS = ('f32', 'f16x3', 'f16x3w')


def _mc(case):
    mc = dict(trace64.make_net(case.net)[0])
    mc['ray_tracer'] = case.params()
    return mc


_PACKED = {}


def _packed(net, split):
    if (net, split) not in _PACKED:
        mc, sd = trace64.make_net(net)[:2]
        _PACKED[(net, split)] = build_sdf(mc, sd, f16x3=split)
    return _PACKED[(net, split)]


_BOUNDS = {}


def _bounds(net):
    """(coarse_tau, minsdf_lipschitz) as the renderer calibrates them for this net"""
    if net not in _BOUNDS:
        pm32 = _packed(net, False)
        _BOUNDS[net] = (ops.calibrate_coarse_tau(_packed(net, True)),
                        ops.calibrate_lipschitz(lambda x: ops.sdf_value_grad(pm32, x)[2], DEV))
    return _BOUNDS[net]


def _trace(case, refs, precision, **kw):
    return run_gpu_trace(_mc(case), trace64.make_net(case.net)[1], refs.o, refs.d, refs.om, case.training, refs.steps, precision,
                         pm=_packed(case.net, precision.startswith('f16x3')), **kw)


def _hold(case, refs, precisions):
    """the kernel in each arithmetic against the judge, compare_trace's median / 95 % bounds on the decidable rays, and the
    oracle's evaluation counts"""
    sdf32 = trace64.make_net(case.net)[2]
    n_steps = refs.p['n_steps']
    for precision in precisions:
        got = _trace(case, refs, precision)
        trace64.judge(refs, got, '%s %s' % (case.id, precision))
        dec = refs.decidable
        if dec.any():
            sub = tuple(t.cpu()[dec] for t in got[:3]) + (None,)
            compare_trace(sdf32, refs.o[dec], refs.d[dec], sub, refs.r32['hit'][dec], refs.r32['dists'][dec], (case.id, precision),
                          refs.argmin[dec], worst=False)
        gpu_evals = ops.algorithmic_evals(got[3].cpu().long(), n_steps).sum().item()
        cpu_evals = trace64.oracle_evals(refs.r32['counters'])
        print('[trace64 %s %s] evaluations: kernel %d, oracle %d' % (case.id, precision, gpu_evals, cpu_evals))
        assert abs(gpu_evals - cpu_evals) <= 0.01 * cpu_evals, (case.id, precision, gpu_evals, cpu_evals)


# ---- the matrix ----------------------------------------------------------------------------------------------------------
# width 64, bumpy 0.03: every parameter set on `shell` and `inside`, every family on default, in all three arithmetics
SMALL = trace64.matrix()
# ... the other nets sparingly (their fp64 references run on the GPU, in torch)
OTHER = [
    (Case('physg64-smooth', 'shell', 'default', True, 1500, ('traced_hit', 'bisected_hit', 'argmin', 'moved_tmin', 'no_sphere')), ARITHMETICS),
    (Case('physg64-smooth', 'inside', 'default', True, 1500, ('traced_hit', 'argmin')), ARITHMETICS),
    (Case('physg64-smooth', 'shell', 'default', False, 1500, ('traced_hit', 'bisected_hit', 'no_sphere')), ARITHMETICS),
    (Case('physg64-smooth', 'inside', 'it0', False, 1500, ('bisected_hit', 'sampler_miss')), ARITHMETICS),
    (Case('physg512-bumpy', 'shell', 'default', True, 900, ('traced_hit', 'argmin', 'no_sphere')), ARITHMETICS),
    (Case('physg512-bumpy', 'inside', 'default', True, 900, ('traced_hit', 'argmin')), ('f16x3w',)),
    (Case('physg512-bumpy', 'graze', 'default', True, 900, ('argmin', 'no_sphere')), ('f16x3w',)),
    (Case('physg512-bumpy', 'away', 'default', True, 900, ('collapsed',)), ('f16x3w',)),
    (Case('physg512-bumpy', 'shell', 'n128_it25_k5', True, 900, ('traced_hit', 'argmin', 'no_sphere')), ('f16x3w',)),
    (Case('physg512-bumpy', 'shell', 'n37_it3', False, 900, ('bisected_hit', 'no_sphere')), ('f16x3', 'f16x3w')),
    (Case('physg512-bumpy', 'inside', 'it0', False, 900, ('bisected_hit', 'sampler_miss')), ('f16x3w',)),
    (Case('physg512-bumpy', 'inside', 'root0', True, 900, ('traced_hit', 'argmin')), ('f16x3w',)),
    (Case('neus256-bumpy', 'shell', 'default', True, 1000, ('traced_hit', 'argmin', 'no_sphere')), ('f16x3w',)),
]


@pytest.mark.parametrize('case', SMALL, ids=[c.id for c in SMALL])
def test_tracer_rays_and_parameters_vs_fp64(case):
    """Consensus verdict, argmin certificate, constants and evaluation counts (trace64's docstring) - hit mask EQUAL on the
    decidable rays, surface depths within one sdf_threshold of fp64."""
    _hold(case, trace64.References(case), ARITHMETICS)


@pytest.mark.parametrize('case,precisions', OTHER, ids=[c.id for c, _ in OTHER])
def test_tracer_rays_vs_fp64_on_the_other_nets(case, precisions):
    _hold(case, trace64.References(case, device=DEV), precisions)


# ---- "changes no decision", off the shipped rays ----------------------------------------------------------------------------
def _same(got, base, what):
    for k, name in enumerate(('points', 'hit mask', 'depths')):
        assert torch.equal(got[k], base[k]), what + (name, (got[2] - base[2]).abs().max().item())


@pytest.mark.parametrize('n_steps', [16, 37, 100, 128])
@pytest.mark.parametrize('family', ['inside', 'graze', 'away'])
@pytest.mark.parametrize('net', ['physg512-bumpy', 'neus256-bumpy'])
def test_tracer_schedules_change_no_decision_off_the_shipped_rays(net, family, n_steps, monkeypatch):
    """The bit-identity claims of test_gpu_kernels.py - the coarse pass with the measured tau, a cap of one refined sample and a
    loose tau, NEFII_SAMPLER_WINDOW 3 and 0, the staged min-SDF and bracket searches, minsdf_group, the leading-sample chunk,
    bisection levels 1, 2 and 5 - on rays that start inside the sphere, graze it or leave it, with 16, 37, 100 and 128 samples
    (quarter rows that are no multiple of 4, the 7-bit sample id at its end): points, hit mask and depths BIT-IDENTICAL to the
    plain split-precision trace."""
    case = Case(net, family, dict(n_steps=n_steps), True, 3000, ())
    mc, sd = _mc(case), trace64.make_net(net)[1]
    pm = _packed(net, True)
    assert ops.coarse_supported(pm)
    tau, lip = _bounds(net)
    o, d, om, steps = case.rays()
    rows = torch.rand(6 * n_steps, generator=torch.Generator().manual_seed(5))
    for training in (False, True):
        run = lambda st=steps, **kw: run_gpu_trace(mc, sd, o, d, om, training, st, 'f16x3w', pm=pm, **kw)
        base = run()
        cb = base[3].cpu().long()
        assert cb[:, _lib.CNT_REFINED].sum() == 0 and cb[:, _lib.CNT_COARSE_WINDOWS].sum() == 0 and cb[:, _lib.CNT_COARSE_SAMPLES].sum() == 0
        alg = ops.algorithmic_evals(cb, n_steps).sum()
        ran_coarse = 0
        for window in ('3', '0'):
            monkeypatch.setenv('NEFII_SAMPLER_WINDOW', window)
            for tag, kw in (('measured', dict(coarse_tau=tau)), ('cap1', dict(coarse_tau=tau, coarse_cap=1)), ('loose', dict(coarse_tau=0.5)),
                            ('staged', dict(coarse_tau=tau, minsdf_lipschitz=lip))):
                got = run(**kw)
                _same(got, base, (net, family, n_steps, training, window, tag))
                c = got[3].cpu().long()
                assert ops.algorithmic_evals(c, n_steps).sum() == alg
                assert c[:, _lib.CNT_LIP_AUDIT].max() == 0
                ran_coarse += int(c[:, _lib.CNT_COARSE_WINDOWS].sum() + c[:, _lib.CNT_COARSE_SAMPLES].sum())
        monkeypatch.delenv('NEFII_SAMPLER_WINDOW')
        if cb[:, _lib.CNT_SEARCHES].sum() > 0:
            assert ran_coarse > 0, 'the coarse pass never ran'
        if training:
            for kw in (dict(), dict(coarse_tau=tau), dict(coarse_tau=tau, minsdf_lipschitz=lip)):
                grouped = run(st=rows, minsdf_group=500, **kw)
                if not kw:
                    gbase = grouped
                else:
                    _same(grouped, gbase, (net, family, n_steps, 'minsdf_group', tuple(kw)))
        for chunk in ('0', '2', '6', '16', '31'):
            monkeypatch.setenv('NEFII_SAMPLER_CHUNK', chunk)
            _same(run(coarse_tau=tau), base, (net, family, n_steps, training, 'chunk', chunk))
        monkeypatch.delenv('NEFII_SAMPLER_CHUNK')
        lin = torch.linspace(0, 1, steps=n_steps).to(DEV)
        for levels in (1, 2, 5):
            if n_steps < (1 << levels):
                continue
            tp = ops.make_tracer_params(mc['ray_tracer'], training, 'f16x3w', levels)
            got = ops.trace_rays(pm, tp, o.to(DEV), d.to(DEV), om.to(DEV), lin, steps.to(DEV))
            _same(got, base, (net, family, n_steps, training, 'levels', levels))


@pytest.mark.parametrize('net', ['physg512-bumpy', 'neus256-bumpy'])
def test_tracer_coarse_pass_stays_off_above_128_samples(net):
    """n_steps = 129 does not fit the 7-bit sample id: the coarse pass and the staged searches must not run - their counters stay
    zero and the outputs are those of the plain trace."""
    case = Case(net, 'shell', dict(n_steps=129), True, 2000, ())
    mc, sd = _mc(case), trace64.make_net(net)[1]
    pm = _packed(net, True)
    o, d, om, steps = case.rays()
    for training in (False, True):
        base = run_gpu_trace(mc, sd, o, d, om, training, steps, 'f16x3w', pm=pm)
        got = run_gpu_trace(mc, sd, o, d, om, training, steps, 'f16x3w', pm=pm, coarse_tau=0.01, minsdf_lipschitz=2.0, trace_tier=1)
        _same(got, base, (net, 129, training))
        c = got[3].cpu().long()
        for col in (_lib.CNT_REFINED, _lib.CNT_COARSE_WINDOWS, _lib.CNT_COARSE_SAMPLES, _lib.CNT_COARSE_SINGLES, _lib.CNT_REPEATS):
            assert c[:, col].sum() == 0, col
        assert torch.equal(c[:, _lib.CNT_SEARCHES], c[:, _lib.CNT_DENSE_ROWS]) and c[:, _lib.CNT_SEARCHES].sum() > 0


# ---- hand-made rays --------------------------------------------------------------------------------------------------------
HAND = [   # origin, direction, what
    ((0., 0., 0.), (0., 0., 1.), 'origin at the centre'),
    ((0., 0., -1.), (0., 0., 1.), 'origin on the sphere, pointing in'),
    ((0., 0., 1.), (0., 0., 1.), 'origin on the sphere, pointing out'),
    ((0., 1., -2.), (0., 0., 1.), 'under == 0 exactly: a miss, the test is under > 0'),
    ((2.5, 0., 0.), (-1., 0., 0.), 'axis-aligned, through the middle'),
    ((0., -3., 0.), (0., 1., 0.), 'axis-aligned, through the middle'),
]


@pytest.mark.parametrize('mask', ['true', 'false'])
@pytest.mark.parametrize('net', ['physg64-smooth', 'physg64-bumpy', 'physg512-bumpy'])
def test_tracer_hand_made_rays(net, mask):
    """Six rays whose sphere intersection is exact in fp32, with object_mask all true and all false: against the fp64 trace
    through the judge, and exactly where the value is a constant."""
    o = torch.tensor([h[0] for h in HAND])
    d = torch.tensor([h[1] for h in HAND])
    om = torch.full((len(HAND),), mask == 'true')
    steps = torch.rand(100, generator=torch.Generator().manual_seed(3))
    for training in (False, True):
        case = Case(net, 'hand', 'default', training, len(HAND), (), given=(o, d, om, steps))
        refs = trace64.References(case, device=DEV)
        assert refs.r64['sphere_hit'].tolist() == [True, True, True, False, True, True]
        assert refs.cls['collapsed'].tolist() == [False, False, True, False, False, False]
        for precision in ARITHMETICS:
            got = _trace(case, refs, precision)
            trace64.judge(refs, got, '%s %s mask %s' % (case.id, precision, mask))
            pts, hit, dist = (t.cpu() for t in got[:3])
            r = refs.r64
            print('[hand %s %s train=%d mask %s] hit %s dist %s (fp64 %s)' % (net, precision, training, mask, hit.tolist(), dist.tolist(),
                                                                            [round(v, 7) for v in r['dists'].tolist()]))
            # the centre lies inside the body: the start front has arrived at its clamp, 0.01, and never moves (a masked-out
            # hit in training mode goes on to the min-SDF search behind it)
            assert r['hit'][0] and hit[0]
            if mask == 'true' or not training:
                assert r['dists'][0].item() == 0.01 and dist[0].item() == torch.tensor(0.01).item()
            # under == 0: a miss
            assert not hit[3]
            if training:
                assert dist[3].item() == 2.0 and torch.equal(pts[3], torch.tensor([0., 1., 0.]))
            else:
                assert dist[3].item() == 0.0 and torch.equal(pts[3], o[3])
            # pointing out of the sphere from its surface: both depths clamp to 0.01
            assert not hit[2]
            if training:
                assert dist[2].item() == torch.tensor(0.01).item()
            # the rays through the middle end on the surface, on their axis
            # (their depths: the judge above - every one of them must be decidable)
            for i in (1, 4, 5):
                assert refs.decidable[i] and r['hit'][i] and hit[i]
                off_axis = pts[i][d[i] == 0]
                assert (off_axis == 0).all()


# ---- batches with nothing to evaluate ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('training', [False, True])
@pytest.mark.parametrize('n', [1, 255, 256, 257, 1025])
def test_tracer_batches_in_which_no_ray_asks_for_an_evaluation(n, training):
    """All rays miss the sphere: no round has a query, every evaluator launch finds empty lists; eval: dist 0, point = origin;
    training: dist = -d.o."""
    for net, precisions in (('physg64-bumpy', ARITHMETICS), ('physg512-bumpy', ('f16x3w',))):
        case = Case(net, 'miss', 'default', training, n, ())
        refs = trace64.References(case, device=DEV)
        assert not refs.r64['sphere_hit'].any()
        for precision in precisions:
            got = _trace(case, refs, precision)
            trace64.judge(refs, got, '%s %s n=%d' % (case.id, precision, n))
            c = got[3].cpu().long()
            assert ops.algorithmic_evals(c, 100).sum() == 0 and c[:, _lib.CNT_WORK].sum() == 0
        got = _trace(case, refs, 'f16x3w', coarse_tau=_bounds(net)[0], minsdf_lipschitz=2.0, trace_tier=1)
        trace64.judge(refs, got, '%s coarse n=%d' % (case.id, n))
        assert got[3].cpu().long()[:, _lib.CNT_WORK].sum() == 0


@pytest.mark.parametrize('training', [False, True])
def test_tracer_mixed_batch_whose_last_block_is_all_misses(training):
    """600 rays: two advance blocks of `shell` and `inside` rays, then 88 rays that all miss the sphere."""
    for net, precisions in (('physg64-bumpy', ARITHMETICS), ('physg512-bumpy', ('f16x3w',))):
        parts = [trace64.rays('shell', 256, 41), trace64.rays('inside', 256, 42), trace64.rays('miss', 88, 43)]
        given = tuple(torch.cat([p[k] for p in parts]) for k in range(3)) + (parts[0][3],)
        case = Case(net, 'mixed', 'default', training, 600, ('traced_hit', 'no_sphere'), given=given)
        refs = trace64.References(case, device=DEV)
        assert not refs.r64['sphere_hit'][512:].any() and refs.r64['sphere_hit'][:512].sum() > 400
        _hold(case, refs, precisions)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
E_ARG, E_SHAPE = -1, -2          # NEFII_E_ARG, NEFII_E_SHAPE (include/nefii_amd.h; _lib.check names them)
REFUSALS = [     # what, fields set on valid training-mode parameters, expected code (read off prepare_job)
    ('n_steps < 2^bisect_levels', dict(n_steps=7), E_SHAPE),
    ('n_steps < 2^bisect_levels, 5 levels', dict(n_steps=31, bisect_levels=5), E_SHAPE),
    ('sphere_tracing_iters 251', dict(sphere_tracing_iters=251), E_SHAPE),
    ('line_step_iters 16', dict(line_step_iters=16), E_SHAPE),
    ('n_rootfind_steps 251', dict(n_rootfind_steps=251), E_SHAPE),
    ('sphere_tracing_iters -1', dict(sphere_tracing_iters=-1), E_SHAPE),
    ('line_step_iters -1', dict(line_step_iters=-1), E_SHAPE),
    ('n_rootfind_steps -1', dict(n_rootfind_steps=-1), E_SHAPE),
    ('bisect_levels 6', dict(bisect_levels=6), E_ARG),
    ('bisect_levels -1', dict(bisect_levels=-1), E_ARG),
    ('coarse_tau 1.5', dict(coarse_tau=1.5), E_ARG),
    ('coarse_tau negative', dict(coarse_tau=-1e-3), E_ARG),
    ('minsdf_lipschitz negative', dict(coarse_tau=1e-3, minsdf_lipschitz=-1.0), E_ARG),
    ('trace_tier 2', dict(coarse_tau=1e-3, trace_tier=2), E_ARG),
    ('unread_misses 2', dict(unread_misses=2), E_ARG),
    ('split_fp8 2', dict(split_fp8=2), E_ARG),
    ('precision 3', dict(precision=3), E_ARG),
    ('precision -1', dict(precision=-1), E_ARG),
    ('training without minsdf_steps', 'no steps', E_ARG),
    ('a short workspace', 'short', E_SHAPE),
    ('split precision on a net packed without it', 'unsplit', E_ARG),
]


@pytest.mark.parametrize('net', ['physg64-bumpy', 'physg512-bumpy'])
def test_tracer_refuses_by_return_code_and_launches_nothing(net):
    """Every refusal of prepare_job by its return code - and nothing enqueued: outputs, counters and the workspace (which an
    accepted call clears first) keep the pattern they were filled with.  The same buffers then run an accepted call."""
    from nefii_amd.ops import _ptr, _stream
    lib = _lib.lib()
    case = Case(net, 'shell', 'default', True, 300, ())
    o, d, om, steps = (t.to(DEV) for t in case.rays())
    om = om.to(torch.uint8)
    n = o.shape[0]
    pm, pm32 = _packed(net, True), _packed(net, False)
    lin = torch.linspace(0, 1, steps=100).to(DEV)
    for what, change, code in REFUSALS:
        tp = ops.make_tracer_params(case.params(), True, 'f16x3w')
        if isinstance(change, dict):
            for k, v in change.items():
                setattr(tp, k, v)
        good = ops.make_tracer_params(case.params(), True, 'f16x3w')
        nbytes = max(lib.nefii_trace_workspace_bytes(n, ctypes.byref(good)), lib.nefii_trace_workspace_bytes(n, ctypes.byref(tp)))
        rounds = max(lib.nefii_trace_max_rounds(ctypes.byref(good)), 1)
        ws = torch.full((nbytes,), 0x5A, device=DEV, dtype=torch.uint8)
        pts = torch.full((n, 3), -7.0, device=DEV)
        hit = torch.full((n,), 9, device=DEV, dtype=torch.uint8)
        dist = torch.full((n,), -7.0, device=DEV)
        cnt = torch.full((rounds, _lib.TRACE_COUNTERS), -3, device=DEV, dtype=torch.int32)
        rc = lib.nefii_trace_rays(ctypes.byref((pm32 if change == 'unsplit' else pm).struct), ctypes.byref(tp), _ptr(o), _ptr(d), _ptr(om), n,
                                  _ptr(lin), None if change == 'no steps' else _ptr(steps), _ptr(pts), _ptr(hit), _ptr(dist), _ptr(ws),
                                  lib.nefii_trace_workspace_bytes(n, ctypes.byref(tp)) - 1 if change == 'short' else nbytes,
                                  _ptr(cnt), _stream())
        torch.cuda.synchronize()
        assert rc == code, (what, rc, code)
        assert (ws == 0x5A).all() and (pts == -7.0).all() and (hit == 9).all() and (dist == -7.0).all() and (cnt == -3).all(), \
            (what, 'a refused call wrote something')
    # the same call, accepted
    tp = ops.make_tracer_params(case.params(), True, 'f16x3w')
    rc = lib.nefii_trace_rays(ctypes.byref(pm.struct), ctypes.byref(tp), _ptr(o), _ptr(d), _ptr(om), n, _ptr(lin), _ptr(steps), _ptr(pts),
                              _ptr(hit), _ptr(dist), _ptr(ws), nbytes, _ptr(cnt), _stream())
    torch.cuda.synchronize()
    assert rc == 0 and (hit <= 1).all() and hit.sum() > 0 and torch.isfinite(dist).all()
    # ops.trace_rays turns a refusal into an error, never into another path
    bad = ops.make_tracer_params(dict(case.params(), line_step_iters=16), True, 'f16x3w')
    with pytest.raises(RuntimeError, match='status -2'):
        ops.trace_rays(pm, bad, o, d, om, lin, steps)
