"""The SDF interval grid and its readers against fp64, on every net that ships (yardsticks: tests/grid64.py for the bounds,
tests/trace64.py for the traces; profiles/grid_fp64/README.md has the measured margins).

Builds.  ops.build_bound_grid(vertices=True) and ops.build_bound_grid_blocks with tau = ops.calibrate_coarse_tau(pm, radius), as
the model passes it, on every net of trace64.NETS that has a single-pass evaluator; G = 37 (38 vertex planes = 4 slabs of 8 and
6; 9 blocks of 4 and 1), 64 and the shipped 256 (sampled) at radius 1, and G = 64 at radius 0.7 and 1.5 on physg512-bumpy.
grid64.judge holds them to its rules 1 to 5 with zero tolerance; every sampled point's block bound lies at or below its cell's.
Builds with understated slopes and with tau = 0 are caught (built and looked up, never traced).

Readers.  physg512-bumpy and the two trained scenes, ray families `shell` and `inside`, 1500 rays, each trace with
minsdf_lipschitz from ops.calibrate_lipschitz, held by trace64.judge to the four reference traces of its case:
  (a) eval mode with bound_grid and bound_vertices;  (b) training mode with bound_grid_training and the crossing certificate;
  (c) eval mode with unread misses and the free-stretch certificate, judged on the hit mask and the hits' depths;
at G = 64, and at the shipped G = 256 on the frame.  No vacuous pass: (a) reads the grid and runs fewer quarter rows than the
trace without it, (b) and (c) certify rays, the in-kernel audit stays silent.

The cases.  MAX_UNDECIDABLE and MIN_CLASS are conditions on the four REFERENCES.  Ray seed 7 (trace64.Case's default) meets both
on every case below: 0.5 - 2.1 % undecidable.  The classes named per case are the ones with at least MIN_CLASS decidable rays
there (CLASSES below); the thin bars of the frame give `inside` 18 - 20 sampler misses among 1500 rays with every seed tried
(7, 8, 9, 10: 18, 20, 19, 20; the bowl's `shell` 26, 27, 16, 23), so that class is named where the geometry gives it: the frame's
and the bumpy body's `shell`.  moved_tmin has 21 decidable rays on the frame's `inside` under seed 7 (22, 38, 31 under 8, 9, 10)
and 22 / 17 on physg512-bumpy: not named there.  Seeds 8, 9 and 10 met both conditions as well (0.3 - 1.5 % undecidable) and
would have added no class on every case, so the default seed stays.

Sparse export.  test_gpu_mesh_sparse.py's protocol on the thin bars of frame_trained.

Measured on an MI355X (47 tests, 45 s; the slowest, 6.5 s, is the four reference traces of a training-mode case): no rule
broken on any net or grid - least corner margin 7.8e-4 under a tau of 1.17e-3 (bowl, G = 256), least cell margin 7.5e-3, slope
bound at least 1.50 x the steepest difference quotient, vertex values within 0.35 tau over the whole cube; 0 hit-mask flips and a
silent audit in all 24 reader cases; the frame's sparse export equal to the dense one with 46 % of its bricks active."""
import functools
import warnings

import pytest
import torch

import grid64
import trace64
from nefii_amd import _lib, ops
from trace64 import Case
from trace_cmp import build_sdf

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WIDE = ('physg512-bumpy', 'conf512-bowl-trained', 'conf512-frame-trained')
GRIDS = [(37, 1.0), (64, 1.0), (256, 1.0)]
RADII = {0.7: 'r0.7', 1.5: 'r1.5'}          # trace64.PARAM_SETS


# ---- the builds --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _packed(net, split=True):
    mc, sd = trace64.make_net(net)[:2]
    return build_sdf(mc, sd, f16x3=split)


def _supported(net):
    return ops.coarse_supported(_packed(net))


@functools.lru_cache(maxsize=None)
def _sdf64(net):
    return grid64.sdf64_of(net, chunk=131072)


@functools.lru_cache(maxsize=None)
def _tau(net, radius):
    return ops.calibrate_coarse_tau(_packed(net), radius)


@functools.lru_cache(maxsize=4)
def _built(net, G, radius):
    """(grid64.Grid, cells, (vert_g, cell_l), blocks) of the kernels' build"""
    pm = _packed(net)
    tau = _tau(net, radius)
    cells, verts = ops.build_bound_grid(pm, radius, tau, G, vertices=True)
    blocks = ops.build_bound_grid_blocks(cells)
    lo, hi = grid64.unpack(cells)
    return grid64.Grid(_sdf64(net), G, radius, tau, lo, hi, *verts), cells, verts, blocks


def _hold_build(net, G, radius):
    grid, cells, verts, blocks = _built(net, G, radius)
    what = '%s G %d r %.1f' % (net, G, radius)
    p = grid64.points(G, radius, seed=G, budget=400000, cell_l=grid.cell_l, vert_g=grid.vert_g, device=DEV)
    ids = None if G <= grid64.ALL_CELLS_G else grid64.vertex_sample(G, 200000, seed=G)
    fig = grid64.judge(what, grid, p.x, ids)
    assert fig['points'] >= (9 * G ** 3 if G <= grid64.ALL_CELLS_G else 300000), fig['points']
    # the block level: at or below the cell's lower end, for every sampled point with a cell
    first = fig['first']
    c, inside = grid64.cell_of(p.x, G, grid.radius)
    b = c // ops.BOUND_GRID_BLOCK
    assert blocks.shape[0] == -(-G // ops.BOUND_GRID_BLOCK)
    blo = blocks[b[:, 0], b[:, 1], b[:, 2]].float()
    above = inside & ~(blo <= first['lo_cell'])
    print('[grid64 %s] block level: %d look-ups, least lo_cell - block %.3e, blocks above their cell %d' % (
        what, int(inside.sum()), float((first['lo_cell'] - blo)[inside].min()), int(above.sum())))
    assert int(above.sum()) == 0
    return fig


def test_the_wide_nets_have_a_grid():
    """the list of nets below cannot shrink silently"""
    have = [net for net in trace64.NETS if _supported(net)]
    print('[grid64] nets with a single-pass evaluator: %s' % ', '.join(have))
    assert all(net in have for net in WIDE), have


@pytest.mark.parametrize('G,radius', GRIDS, ids=['G%d' % g for g, _ in GRIDS])
@pytest.mark.parametrize('net', list(trace64.NETS))
def test_build_holds_against_fp64(net, G, radius):
    if not _supported(net):
        # no single-pass evaluator, no grid: the build says so and writes nothing
        with pytest.raises(RuntimeError):
            ops.build_bound_grid(_packed(net), radius, 1e-4, G, vertices=True)
        return
    _hold_build(net, G, radius)


@pytest.mark.parametrize('radius', list(RADII))
def test_build_holds_at_other_radii(radius):
    assert trace64.PARAM_SETS[RADII[radius]]['object_bounding_sphere'] == radius
    _hold_build('physg512-bumpy', 64, radius)


def test_the_judge_catches_bad_builds_of_the_kernels():
    """understated slopes, and tau = 0, at G = 37 on the frame: built and looked up, never traced"""
    net, G, radius = 'conf512-frame-trained', 37, 1.0
    pm, tau = _packed(net), _tau(net, radius)
    good = _built(net, G, radius)[0]
    x = grid64.points(G, radius, seed=G, budget=400000, cell_l=good.cell_l, vert_g=good.vert_g, device=DEV).x
    for what, kw, t in (('safety 0.25, floor 0.05', dict(safety=0.25, l_floor=0.05), tau), ('tau 0', {}, 0.0)):
        cells, verts = ops.build_bound_grid(pm, radius, t, G, vertices=True, **kw)
        lo, hi = grid64.unpack(cells)
        fig = grid64.judge('%s G %d %s' % (net, G, what), grid64.Grid(_sdf64(net), G, radius, t, lo, hi, *verts), x, check=False,
                           rounds=0, grad_sample=1000)
        v = fig['violations']
        if t > 0.0:
            assert v[3] + v[4] > 0, v
        else:
            assert sum(v.values()) > 0, v
        with pytest.raises(AssertionError):
            grid64.hold(what, fig)


# ---- the readers -------------------------------------------------------------------------------------------------------------
N_RAYS = 1500
CLASSES = {     # (net, family) -> (eval mode, training mode): the classes with at least MIN_CLASS decidable rays under ray seed 7
    ('physg512-bumpy', 'shell'): (('traced_hit', 'bisected_hit', 'sampler_miss', 'no_sphere'),
                                  ('traced_hit', 'bisected_hit', 'sampler_miss', 'argmin', 'no_sphere')),
    ('physg512-bumpy', 'inside'): (('traced_hit', 'bisected_hit'), ('traced_hit', 'bisected_hit', 'argmin')),
    ('conf512-bowl-trained', 'shell'): (('traced_hit', 'bisected_hit', 'no_sphere'),
                                        ('traced_hit', 'bisected_hit', 'argmin', 'moved_tmin', 'no_sphere')),
    ('conf512-bowl-trained', 'inside'): (('traced_hit', 'bisected_hit'), ('traced_hit', 'bisected_hit', 'argmin', 'moved_tmin')),
    ('conf512-frame-trained', 'shell'): (('traced_hit', 'bisected_hit', 'sampler_miss', 'no_sphere'),
                                         ('traced_hit', 'bisected_hit', 'sampler_miss', 'argmin', 'moved_tmin', 'no_sphere')),
    ('conf512-frame-trained', 'inside'): (('traced_hit', 'bisected_hit'), ('traced_hit', 'bisected_hit', 'argmin')),
}
READERS = [(net, fam, 64) for net, fam in CLASSES] + [('conf512-frame-trained', fam, 256) for fam in ('shell', 'inside')]


@functools.lru_cache(maxsize=None)
def _refs(net, family, training):
    case = Case(net, family, 'default', training, N_RAYS, CLASSES[(net, family)][1 if training else 0])
    return trace64.References(case, device=DEV)


@functools.lru_cache(maxsize=None)
def _lip(net):
    pm32 = _packed(net, False)
    return ops.calibrate_lipschitz(lambda x: ops.sdf_value_grad(pm32, x)[2], DEV)


def _trace(refs, net, G=0, training=False, unread=0, parts=0, lip=None):
    """-> (points, hit, depths, counters, certify counts); G = 0: without the grid"""
    tau = _tau(net, 1.0)
    tp = ops.make_tracer_params(refs.p, training, 'f16x3w', coarse_tau=tau, minsdf_lipschitz=_lip(net) if lip is None else lip,
                                unread_misses=unread)
    lin = torch.linspace(0, 1, steps=tp.n_steps).to(DEV)
    cells, verts, blocks = _built(net, G, 1.0)[1:] if G else (None, None, None)
    counts = torch.zeros(ops.CERTIFY_COUNTS, device=DEV, dtype=torch.int32)
    out = ops.trace_rays(_packed(net), tp, refs.o.to(DEV).contiguous(), refs.d.to(DEV).contiguous(), refs.om.to(DEV), lin,
                         refs.steps.to(DEV), want_counters=True, bound_grid=cells, bound_vertices=verts,
                         bound_grid_training=bool(training and G), bound_grid_certify=blocks if parts else None,
                         certify_counts=counts, certify_parts=parts or 3)
    return out + (counts.cpu().tolist(),)


def _audit(counters):
    return counters[:, _lib.CNT_LIP_AUDIT].cpu().contiguous().view(torch.float32).max().item()


def _sum(counters, col):
    return int(counters[:, col].sum())


@pytest.mark.parametrize('net,family,G', READERS, ids=['%s-%s-G%d' % r for r in READERS])
def test_eval_trace_reading_the_grid(net, family, G):
    """(a)"""
    refs = _refs(net, family, False)
    got = _trace(refs, net, G)
    trace64.judge(refs, got, '%s G %d grid + corners' % (refs.case.id, G))
    off = _trace(refs, net, 0, lip=0.0)          # (what NEFII_BOUND_GRID=0 leaves of an eval-mode trace: unstaged)
    w0, w1 = _sum(off[3], _lib.CNT_COARSE_WINDOWS), _sum(got[3], _lib.CNT_COARSE_WINDOWS)
    print('[grid64 %s G %d (a)] %d bracket searches: quarter rows %d -> %d, %d survivors; audit %.2e' % (
        refs.case.id, G, _sum(got[3], _lib.CNT_SEARCHES), w0, w1, _sum(got[3], _lib.CNT_COARSE_SAMPLES), _audit(got[3])))
    assert _sum(got[3], _lib.CNT_COARSE_SAMPLES) > 0 and w1 < w0, (w0, w1)
    assert _audit(got[3]) == 0.0


@pytest.mark.parametrize('net,family,G', READERS, ids=['%s-%s-G%d' % r for r in READERS])
def test_training_trace_reading_the_grid_and_certifying(net, family, G):
    """(b)"""
    refs = _refs(net, family, True)
    got = _trace(refs, net, G, training=True, parts=1)
    trace64.judge(refs, got, '%s G %d grid in training mode + crossing certificate' % (refs.case.id, G))
    print('[grid64 %s G %d (b)] certified %d rays of %d misses (%d block look-ups); audit %.2e' % (
        refs.case.id, G, got[4][0], int((~got[1]).sum()), got[4][1], _audit(got[3])))
    assert got[4][0] > 0 and got[4][2] == 0, got[4]
    assert _audit(got[3]) == 0.0


@pytest.mark.parametrize('net,family,G', READERS, ids=['%s-%s-G%d' % r for r in READERS])
def test_unread_misses_ended_as_free(net, family, G):
    """(c)"""
    refs = _refs(net, family, False)
    got = _trace(refs, net, G, unread=1, parts=2)
    trace64.judge(refs, got, '%s G %d unread misses + free-stretch certificate' % (refs.case.id, G), hits_only=True)
    print('[grid64 %s G %d (c)] ended as free %d rays of %d misses (%d look-ups); audit %.2e' % (
        refs.case.id, G, got[4][2], int((~got[1]).sum()), got[4][3], _audit(got[3])))
    assert got[4][2] > 0 and got[4][0] == 0, got[4]
    assert _audit(got[3]) == 0.0


# ---- sparse export on the thin geometry --------------------------------------------------------------------------------------
def test_sparse_export_of_the_frame_equals_the_dense_export(monkeypatch):
    from nefii_amd.mesh import extract_mesh
    from test_gpu_mesh import scene_model
    from test_gpu_mesh_sparse import same_mesh
    model, _, _ = scene_model('frame_trained', 'conf')
    monkeypatch.setattr(ops, 'BOUND_GRID_SIZE', 64)
    dense = extract_mesh(model, resolution=128)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        sparse = extract_mesh(model, resolution=128, sparse=True)
    s = sparse.meta['sparse']
    print('[grid64 sparse export, frame] r 128, G 64: %s; active bricks %.1f %%, evaluated points %.1f %% of the dense grid\'s' % (
        s, 100.0 * s['active_bricks'] / s['bricks'], 100.0 * s['evaluated_points'] / s['dense_points']))
    assert 'sparse' not in dense.meta and dense.verts.shape[0] > 1000
    same_mesh(sparse, dense)
    assert s['audit_violations'] == 0 and s['fallback'] is None
    assert s['dense_points'] == 128 ** 3 and s['evaluated_points'] < s['dense_points']
