"""tests/grid64.py without a GPU: the restatement's build (tests/test_bound_vertices_cpu.py), from fp64 vertex values rounded to
fp32, passes the judge on both trained scenes at G = 24; builds that understate the slope or carry shifted vertex values are
caught; and the point set holds the strata it promises.  tests/test_gpu_grid_fp64.py holds the kernels' builds to the same judge."""
import functools

import pytest
import torch

import grid64
import test_bound_vertices_cpu as model

G, TAU, RADIUS = 24, 1e-4, 1.0
L_FLOOR, SAFETY = 1.0, 1.5          # ops.BOUND_GRID_L_FLOOR, ops.BOUND_GRID_SAFETY
TRAINED = ('conf512-bowl-trained', 'conf512-frame-trained')


@functools.lru_cache(maxsize=None)
def _vertex_values(net):
    sdf64 = grid64.sdf64_of(net)
    probe = grid64.Grid(sdf64, G, RADIUS, TAU, torch.zeros(G, G, G).half(), torch.zeros(G, G, G).half())
    x = probe.vertex_points(torch.arange((G + 1) ** 3))
    return sdf64, sdf64(x).float().reshape(G + 1, G + 1, G + 1)


def _grid(net, shift=0.0, **kw):
    sdf64, g = _vertex_values(net)
    lo, hi, g16, l16 = model.build(g + shift, RADIUS, TAU, kw.pop('l_floor', L_FLOOR), kw.pop('safety', SAFETY))
    return grid64.Grid(sdf64, G, RADIUS, TAU, lo, hi, g16, l16)


@functools.lru_cache(maxsize=None)
def _points(net):
    grid = _grid(net)
    return grid64.points(G, RADIUS, seed=3, budget=40000, cell_l=grid.cell_l, vert_g=grid.vert_g)


@pytest.mark.parametrize('net', TRAINED)
def test_restated_build_passes_the_judge(net):
    fig = grid64.judge('%s restated G %d' % (net, G), _grid(net), _points(net).x, grad_sample=4000)
    assert fig['vertices'] == (G + 1) ** 3 and fig['bounded'] > 9 * G ** 3
    # exact vertex values: all that rule 1 sees is the rounding to fp32 and to fp16, far inside the allowance
    assert fig['over_in'] < -0.9 * TAU and fig['over_out'] < -0.9 * TAU


@pytest.mark.parametrize('net', TRAINED)
def test_the_judge_has_teeth(net):
    x = _points(net).x
    short = grid64.judge('%s safety 0.25, floor 0.05' % net, _grid(net, safety=0.25, l_floor=0.05), x, check=False, rounds=0, grad_sample=500)
    assert short['violations'][3] + short['violations'][4] > 0, short['violations']
    with pytest.raises(AssertionError):
        grid64.hold('understated slopes', short)
    shifted = grid64.judge('%s vertex values + 3 tau' % net, _grid(net, shift=3.0 * TAU), x, check=False, rounds=0, grad_sample=500)
    assert shifted['violations'][1] > 0, shifted['violations']
    with pytest.raises(AssertionError):
        grid64.hold('shifted vertex values', shifted)


def _check_strata(p, g, radius):
    cells, st = p.cells, p.strata
    corner = {tuple(c) for c in cells[st['corner_cells']].tolist()}
    assert corner == {(a, b, c) for a in (0, g - 1) for b in (0, g - 1) for c in (0, g - 1)}
    outer = cells[st['outer']]
    assert outer.shape[0] > 0 and ((outer == 0) | (outer == g - 1)).any(-1).all()
    for ax in range(3):
        for side in (0, g - 1):
            assert (outer[:, ax] == side).any(), (ax, side)
    assert ((cells >= 0) & (cells < g)).all()
    # per chosen cell: its centre and 8 points a hair inside its corners, in the order of `cells`
    n = cells.shape[0]
    assert int((p.kind == 0).sum()) == n and int((p.kind == 1).sum()) == 8 * n
    h = 2.0 * radius / g
    pts = p.x[:9 * n].double().reshape(n, 9, 3)
    base = -radius + cells.double() * h
    assert (pts[:, 0] - (base + 0.5 * h)).abs().max() < 1e-6 * radius
    rel = (pts[:, 1:] - base[:, None]) / h
    inside = ((rel > 0) & (rel < 1)).all()
    near = torch.minimum(rel, 1 - rel)
    assert inside and (near - 0.001).abs().max() < 1e-3, (bool(inside), float(near.min()), float(near.max()))
    # the faces: on them, one ulp inside and one ulp past
    face = p.x[p.kind == 2]
    r32 = torch.tensor(radius, dtype=torch.float32)
    below = torch.nextafter(r32, torch.tensor(0.0))
    for v in (r32, -r32, below, torch.nextafter(r32, torch.tensor(9.0)), torch.nextafter(-r32, torch.tensor(-9.0))):
        for ax in range(3):
            assert (face[:, ax] == v).any(), (float(v), ax)
    assert (face == below).all(-1).any(), 'the cube\'s far corner, one ulp inside'
    uni = p.x[p.kind == 3]
    assert uni.shape[0] > 0 and (uni.abs() <= radius).all()
    assert p.x.dtype == torch.float32 and p.x.shape[0] == p.kind.shape[0]


def test_point_set_holds_its_strata():
    _check_strata(_points(TRAINED[0]), G, RADIUS)
    p = _points(TRAINED[0])
    assert p.cells.shape[0] >= G ** 3 and 'steepest' in p.strata and 'near_surface' in p.strata
    again = grid64.points(G, RADIUS, seed=3, budget=40000, cell_l=_grid(TRAINED[0]).cell_l, vert_g=_grid(TRAINED[0]).vert_g)
    assert torch.equal(again.x, p.x)


@pytest.mark.parametrize('g,radius', [(80, 0.7), (256, 1.5)])
def test_sampled_point_set_stays_within_its_budget(g, radius):
    """above ALL_CELLS_G the cells are a sample: the strata are there all the same, the steepest and the nearest-to-the-surface
    cells are the ones asked for"""
    gen = torch.Generator().manual_seed(g)
    cell_l = (1.0 + torch.rand(g, g, g, generator=gen)).half()
    vert_g = (0.1 + 0.4 * torch.rand(g + 1, g + 1, g + 1, generator=gen)).half()
    cell_l[5, 6, 7], cell_l[g - 1, 0, 3] = 9.0, 8.0
    vert_g[11, 12, 13] = 0.0
    budget = 60000
    p = grid64.points(g, radius, seed=1, budget=budget, cell_l=cell_l, vert_g=vert_g, k=16)
    assert 0.8 * budget <= p.x.shape[0] <= budget
    _check_strata(p, g, float(torch.tensor(radius, dtype=torch.float32)))
    steep = p.cells[p.strata['steepest']].tolist()
    assert [5, 6, 7] in steep and [g - 1, 0, 3] in steep and len(steep) == 16
    near = p.cells[p.strata['near_surface']].tolist()
    assert all([10 + a, 11 + b, 12 + c] in near for a in (0, 1) for b in (0, 1) for c in (0, 1)), 'the 8 cells around the zero vertex'


def test_search_walks_downhill():
    """a margin with one narrow pit the sample misses: three rounds from the 256 least margins reach its bottom"""
    pit = torch.tensor([0.3137, -0.2711, 0.5523])
    margin = lambda p: (p.double() - pit.double()).norm(dim=1)
    x = (torch.rand(20000, 3, generator=torch.Generator().manual_seed(2)) * 2 - 1).float()
    h = 2.0 / 24
    xs, ms = grid64.search(margin, x, h)
    assert ms.min() < 0.5 * margin(x).min() and xs.shape[0] == 256 * 256 and (xs.abs() <= 1).all()
    # clamped inside the cube: a pit outside it is approached no further than the face
    out = lambda p: (p.double() - torch.tensor([1.2, 0.0, 0.0], dtype=torch.float64)).norm(dim=1)
    xs, ms = grid64.search(out, x, h)
    assert xs[:, 0].max() < 1.0 and (xs >= -1).all()
