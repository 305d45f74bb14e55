"""Sparse mesh export without a GPU (DESIGN.md 6f "Sparse export"): the NumPy restatement of the brick classification
(tests/mesh_sparse_ref.py) is conservative on an analytic interval grid, the point functions give the dense grids' rows, the
evaluated set covers what the active bricks read and owns every point once, arguments are refused before any work, and the
command line knows the flags."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import mesh_sparse_ref as ref  # noqa: E402


def sphere_cells(G, radius, r):
    """interval grid of the SDF |p| - r over [-radius, radius]^3: exact bounds per cell, rounded outwards to fp16"""
    e = np.linspace(-radius, radius, G + 1)
    lo1, hi1 = e[:-1], e[1:]
    near = np.where((lo1 <= 0) & (hi1 >= 0), 0.0, np.minimum(np.abs(lo1), np.abs(hi1)))
    far = np.maximum(np.abs(lo1), np.abs(hi1))
    dmin = np.sqrt(near[:, None, None] ** 2 + near[None, :, None] ** 2 + near[None, None, :] ** 2)
    dmax = np.sqrt(far[:, None, None] ** 2 + far[None, :, None] ** 2 + far[None, None, :] ** 2)
    return ref.pack_cells(dmin - r - 1e-6, dmax - r + 1e-6)


@pytest.mark.parametrize('rotated', [False, True])
@pytest.mark.parametrize('brick', [8, 4])
def test_restated_rule_is_conservative_on_a_sphere(rotated, brick):
    G, R, r = 32, 1.0, 0.4
    cells = sphere_cells(G, R, r)
    shape = (41, 37, 44)
    sp = 0.035
    rot = ref.rotation((1.0, 2.0, 3.0), 0.7) if rotated else np.eye(3)
    steps = sp * rot
    p0 = np.array([0.05, -0.03, 0.02]) - sum(steps[a] * (shape[a] - 1) / 2 for a in range(3))
    active = ref.classify_bricks(cells, R, shape, p0, steps, 0.0, brick)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing='ij'), -1).astype(np.float64)
    pts = (((p0 + idx[..., 0:1] * steps[0]) + idx[..., 1:2] * steps[1]) + idx[..., 2:3] * steps[2]).astype(np.float32)
    vol = (np.linalg.norm(pts.astype(np.float64), axis=-1) - r).astype(np.float32)
    crossing = ref.crossing_bricks(vol, 0.0, brick)
    assert crossing.sum() > 10
    assert not np.any((crossing == 1) & (active == 0)), 'a brick with a sign change was ruled out'
    assert (active == 0).sum() > 0, 'the rule rules nothing out: the check above is empty'


def test_restated_rule_outside_the_cube_and_non_finite_words():
    G, R = 8, 1.0
    lo = np.full((G, G, G), 0.25, np.float32)
    hi = np.full((G, G, G), 0.5, np.float32)
    steps = 0.02 * np.eye(3)
    inside = ref.classify_bricks(ref.pack_cells(lo, hi), R, (17, 17, 17), [-0.2] * 3, steps, 0.0, 8)
    assert inside.shape == (2, 2, 2) and not inside.any()                       # 0 < lo everywhere
    assert ref.classify_bricks(ref.pack_cells(lo, hi), R, (17, 17, 17), [-0.2] * 3, steps, 0.3, 8).all()
    out = ref.classify_bricks(ref.pack_cells(lo, hi), R, (17, 17, 17), [0.8, -0.2, -0.2], steps, 0.0, 8)
    assert out[1].all() and not out[0].any()                                    # x runs to 1.12: the second layer leaves
    edge = ref.classify_bricks(ref.pack_cells(lo, hi), R, (17, 17, 17), [0.68, -0.2, -0.2], steps, 0.0, 8)
    assert edge[1].all()                                                        # ends AT 1.0: widened, it leaves
    lo[4, 4, 4] = np.nan                                                        # the cell [0, 0.25]^3
    out = ref.classify_bricks(ref.pack_cells(lo, hi), R, (17, 17, 17), [-0.2] * 3, steps, 0.0, 8)
    assert out[1, 1, 1] == 1 and out.sum() == 1                                 # only the brick that reaches past 0 on every axis


def test_point_functions_give_the_dense_rows():
    from nefii_amd import mesh
    r, bound = 13, 1.05
    n = r ** 3
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, n, (500,), generator=g)
    ax = mesh.grid_axis(r, bound, 'cpu')
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing='ij')
    dense = torch.stack([X, Y, Z], -1).reshape(-1, 3)
    assert torch.equal(mesh.grid_points_at(idx, r, bound), dense[idx])
    assert torch.equal(mesh.grid_points_at(torch.arange(n), r, bound), dense)
    pts = torch.randn(200, 3, generator=g, dtype=torch.float64) * torch.tensor([0.5, 0.2, 0.3], dtype=torch.float64)
    grid = mesh.aligned_grid(pts, 11, 0.1)
    m = grid.numel()
    idx = torch.randint(0, m, (700,), generator=g)
    rows = grid.points(0, m)
    assert torch.equal(grid.points_at(idx), rows[idx])
    p0, steps = grid.frame()
    i = torch.tensor([0, m - 1])
    nx, ny, nz = grid.shape
    want = np.array(p0) + (nx - 1) * np.array(steps[0]) + (ny - 1) * np.array(steps[1]) + (nz - 1) * np.array(steps[2])
    got = grid.points_at(i).double().numpy()
    assert np.abs(got[0] - np.array(p0)).max() < 1e-6 and np.abs(got[1] - want).max() < 1e-5


def test_both_grids_have_one_point_expression():
    from nefii_amd import mesh
    g = torch.Generator().manual_seed(2)
    pts = torch.randn(200, 3, generator=g, dtype=torch.float64) * torch.tensor([0.5, 0.2, 0.3], dtype=torch.float64)
    for grid in (mesh.UniformGrid(13, 1.05), mesh.aligned_grid(pts, 11, 0.1)):
        n = grid.numel()
        assert n == grid.shape[0] * grid.shape[1] * grid.shape[2]
        for a, b in ((0, n), (n // 3 + 1, n - 7), (n - 1, n), (5, 5)):
            rows = grid.points(a, b)
            assert rows.dtype == torch.float32 and tuple(rows.shape) == (b - a, 3)
            assert torch.equal(rows, grid.points_at(torch.arange(a, b)))


def test_uniform_grid_is_what_extract_mesh_built_inline():
    from nefii_amd import mesh
    r, bound = 13, 1.05
    grid = mesh.UniformGrid(r, bound)
    sp = 2.0 * bound / (r - 1)
    assert grid.shape == (13, 13, 13) and grid.numel() == 13 ** 3
    assert grid.origin == (-bound, -bound, -bound) and grid.spacing == sp
    assert grid.frame() == ([-bound] * 3, [[sp, 0.0, 0.0], [0.0, sp, 0.0], [0.0, 0.0, sp]])
    assert all(type(v) is float for v in grid.frame()[0] + sum(grid.frame()[1], []))
    local = torch.randn(5, 3)
    assert grid.to_world(local) is local
    # the public wrappers and the evaluator's rows are the grid's points
    idx = torch.randint(0, r ** 3, (300,), generator=torch.Generator().manual_seed(3))
    assert torch.equal(mesh.grid_points_at(idx, r, bound), grid.points_at(idx))
    assert torch.equal(mesh.grid_axis(r, bound, 'cpu'), torch.linspace(-bound, bound, r, dtype=torch.float32))

    class Recorder(torch.nn.Module):                                            # a "network" that keeps the points it is asked for
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
            self.seen = []

        def forward(self, x):
            self.seen.append(x)
            return x[:, :1] + x[:, 2:]

    net = Recorder()
    vol = mesh.sdf_grid(net, r, bound, chunk=500, precision='f32')              # 2197 points in five chunks
    rows = grid.points_at(torch.arange(r ** 3))
    assert len(net.seen) == 5 and torch.equal(torch.cat(net.seen), rows)
    assert tuple(vol.shape) == grid.shape and torch.equal(vol.reshape(-1), rows[:, 0] + rows[:, 2])
    for res, msg in ((1, 'resolution must be >= 2'), (1300, 'fewer than 2\\^31 points')):
        with pytest.raises(ValueError, match=msg):
            mesh.sdf_grid(net, res, bound)
    assert len(net.seen) == 5                                                   # refused before anything was evaluated


@pytest.mark.parametrize('shape,brick', [((2, 2, 2), 8), ((9, 9, 9), 8), ((10, 9, 17), 8), ((37, 21, 50), 4), ((17, 18, 16), 8)])
def test_evaluated_set_covers_the_active_bricks_and_owns_each_point_once(shape, brick):
    from nefii_amd import ops
    cb, pb = ops.brick_dims(shape, brick)
    assert cb == ref.brick_counts(shape, brick)
    g = torch.Generator().manual_seed(1)
    active = (torch.rand(cb, generator=g) < 0.3).to(torch.uint8)
    ev = ops.dilate_bricks(active, shape, brick)
    assert tuple(ev.shape) == pb
    owner = [torch.arange(n) // brick for n in shape]
    assert all(int(o.max()) == p - 1 for o, p in zip(owner, pb))                # every point has an owner, no brick is empty
    need = torch.zeros(pb, dtype=torch.bool)
    for b in active.nonzero().tolist():
        rng = [range(b[a] * brick, min(b[a] * brick + brick, shape[a] - 1) + 1) for a in range(3)]
        for a0 in {int(owner[0][i]) for i in rng[0]}:
            for a1 in {int(owner[1][i]) for i in rng[1]}:
                for a2 in {int(owner[2][i]) for i in rng[2]}:
                    need[a0, a1, a2] = True
    assert bool((ev | ~need).all()), 'an active brick reads a point of a brick that is not evaluated'
    assert int(ev.sum()) <= 8 * max(1, int(active.sum()))


def test_capped_probes_span_the_grid():
    from nefii_amd import mesh
    cb, brick = (200, 200, 200), 8                                             # 8 M skipped bricks: about 125 k picks, over the cap
    shape = tuple(n * brick + 1 for n in cb)
    idx = mesh._probe_indices(torch.zeros(cb, dtype=torch.uint8), shape, brick)
    assert idx.shape[0] == mesh.SPARSE_PROBE_CAP and idx.unique().shape[0] == idx.shape[0]
    i = idx // (shape[1] * shape[2])
    per_quarter = torch.bincount(i * 4 // shape[0], minlength=4)
    assert per_quarter.min() > mesh.SPARSE_PROBE_CAP // 5, per_quarter.tolist()  # every quarter along x gets about a quarter
    assert (i % brick == brick // 2).all()                                       # centres
    few = mesh._probe_indices(torch.zeros(20, 20, 20, dtype=torch.uint8), (161, 161, 161), brick)
    assert 8000 // 128 < few.shape[0] < 8000 // 32                               # about one in 64
    assert mesh._probe_indices(torch.ones(3, 3, 3, dtype=torch.uint8), (25, 25, 25), brick).shape[0] == 0


def test_limits_are_refused_before_any_work():
    from nefii_amd import mesh, ops
    for shape, brick in (((4097, 9, 9), 8), ((9, 9, 1), 8), ((9, 9, 9), 1), ((9, 9, 9), 9), ((4096, 4096, 4096), 2)):
        with pytest.raises(ValueError):
            ops.brick_dims(shape, brick)
    assert ops.brick_dims((4096, 4096, 4096), 8) == ((512,) * 3, (512,) * 3)
    assert ops.brick_dims((4089, 9, 9), 8)[1][0] == 512 and ops.brick_dims((4089, 9, 9), 8)[0][0] == 511

    calls = []

    def sample(idx):
        calls.append(idx)
        return idx.float()

    with pytest.raises(ValueError):
        ops.marching_cubes_sparse(sample, (5000, 9, 9), torch.zeros(1, 1, 1), 0.0, (0, 0, 0), (1, 1, 1))
    assert not calls
    net = torch.nn.Linear(3, 1)                                                  # stands for a network that is not on the GPU
    with pytest.raises(ValueError, match='4096'):
        mesh.extract_mesh(net, resolution=5000, bound=1.0, sparse=True)
    with pytest.raises(ValueError, match='brick'):
        mesh.extract_mesh(net, resolution=64, bound=1.0, sparse=True, brick=16)
    with pytest.raises(ValueError, match='GPU'):
        mesh.extract_mesh(net, resolution=64, bound=1.0, sparse=True)


def test_the_source_is_built_and_the_entries_refuse_on_the_host():
    import ctypes
    from nefii_amd import _lib, build
    assert 'nefii_mcubes_sparse.hip' in build.SOURCES
    with open(os.path.join(ROOT, 'include', 'nefii_amd.h')) as f:
        header = f.read()
    lib = _lib.lib()
    for name in ('nefii_mcubes_classify_bricks', 'nefii_mcubes_sparse_count', 'nefii_mcubes_sparse_emit'):
        assert name in _lib.SIGNATURES and 'int %s(' % name in header and getattr(lib, name) is not None
    assert lib.nefii_abi_version() == 19
    E_ARG, E_SHAPE = -1, -2
    p = ctypes.c_void_p(256)                                  # never dereferenced: every call below returns before a launch
    frame = (ctypes.c_double * 12)(*([0.0] * 3 + [0.1, 0, 0, 0, 0.1, 0, 0, 0, 0.1]))
    bad_frame = (ctypes.c_double * 12)(*([float('nan')] + [0.0] * 11))

    def classify(cells=p, G=16, radius=1.0, shape=(9, 9, 9), fr=frame, level=0.0, B=8, out=p):
        return lib.nefii_mcubes_classify_bricks(cells, G, radius, *shape, fr, level, B, out, None)

    assert classify(cells=None) == E_ARG and classify(out=None) == E_ARG and classify(fr=bad_frame) == E_ARG
    assert classify(radius=0.0) == E_ARG and classify(level=float('inf')) == E_ARG
    assert classify(G=1) == E_SHAPE and classify(G=641) == E_SHAPE and classify(B=1) == E_SHAPE and classify(B=9) == E_SHAPE
    assert classify(shape=(4097, 9, 9)) == E_SHAPE and classify(shape=(9, 1, 9)) == E_SHAPE
    assert classify(shape=(4096, 4096, 4096), B=2) == E_SHAPE                 # 2^33 bricks

    def count(vals=p, smap=p, slots=1, shape=(9, 9, 9), B=8, alist=p, n=1, level=0.0, cnt=p):
        return lib.nefii_mcubes_sparse_count(vals, smap, slots, *shape, B, alist, n, level, cnt, None)

    assert count(vals=None) == E_ARG and count(n=0) == E_ARG and count(slots=0) == E_ARG and count(level=float('nan')) == E_ARG
    assert count(shape=(9, 9, 5000)) == E_SHAPE and count(B=16) == E_SHAPE

    def emit(vals=p, shape=(9, 9, 9), B=8, origin=(0.0, 0.0, 0.0), max_verts=1, keys=p):
        return lib.nefii_mcubes_sparse_emit(vals, p, 1, *shape, B, p, 1, 0.0, *origin, 1.0, 1.0, 1.0, p, keys, p, max_verts, p, p,
                                            1, None)

    assert emit(vals=None) == E_ARG and emit(keys=None) == E_ARG and emit(max_verts=-1) == E_ARG
    assert emit(origin=(0.0, float('inf'), 0.0)) == E_ARG and emit(shape=(1, 9, 9)) == E_SHAPE


def test_command_line_knows_the_flags(capsys):
    from nefii_amd.scripts import extract_mesh as cli
    opt = cli.build_parser().parse_args(['--conf', 'x.conf', '--resolution', '2048', '--sparse', '--brick', '4'])
    assert opt.sparse and opt.brick == 4 and opt.resolution == 2048
    opt = cli.build_parser().parse_args(['--conf', 'x.conf'])
    assert not opt.sparse and opt.brick == 8
    with pytest.raises(SystemExit) as e:
        cli.build_parser().parse_args(['--sparse', '--help'])
    assert e.value.code == 0
    assert '--sparse' in capsys.readouterr().out
