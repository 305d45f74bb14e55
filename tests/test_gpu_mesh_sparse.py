"""Sparse mesh export on the GPU (DESIGN.md 6f "Sparse export"): the brick kernels against dense marching cubes and the numpy
oracle on given volumes, the classification against its NumPy restatement bit for bit, extract_mesh(sparse=True) against the
dense export on a fitted scene net, the audit on doctored intervals, and a grid beyond what int32 keys could index."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import mc_ref  # noqa: E402
import mesh_sparse_ref as ref  # noqa: E402
from test_gpu_mesh import scene_model, smooth_field  # noqa: E402

DEV = torch.device('cuda:0')


# ---- 1. the kernels against dense marching cubes, on given volumes ---------------------------------------------------------
def run_sparse(vol, active, level, origin, spacing, brick):
    """marching_cubes_sparse on samples of `vol`; asserts that no grid point is sampled twice"""
    from nefii_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(DEV)
    flat = t.reshape(-1)
    seen = torch.zeros(flat.shape[0], device=DEV, dtype=torch.int32)

    def sample(idx):
        assert idx.dtype == torch.int64
        seen.index_add_(0, idx, torch.ones_like(idx, dtype=torch.int32))
        return flat[idx]

    stats = {}
    v, f = ops.marching_cubes_sparse(sample, vol.shape, torch.from_numpy(active).to(DEV), level, origin, spacing, brick,
                                     chunk=32768, stats=stats)
    assert int(seen.max()) <= 1, 'a grid point was evaluated twice'
    assert stats['evaluated_points'] == int(seen.sum())
    return v, f


def sparse_vs_dense(vol, level, origin, spacing, brick, seed):
    from nefii_amd import mesh
    t = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(DEV)
    dv, df = mesh.marching_cubes(t, level, spacing=spacing, origin=origin)
    rv, rf = mc_ref.marching_cubes(vol, level, origin, spacing)
    crossing = ref.crossing_bricks(vol, level, brick)
    r = np.random.default_rng(seed)
    extra = (crossing | (r.random(crossing.shape) < 0.3)).astype(np.uint8)
    for active in (crossing, extra, np.ones_like(crossing)):
        v, f = run_sparse(vol, active, level, origin, spacing, brick)
        assert v.dtype == torch.float32 and f.dtype == torch.int64
        assert tuple(v.shape) == tuple(dv.shape) and tuple(f.shape) == tuple(df.shape), (v.shape, dv.shape, f.shape, df.shape)
        assert torch.equal(v, dv) and torch.equal(f, df)
        assert np.array_equal(f.cpu().numpy(), rf)
    v2, f2 = run_sparse(vol, crossing, level, origin, spacing, brick)
    assert torch.equal(v, v2) and torch.equal(f, f2)                             # two runs: the same bits
    return crossing


@pytest.mark.parametrize('shape,brick', [((2, 2, 2), 8), ((9, 9, 9), 8), ((10, 9, 17), 8), ((37, 21, 50), 8),
                                         ((70, 64, 57), 8), ((70, 64, 57), 4)])
def test_sparse_kernels_match_dense_marching_cubes(shape, brick):
    from nefii_amd import ops
    r = np.random.default_rng(3)
    ties = r.integers(-2, 3, shape).astype(np.float32) * 0.5                     # exact ties with the level included
    sparse_vs_dense(ties, 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), brick, 1)
    sparse_vs_dense(ties, 0.5, (-1.0, 2.0, 0.25), (0.5, 0.25, 2.0), brick, 2)
    sparse_vs_dense(smooth_field(shape, seed=5), 0.1, (-1.5, -1.0, -0.75), (0.01, 0.02, 0.03), brick, 3)
    # a sphere: most bricks hold no crossing, so the active set is a thin shell (integer radius^2: ties on the axes)
    X, Y, Z = np.meshgrid(*[np.arange(n, dtype=np.float32) - (n - 1) // 2 for n in shape], indexing='ij')
    sphere = X * X + Y * Y + Z * Z - np.float32(min(shape) // 3) ** 2
    crossing = sparse_vs_dense(sphere, 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), brick, 4)
    if min(shape) > 3 * brick:
        assert 0 < crossing.sum() < crossing.size
    # no crossing at all, and no active brick over a volume that has crossings
    cb, _ = ops.brick_dims(shape, brick)
    for vol, active in ((np.ones(shape, np.float32), np.ones(cb, np.uint8)), (ties, np.zeros(cb, np.uint8))):
        v, f = run_sparse(vol, active, 0.0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), brick)
        assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == torch.int64


# ---- 2. classification against the NumPy restatement, bit for bit ---------------------------------------------------------
def random_cells(G, seed, nan=False):
    r = np.random.default_rng(seed)
    # a smooth field with a spread per cell, so that runs of cells exclude the level and others do not
    e = np.linspace(-1, 1, G)
    X, Y, Z = np.meshgrid(e, e, e, indexing='ij')
    mid = np.sqrt(X * X + Y * Y + Z * Z) - 0.3 + 0.02 * r.normal(size=(G, G, G))
    half = 0.03 + 0.05 * r.random((G, G, G))
    lo, hi = (mid - half).astype(np.float32), (mid + half).astype(np.float32)
    if nan:
        lo[r.random((G, G, G)) < 0.002] = np.nan
        hi[r.random((G, G, G)) < 0.002] = np.inf
    return ref.pack_cells(lo, hi)


def uniform_frame(res, bound):
    sp = 2.0 * bound / (res - 1)
    return (res,) * 3, [-bound] * 3, [[sp, 0.0, 0.0], [0.0, sp, 0.0], [0.0, 0.0, sp]]


def rotated_frame(shape, sp, centre):
    steps = sp * ref.rotation((1.0, 2.0, 3.0), 0.7)
    p0 = np.asarray(centre) - sum(steps[a] * (shape[a] - 1) / 2 for a in range(3))
    return shape, p0.tolist(), steps.tolist()


CLASSIFY_CASES = {
    # G = 16 over [-1, 1]^3: interval cells of edge 0.125
    'under one cell per brick': (uniform_frame(145, 0.9), 8, False),             # brick 0.1
    'exactly one cell per brick': (uniform_frame(129, 1.0), 8, False),           # brick 0.125, and the box ends AT the cube
    'about 100 cells per brick (wave per brick)': (uniform_frame(28, 0.95), 8, False),     # brick 0.563: 5 or 6 cells per axis
    'brick of 4': (uniform_frame(77, 0.8), 4, False),
    'rotated': (rotated_frame((90, 70, 81), 0.0125, (0.05, -0.02, 0.0)), 8, False),
    'rotated, wave per brick': (rotated_frame((30, 23, 27), 0.04, (0.0, 0.05, -0.05)), 8, False),
    'sticking out of the cube': (uniform_frame(100, 1.3), 8, False),
    'rotated and sticking out': (rotated_frame((60, 60, 60), 0.03, (0.3, 0.0, 0.0)), 8, False),
    'non-finite words': (uniform_frame(97, 0.9), 8, True),
    'non-finite words, wave per brick': (uniform_frame(28, 0.95), 8, True),
}


@pytest.mark.parametrize('case', list(CLASSIFY_CASES))
def test_classification_matches_the_restatement(case):
    from nefii_amd import ops
    (shape, p0, steps), brick, nan = CLASSIFY_CASES[case]
    cells = random_cells(16, 11, nan)
    for level in (0.0, 0.1):
        want = ref.classify_bricks(cells, 1.0, shape, p0, steps, level, brick)
        got = ops.classify_bricks(torch.from_numpy(cells).to(DEV), 1.0, (shape, p0, steps), level, brick)
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
        diff = got.cpu().numpy() != want
        assert not diff.any(), (case, level, int(diff.sum()), np.argwhere(diff)[:5].tolist())
        assert want.any() and not want.all(), 'the case decides nothing'


# ---- 3. end to end on a network with a grid --------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def bowl():
    model, _, _ = scene_model('bowl_trained', 'conf')
    return model


def same_mesh(a, b):
    for name in ('verts', 'faces', 'normals', 'diffuse_albedo', 'roughness', 'specular_reflection'):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.dtype == y.dtype and torch.equal(x, y), name


def test_sparse_export_equals_the_dense_export(bowl, monkeypatch):
    from nefii_amd import ops
    from nefii_amd.mesh import extract_mesh
    monkeypatch.setattr(ops, 'BOUND_GRID_SIZE', 64)
    dense = extract_mesh(bowl, resolution=192)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        sparse = extract_mesh(bowl, resolution=192, sparse=True)
    s = sparse.meta['sparse']
    print('[sparse export] r 192, G 64: %s; grid %.4f s against %.4f s dense' % (s, sparse.meta['grid_s'], dense.meta['grid_s']))
    assert 'sparse' not in dense.meta
    assert dense.verts.shape[0] > 1000
    same_mesh(sparse, dense)
    assert s['audit_violations'] == 0 and s['fallback'] is None
    assert s['brick'] == 8 and s['bricks'] == 24 ** 3 and s['dense_points'] == 192 ** 3
    assert s['active_bricks'] < s['bricks'] / 2
    assert s['evaluated_points'] < s['dense_points'] and s['probes'] > 0


def test_sparse_export_on_the_aligned_grid(bowl, monkeypatch):
    from nefii_amd import mesh, ops
    # G = 128: at G = 64 the share of active bricks on this grid was 45 %, too close to the cap below to rest a test on
    monkeypatch.setattr(ops, 'BOUND_GRID_SIZE', 128)
    kw = dict(resolution=96, high_res=True, low_resolution=48, keep='largest')
    dense = mesh.extract_mesh(bowl, **kw)
    # the aligned grid's points at arbitrary indices are the rows of the dense function (an fp64 [N,3] @ [3,3] product
    # whose rows do not depend on each other)
    grid = mesh.aligned_grid(dense.verts, 40, 0.2)
    n = grid.numel()
    idx = torch.randint(0, n, (20000,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(0))
    assert torch.equal(grid.points_at(idx, DEV), grid.points(0, n, DEV)[idx])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        sparse = mesh.extract_mesh(bowl, sparse=True, **kw)
    s = sparse.meta['sparse']
    print('[sparse export] aligned %s, G 128: %s' % (sparse.meta['grid_shape'], s))
    same_mesh(sparse, dense)
    assert sparse.meta['grid_shape'] == dense.meta['grid_shape']
    assert s['audit_violations'] == 0 and s['fallback'] is None
    assert s['active_bricks'] < s['bricks'] / 2
    assert s['evaluated_points'] < s['dense_points']


# ---- 4. the audit ----------------------------------------------------------------------------------------------------------
def test_doctored_intervals_are_caught_and_the_export_repeated(monkeypatch):
    from nefii_amd import ops
    from nefii_amd.mesh import extract_mesh
    bowl, _, _ = scene_model('bowl_trained', 'conf')                            # its own network: the audit drops its grid
    net = bowl.implicit_network
    R = float(bowl.object_bounding_sphere)
    res, B, G = 192, 8, 64
    dense = extract_mesh(bowl, resolution=res, materials=False)
    cells = net.bound_grid(radius=R, G=G)
    assert cells is not None
    # the brick around a vertex of the surface, and every interval cell its box touches (one more on each side)
    sp = 2.0 * R / (res - 1)
    v = dense.verts[dense.verts.shape[0] // 2].double().cpu().numpy()
    b = np.floor((v + R) / sp / B).astype(int)
    c0 = np.clip(np.floor(b * B * sp / (2 * R / G)).astype(int) - 1, 0, G - 1)
    c1 = np.clip(np.floor((b + 1) * B * sp / (2 * R / G)).astype(int) + 1, 0, G - 1)
    doctored = cells.clone()
    word = int(ref.pack_cells(np.float32(0.5), np.float32(1.0)))                 # 0.5 <= sdf <= 1: no surface here
    doctored[c0[0]:c1[0] + 1, c0[1]:c1[1] + 1, c0[2]:c1[2] + 1] = word
    monkeypatch.setattr(ops, 'BOUND_GRID_SIZE', G)
    net._grid = net._grid[:3] + (G, doctored, None)
    assert net.bound_grid(radius=R) is doctored
    # with a dense limit below this grid the repeat cannot be the dense path: it is the brick kernels with every brick active
    with monkeypatch.context() as m, pytest.warns(UserWarning, match='sparse mesh export'):
        m.setattr(ops, 'MCUBES_MAX_POINTS', res ** 3 - 1)
        sparse = extract_mesh(bowl, resolution=res, materials=False, sparse=True)
    s = sparse.meta['sparse']
    print('[sparse export] doctored: %s' % (s,))
    assert s['fallback'] == 'audit' and s['audit_violations'] > 0
    assert s['active_bricks'] == s['bricks'] and s['evaluated_points'] == res ** 3
    assert net._grid is None and net.bound_grid(radius=R) is None                # dropped, and not rebuilt for these weights
    same_mesh(sparse, dense)
    # ... and the next sparse export of this network says that it has no grid
    again = extract_mesh(bowl, resolution=res, materials=False, sparse=True)
    assert again.meta['sparse']['fallback'] == 'no_grid'
    same_mesh(again, dense)


def test_a_violation_that_only_a_probe_can_see(monkeypatch):
    """Intervals that exclude the level EVERYWHERE, on a grid that ends inside the cube: no brick is active, so nothing is
    evaluated and audit (a) has nothing to hold - only the probes of the skipped bricks can tell that the surface is there."""
    from nefii_amd import ops
    from nefii_amd.mesh import extract_mesh
    bowl, _, _ = scene_model('bowl_trained', 'conf')
    net = bowl.implicit_network
    R = float(bowl.object_bounding_sphere)
    res, G = 96, 64
    dense = extract_mesh(bowl, resolution=res, bound=0.9 * R, materials=False)
    assert dense.verts.shape[0] > 1000
    monkeypatch.setattr(ops, 'BOUND_GRID_SIZE', G)
    cells = net.bound_grid(radius=R)
    word = int(ref.pack_cells(np.float32(0.5), np.float32(1.0)))                 # 0.5 <= sdf <= 1 in every cell
    doctored = torch.full_like(cells, word)
    net._grid = net._grid[:3] + (G, doctored, None)
    active = ops.classify_bricks(doctored, R, ((res,) * 3, [-0.9 * R] * 3, (np.eye(3) * 1.8 * R / (res - 1)).tolist()), 0.0)
    assert int(active.sum()) == 0
    with pytest.warns(UserWarning, match='sparse mesh export'):
        sparse = extract_mesh(bowl, resolution=res, bound=0.9 * R, materials=False, sparse=True)
    s = sparse.meta['sparse']
    print('[sparse export] probes only: %s' % (s,))
    assert s['fallback'] == 'audit' and s['probes'] >= 12 ** 3 // 128
    assert 0 < s['audit_violations'] <= s['probes']                              # nothing but probes was held
    assert net._grid is None
    same_mesh(sparse, dense)


# ---- 5. beyond the dense limit ---------------------------------------------------------------------------------------------
def test_grid_beyond_int32_keys_around_a_plane():
    from nefii_amd import ops
    shape, B = (4096, 4096, 64), 8                                               # 2^30 points: owner * 3 + axis passes 2^31
    x0 = 4000.25                                                                 # the plane x = x0; every value exact in fp32
    cb, _ = ops.brick_dims(shape, B)
    active = torch.zeros(cb, device=DEV, dtype=torch.uint8)
    active[4000 // B] = 1
    ny, nz = shape[1], shape[2]
    stats = {}
    v, f = ops.marching_cubes_sparse(lambda idx: (idx // (ny * nz)).float() - x0, shape, active, 0.0, (0.0, 0.0, 0.0),
                                     (1.0, 0.5, 2.0), B, stats=stats)
    assert stats['evaluated_points'] == 2 * B * ny * nz                          # the layer of bricks and its upper neighbour
    assert v.shape == (ny * nz, 3) and f.shape == (2 * (ny - 1) * (nz - 1), 3)
    j = torch.arange(ny, device=DEV, dtype=torch.float32)
    k = torch.arange(nz, device=DEV, dtype=torch.float32)
    want = torch.stack([torch.full((ny, nz), x0, device=DEV), (j * 0.5)[:, None].expand(ny, nz),
                        (k * 2.0)[None, :].expand(ny, nz)], -1).reshape(-1, 3)
    assert torch.equal(v, want)                                                  # t = 0.25 / 1 exactly; order (y, z)
    assert int(f.min()) == 0 and int(f.max()) == ny * nz - 1
    a, b, c = (v[f[:, q]] for q in range(3))
    nrm = torch.linalg.cross(b - a, c - a)
    assert bool((nrm[:, 0] > 0).all()) and bool((nrm[:, 1:] == 0).all())         # towards increasing values


def test_limits_are_refused_before_anything_is_allocated(bowl, monkeypatch):
    from nefii_amd import ops
    from nefii_amd.mesh import extract_mesh
    extract_mesh(bowl, resolution=32, materials=False)                           # weights packed, caches warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match='4096'):
        ops.marching_cubes_sparse(lambda idx: idx.float(), (4097, 9, 9), torch.ones(1, 1, 1, device=DEV), 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match='4096'):
        extract_mesh(bowl, resolution=4097, sparse=True)
    monkeypatch.setattr(bowl.implicit_network, 'bound_grid', lambda *a, **k: None)
    with pytest.raises(ValueError, match='interval grid'):
        extract_mesh(bowl, resolution=1400, sparse=True)                         # no grid, and too large for the dense path
    monkeypatch.undo()
    monkeypatch.setattr(bowl.ray_tracer, 'precision', 'f32')
    with pytest.raises(ValueError, match='precision'):
        extract_mesh(bowl, resolution=1400, sparse=True)
    assert torch.cuda.max_memory_allocated() - before < 1 << 20
    m = extract_mesh(bowl, resolution=40, materials=False, sparse=True)          # where the dense path fits, it runs
    assert m.meta['sparse']['fallback'] == 'precision'
    same_mesh(m, extract_mesh(bowl, resolution=40, materials=False))
