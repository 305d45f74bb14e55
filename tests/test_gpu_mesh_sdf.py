"""The mesh signed-distance query through the BVH kernel on the GPU: MeshSDF(method='bvh') - mesh_bvh.build_bvh
and nefii_mesh_sdf_query - against MeshSDF(method='brute') in fp64 (the code before the kernel existed), closed forms where
there are any, and its bitwise guarantees; then the samplers, the Step-1 runner and extract_mesh's comparison on top of it.

Tolerance: |d_bvh - d_brute| <= 1e-10 at unit scale.  fp64 eps is 2.2e-16 on coordinates <= 1 through a few dozen operations;
the two differ by the frame they work in (the kernel measures in MeshSDF's skewed frame, a rotation) and nothing else.
Signs: parity counts are integers, so they are equal EXACTLY, except where a face's 2-D edge function is smaller than 1e-12
in magnitude at the query (meshbvh_ref.fragile): only there can a product rounded differently flip `covers`.  Such queries
may make up 0.1 % of a batch at the most - a guard, not an allowance: the seeded batches here have none."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import meshbvh_ref as mr  # noqa: E402
from test_geometry_cpu import box_mesh, box_sdf  # noqa: E402

from nefii_amd.datasets.sdf_dataset import MeshSDF, SDFSampler  # noqa: E402
from nefii_amd.mesh_bvh import build_bvh  # noqa: E402

DEV = torch.device('cuda')
pytestmark = pytest.mark.gpu
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def torus():
    return mr.torus_mesh(48, 24)


@functools.lru_cache(maxsize=None)
def torus_queries():
    """2048 queries: half surface samples + N(0, 0.0025^2), half uniform in [-1, 1]^3; with the brute-force reference (CPU)"""
    verts, faces = torus()
    rng = np.random.default_rng(1)
    p = np.concatenate([mr.surface_points(verts, faces, 1024, rng) + rng.normal(0, 0.0025, (1024, 3)),
                        rng.uniform(-1, 1, (1024, 3))])
    ref = MeshSDF(verts, faces)(p).numpy()
    return p, ref


def agree(got, ref, ref_mesh, p, signed=True, tol=TOL, what=''):
    """got / ref: [P] numpy.  Distances within tol; signs equal on every query that is not sign-fragile, those <= 0.1 %."""
    err = np.abs(np.abs(got) - np.abs(ref)).max() if len(ref) else 0.0
    print('%s max |d_bvh - d_brute| = %.3g over %d queries' % (what, err, len(ref)))
    assert got.shape == ref.shape and err <= tol, err
    if signed:
        frag = mr.fragile(ref_mesh, p)
        print('%s sign-fragile queries: %d' % (what, frag.sum()))
        assert frag.mean() <= 1e-3
        assert np.array_equal(np.signbit(got[~frag]), np.signbit(ref[~frag]))


def bvh_of(verts, faces, **kw):
    return MeshSDF(verts, faces, device=DEV, method='bvh', **kw)


def test_box_against_the_closed_form():
    lo, hi = (-0.3, -0.2, -0.45), (0.5, 0.35, 0.1)
    v, f, _ = box_mesh(lo, hi)
    p = np.random.Generator(np.random.Philox(2)).uniform(-0.9, 0.9, size=(4000, 3))
    d = bvh_of(v, f)(p).cpu().numpy()
    ref = box_sdf(p, lo, hi)
    print('box: max |d - closed form| = %.3g' % np.abs(d - ref).max())
    assert np.abs(d - ref).max() < 1e-12                    # signs included
    assert (d < 0).sum() > 100 and (d > 0).sum() > 100
    f2 = np.concatenate([f[:, ::-1], [[0, 0, 1]]])          # winding does not matter, nor do degenerate faces
    assert np.abs(bvh_of(v, f2)(p).cpu().numpy() - ref).max() < 1e-12


def test_torus_against_brute_force_and_the_analytic_sign():
    verts, faces = torus()
    p, ref = torus_queries()
    m = bvh_of(verts, faces)
    d = m(p).cpu().numpy()
    agree(d, ref, MeshSDF(verts, faces), p, what='torus 2304:')
    analytic = mr.torus_sdf(p)
    clear = np.abs(analytic) > 0.05
    assert clear.sum() > 800 and np.array_equal(d[clear] < 0, analytic[clear] < 0)
    assert np.array_equal(m(p, signed=False).cpu().numpy(), np.abs(d))          # the unsigned mode is the same distance
    assert m.bvh.n_leaves == 1024


@pytest.mark.parametrize('F', [1, 2, 3, 4, 5, 7, 8, 9, 31, 33])
def test_small_and_ragged_shapes(F):
    """a partial last leaf, a one-leaf tree, padding leaves; a partial wave and a partial block (unsigned: an open mesh)"""
    verts, faces = torus()
    faces = faces[:F]
    rng = np.random.default_rng(100 + F)
    p_all = np.concatenate([mr.surface_points(verts, faces, 129, rng) + rng.normal(0, 0.0025, (129, 3)),
                            rng.uniform(-1, 1, (128, 3))])
    rng.shuffle(p_all)
    ref_mesh, m = MeshSDF(verts, faces), bvh_of(verts, faces)
    ref_all = ref_mesh(p_all, signed=False).numpy()
    for P in (1, 63, 65, 257):
        got = m(p_all[:P], signed=False).cpu().numpy()
        agree(got, ref_all[:P], ref_mesh, p_all[:P], signed=False, what='F %d P %d:' % (F, P))
        assert (got >= 0).all()
    empty = m(np.zeros((0, 3)))
    assert empty.shape == (0,) and empty.dtype == torch.float64 and empty.is_cuda


@pytest.mark.parametrize('case', ['equal_morton', 'doubled_torus', 'sliver_box'])
def test_degenerate_geometry(case):
    rng = np.random.default_rng(7)
    if case == 'equal_morton':
        verts, faces = mr.equal_morton_mesh()
        p = rng.uniform(-0.7, 0.7, (512, 3))
    elif case == 'doubled_torus':
        verts, faces = torus()
        faces = np.concatenate([faces, faces])
        p = torus_queries()[0][::2]
    else:
        lo, hi = (-0.5, -0.5, -0.0005), (0.5, 0.5, 0.0005)
        verts, faces, _ = box_mesh(lo, hi)
        p = rng.uniform(-0.6, 0.6, (1024, 3)) * np.array([1, 1, 0.005])
    ref_mesh = MeshSDF(verts, faces)
    ref = ref_mesh(p).numpy()
    got = bvh_of(verts, faces)(p).cpu().numpy()
    agree(got, ref, ref_mesh, p, what=case + ':')
    if case == 'doubled_torus':
        assert not np.signbit(got).any() and not np.signbit(ref).any()         # every crossing counts twice
    if case == 'sliver_box':
        assert np.abs(got - box_sdf(p, lo, hi)).max() < 1e-12 and 50 < (got < 0).sum() < 924


def test_special_queries():
    verts, faces = torus()
    m, ref_mesh = bvh_of(verts, faces), MeshSDF(verts, faces)
    on = np.concatenate([verts, verts[faces].mean(1)])      # every vertex, every face centroid: the sign at 0 means nothing
    d = m(on).cpu().numpy()
    print('on the surface: max |d| = %.3g' % np.abs(d).max())
    assert np.abs(d).max() <= TOL
    agree(d, ref_mesh(on).numpy(), ref_mesh, on, signed=False, what='vertices and centroids:')
    rng = np.random.default_rng(3)
    far = rng.normal(size=(256, 3))
    far = 100 * far / np.linalg.norm(far, axis=1, keepdims=True)
    got = m(far).cpu().numpy()
    agree(got, ref_mesh(far).numpy(), ref_mesh, far, what='|p| = 100:')
    assert (got > 99).all()


def test_large_tree():
    """262 144 faces: a 17-level tree; the reference is brute force on the GPU"""
    verts, faces = mr.torus_mesh(512, 256)
    assert len(faces) == 262144
    rng = np.random.default_rng(5)
    p = np.concatenate([mr.surface_points(verts, faces, 512, rng) + rng.normal(0, 0.0025, (512, 3)),
                        rng.uniform(-1, 1, (512, 3))])
    ref_mesh = MeshSDF(verts, faces, device=DEV)
    ref = ref_mesh(p).cpu().numpy()
    m = bvh_of(verts, faces)
    got = m(p).cpu().numpy()
    assert m.bvh.n_leaves == 65536 and m.bvh.levels == 17
    agree(got, ref, ref_mesh, p, what='torus 262144:')
    analytic = mr.torus_sdf(p)
    clear = np.abs(analytic) > 0.05
    assert np.array_equal(got[clear] < 0, analytic[clear] < 0)


def test_reproducibility():
    from nefii_amd import ops
    verts, faces = torus()
    p, _ = torus_queries()
    m = bvh_of(verts, faces)
    t = m.bvh
    q = (torch.from_numpy(p).to(DEV) @ m.R.T).contiguous()

    def query(tree, pts):
        return ops.mesh_sdf_query(tree.node_box, tree.n_leaves, tree.tris, tree.leaf_size, pts, True)

    bits = lambda x: x.view(torch.int64)
    d = query(t, q)
    assert torch.equal(bits(d), bits(query(t, q)))                                      # two calls
    order = torch.randperm(q.shape[0], generator=torch.Generator().manual_seed(0)).to(DEV)
    assert torch.equal(bits(d[order]), bits(query(t, q[order].contiguous())))           # a query's place does not matter
    assert torch.equal(bits(d[:77]), bits(query(t, q[:77].contiguous())))
    # the same faces in another order (corners within a face untouched): another tree, the same bits
    shuffle = torch.randperm(m.ra.shape[0], generator=torch.Generator().manual_seed(1)).to(DEV)
    t2 = build_bvh(m.ra[shuffle], m.rb[shuffle], m.rc[shuffle])
    assert not torch.equal(t2.perm, t.perm)
    assert torch.equal(bits(d), bits(query(t2, q)))
    # through MeshSDF: sorted queries give the same bits as unsorted ones
    a = bvh_of(verts, faces, sort_queries=True)(p)
    b = bvh_of(verts, faces, sort_queries=False)(p)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(m(p)))


@pytest.mark.parametrize('scale_to_unit', [True, False])
def test_sampler_bvh_matches_brute(scale_to_unit):
    verts, faces = torus()
    verts = verts * 3.0 + np.array([0.5, -1.0, 2.0])
    s = {k: SDFSampler(None, 2000, scale_to_unit=scale_to_unit, device=DEV, mesh=(verts, faces), method=k)
         for k in ('bvh', 'brute', 'auto')}
    assert s['auto'].method == 'bvh' and s['bvh'].mesh_sdf.method == 'bvh' and s['brute'].mesh_sdf.method == 'brute'
    pb, db = s['bvh'].sample(torch.Generator().manual_seed(11))
    pr, dr = s['brute'].sample(torch.Generator().manual_seed(11))
    assert torch.equal(pb, pr) and db.shape == dr.shape == (2000, 1)
    scale = s['bvh'].scale
    assert (scale > 2.0) == scale_to_unit
    err = (db - dr).abs().max().item()
    print('sampler (scale_to_unit %s): max |d_bvh - d_brute| = %.3g, scale %.3g' % (scale_to_unit, err, scale))
    assert err <= TOL * scale
    assert torch.equal(torch.signbit(db), torch.signbit(dr)) and (db < 0).sum() > 200


def test_geometry_runner_takes_sdf_method(tmp_path):
    from nefii_amd.training.geometry_train import GeometryTrainRunner
    from test_gpu_renderer import _runner_conf
    lo, hi = (-0.45, -0.3, -0.35), (0.4, 0.35, 0.3)
    v, f, _ = box_mesh(lo, hi)
    cfg = _runner_conf(tmp_path)
    for k, (sdf_method, want) in enumerate([('bvh', 'bvh'), (None, 'bvh'), ('brute', 'brute')]):
        kw = {} if sdf_method is None else {'sdf_method': sdf_method}
        r = GeometryTrainRunner(conf=cfg, exps_folder_name=str(tmp_path), expname='s1', new_timestamp='t%d' % k, mesh=(v, f),
                                scale_to_unit=False, sample_num=256, batch_size=512, max_niters=4, **kw)
        assert r.train_dataset.sdf_sampler.method == want and r.train_dataset.sdf_sampler.mesh_sdf.method == want
        if want == 'bvh':
            pts, sdf = next(iter(r.train_dataloader))
            assert pts.shape == (512, 3) and sdf.shape == (512, 1) and pts.is_cuda
            assert np.abs(sdf[:, 0].cpu().numpy() - box_sdf(pts.double().cpu().numpy(), lo, hi)).max() < 1e-6      # float32 items
            assert r.train_dataset.sdf_sampler.mesh_sdf._bvh is not None
            loss = r.train_iteration(pts, sdf)
            assert torch.isfinite(loss).item()


def test_extract_mesh_compare_through_the_tree(tmp_path):
    from nefii_amd.mesh import Mesh
    from nefii_amd.scripts.extract_mesh import compare
    v, f, _ = box_mesh((-0.5, -0.25, -0.375), (0.25, 0.5, 0.125))         # exact in float32
    path = tmp_path / 'box.obj'
    path.write_text('\n'.join(['v %r %r %r' % tuple(float(t) for t in x) for x in v] +
                              ['f %d %d %d' % tuple(int(k) + 1 for k in t) for t in f]))
    keys = ('accuracy_mean', 'accuracy_max', 'completeness_mean', 'completeness_max')
    for grow in (1.0, 1.0625):                              # the box against itself, and against a slightly larger copy
        mesh = Mesh(torch.from_numpy(v * grow).float().to(DEV), torch.from_numpy(f).to(DEV))
        a = compare(mesh, str(path), 2000, False, DEV, method='auto')
        b = compare(mesh, str(path), 2000, False, DEV, method='brute')
        print('compare (x %g): %s' % (grow, [a[k] for k in keys]))
        for k in keys:
            assert abs(a[k] - b[k]) <= 1e-9, (k, a[k], b[k])
        if grow == 1.0:
            assert a['hausdorff'] <= 1e-12
        else:
            assert 0.005 < a['chamfer'] < 0.03
