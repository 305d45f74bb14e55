"""The generalized winding number through the BVH kernel on the GPU: mesh_bvh.build_moments and
nefii_mesh_winding_query against MeshSDF(method='brute').winding in fp64 and against the numpy walk of the same tree
(meshwinding_ref.walk_winding), its bitwise guarantees, then MeshSDF(sign='winding'), the sampler and the Step-1 runner on it.

Tolerances.  beta = 0 is the exact sum: |w_kernel - w_brute| <= 1e-11 (fp64 eps 2.2e-16 through a few thousand additions of
terms <= 2 pi, in another frame and another order; 1e-10 on the 262 144-face torus).  Measured: 6.4e-14 at the most, except
9.1e-12 on the 1 x 1 x 1e-3 box, whose queries come within 1e-3 of an edge, where both arguments of atan2 are small and the
1e-16 by which the two frames' coordinates differ is amplified accordingly.  beta > 0: the kernel makes the walk's
decisions, so it equals the walk to 1e-11 - except where a decision itself hangs on rounding: a query is decision-fragile if
at some inner node it visits |dot(d, d) - (beta r)^2| <= 1e-12 (beta r)^2.  Such queries may make up 0.1 % of a batch - a
guard, not an allowance: the seeded batches have none (test_mesh_winding_cpu.py asserts that).  Signs at beta = 2 equal the
brute-force winding signs wherever |w_brute - 0.5| > E(2) = meshwinding_ref.guard_band(2), twice the largest truncation error
measured on the CPU; at most 1 % of a batch may lie inside that band."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import meshbvh_ref as mr  # noqa: E402
import meshwinding_ref as wr  # noqa: E402
from test_geometry_cpu import box_mesh  # noqa: E402

from nefii_amd.datasets.sdf_dataset import MeshSDF, SDFSampler  # noqa: E402
from nefii_amd.mesh_bvh import build_moments  # noqa: E402

DEV = torch.device('cuda')
pytestmark = pytest.mark.gpu
TOL = 1e-11


def tree_of(verts, faces, beta=2.0, **kw):
    return MeshSDF(verts, faces, device=DEV, method='bvh', sign='winding', winding_beta=beta, **kw)


def kernel(m, q, beta):
    """nefii_mesh_winding_query on queries q [P, 3] (a GPU tensor in the tree's frame), as given"""
    from nefii_amd import ops
    t = m.bvh
    return ops.mesh_winding_query(t.node_box, build_moments(t), t.n_leaves, t.tris, t.leaf_size, q, beta)


def exact_agrees(verts, faces, p, what, tol=TOL):
    got = tree_of(verts, faces, beta=0.0).winding(p).cpu().numpy()
    ref = MeshSDF(verts, faces).winding(p).numpy()
    err = np.abs(got - ref).max() if len(ref) else 0.0
    print('%s max |w_kernel - w_brute| = %.3g over %d queries' % (what, err, len(ref)))
    assert got.shape == ref.shape and err <= tol, err


@pytest.mark.parametrize('F', [1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 33])
def test_exact_sum_on_small_and_ragged_shapes(F):
    """a partial last leaf, a one-leaf tree, padding leaves; a partial wave, more than one workgroup"""
    verts, faces = wr.mesh('closed')
    faces = faces[:F]
    rng = np.random.default_rng(200 + F)
    p_all = np.concatenate([mr.surface_points(verts, faces, 129, rng) + rng.normal(0, 0.0025, (129, 3)),
                            rng.uniform(-1, 1, (128, 3))])
    rng.shuffle(p_all)
    for P in (1, 63, 65, 257):
        exact_agrees(verts, faces, p_all[:P], 'F %d P %d:' % (F, P))
    empty = tree_of(verts, faces, beta=0.0).winding(np.zeros((0, 3)))
    assert empty.shape == (0,) and empty.dtype == torch.float64 and empty.is_cuda


@pytest.mark.parametrize('case', ['equal_morton', 'sliver_box'])
def test_exact_sum_on_degenerate_geometry(case):
    rng = np.random.default_rng(7)
    if case == 'equal_morton':
        verts, faces = mr.equal_morton_mesh()
        p = rng.uniform(-0.7, 0.7, (512, 3))
    else:
        verts, faces, _ = box_mesh((-0.5, -0.5, -0.0005), (0.5, 0.5, 0.0005))
        p = rng.uniform(-0.6, 0.6, (1024, 3)) * np.array([1, 1, 0.005])
    exact_agrees(verts, faces, p, case + ':')
    if case == 'sliver_box':
        w = tree_of(verts, faces, beta=0.0).winding(p).cpu().numpy()
        inside = (np.abs(p[:, :2]) < 0.5).all(1) & (np.abs(p[:, 2]) < 0.0005)
        assert np.abs(np.abs(w) - inside).max() <= TOL and 50 < inside.sum() < 974


def test_queries_on_the_surface_are_finite():
    """on a vertex or in a face's plane w jumps, so there is nothing to compare - but every term is finite"""
    verts, faces = wr.mesh('closed')
    on = np.concatenate([verts, verts[faces].mean(1)])
    for beta in (0.0, 2.0):
        w = tree_of(verts, faces, beta=beta).winding(on)
        assert torch.isfinite(w).all() and w.abs().max().item() < 2.0, beta


@functools.lru_cache(maxsize=None)
def walk_case(kind, beta):
    """(tree MeshSDF, queries 'walk' in the tree's frame on the GPU, the numpy walk of the GPU-built tree, its fragile set)"""
    verts, faces = wr.mesh(kind)
    m = tree_of(verts, faces, beta=beta, sort_queries=False)
    q = (torch.from_numpy(wr.queries(kind, 'walk')).to(DEV) @ m.R.T).contiguous()
    w, frag, _ = wr.walk_winding(m.bvh, build_moments(m.bvh), q.cpu().numpy(), beta)
    return m, q, w, frag


@pytest.mark.parametrize('kind', ['closed', 'open', 'union'])
def test_the_kernel_makes_the_walks_decisions(kind):
    m, q, w_walk, frag = walk_case(kind, 2.0)
    got = kernel(m, q, 2.0).cpu().numpy()
    err = np.abs(got - w_walk)[~frag].max()
    print('%s beta 2: max |w_kernel - w_walk| = %.3g over %d queries, %d decision-fragile' % (kind, err, len(w_walk), frag.sum()))
    assert frag.mean() <= 1e-3 and err <= TOL
    ref = MeshSDF(*wr.mesh(kind)).winding(wr.queries(kind, 'walk')).numpy()
    trunc = np.abs(got - ref).max()
    print('%s beta 2: max |w_kernel - w_brute| = %.4g (E(2) = %.4g)' % (kind, trunc, wr.guard_band(2.0)))
    assert 1e-6 < trunc <= 2.0 * wr.MEASURED_ERROR[kind, 2.0]


@pytest.mark.parametrize('kind', ['closed', 'open', 'union'])
def test_signs_at_beta_two(kind):
    verts, faces = wr.mesh(kind)
    p = wr.queries(kind, 'table')
    w_brute = MeshSDF(verts, faces, device=DEV).winding(p).cpu().numpy()
    w = tree_of(verts, faces).winding(p).cpu().numpy()
    held = np.abs(w_brute - 0.5) > wr.guard_band(2.0)
    print('%s: %d queries, %d inside the band |w - 0.5| <= %.4g, min |w_brute - 0.5| = %.3g' % (
        kind, len(p), (~held).sum(), wr.guard_band(2.0), np.abs(w_brute - 0.5).min()))
    assert (~held).mean() <= 0.01
    assert np.array_equal(w[held] > 0.5, w_brute[held] > 0.5)
    assert np.array_equal(w_brute[held] > 0.5, wr.inside_count(p, kind)[held] > 0)


def test_deep_tree():
    """262 144 faces: a 17-level tree, every face summed (beta = 0); the reference is brute force on the GPU"""
    verts, faces = mr.torus_mesh(512, 256)
    assert len(faces) == 262144
    rng = np.random.default_rng(5)
    p = np.concatenate([mr.surface_points(verts, faces, 512, rng) + rng.normal(0, 0.0025, (512, 3)),
                        rng.uniform(-1, 1, (512, 3))])
    ref = MeshSDF(verts, faces, device=DEV).winding(p).cpu().numpy()
    m = tree_of(verts, faces, beta=0.0)
    got = m.winding(p).cpu().numpy()
    assert m.bvh.n_leaves == 65536 and m.bvh.levels == 17
    err = np.abs(got - ref).max()
    print('torus 262144: max |w_kernel - w_brute| = %.3g' % err)
    assert err <= 1e-10
    clear = np.abs(mr.torus_sdf(p)) > 0.05
    assert np.abs(got[clear] - (mr.torus_sdf(p[clear]) < 0)).max() <= 1e-10


def test_reproducibility():
    verts, faces = wr.mesh('union')
    m, q, _, _ = walk_case('union', 2.0)
    bits = lambda x: x.view(torch.int64)
    for beta in (0.0, 2.0):
        w = kernel(m, q, beta)
        assert torch.equal(bits(w), bits(kernel(m, q, beta)))                               # two calls
        order = torch.randperm(q.shape[0], generator=torch.Generator().manual_seed(0)).to(DEV)
        assert torch.equal(bits(w[order]), bits(kernel(m, q[order].contiguous(), beta)))    # a query's place does not matter
        assert torch.equal(bits(w[:77]), bits(kernel(m, q[:77].contiguous(), beta)))
    # through MeshSDF: sorted queries give the same bits as unsorted ones, for the winding number and the signed distance
    p = wr.queries('union', 'walk')
    a, b = tree_of(verts, faces, sort_queries=True), tree_of(verts, faces, sort_queries=False)
    assert torch.equal(bits(a.winding(p)), bits(b.winding(p))) and torch.equal(bits(a(p)), bits(b(p)))
    assert torch.equal(bits(b.winding(p)), bits(kernel(m, q, 2.0)))


def test_op_refuses_mismatched_trees():
    from nefii_amd import ops
    m, q, _, _ = walk_case('closed', 2.0)
    t, mo = m.bvh, build_moments(m.bvh)
    assert mo.is_cuda and mo.shape == (2 * t.n_leaves - 1, 8) and mo.data_ptr() % 16 == 0
    with pytest.raises(ValueError):
        ops.mesh_winding_query(t.node_box, mo[:-1], t.n_leaves, t.tris, t.leaf_size, q, 2.0)
    with pytest.raises(ValueError):
        ops.mesh_winding_query(t.node_box, mo, t.n_leaves, t.tris, t.leaf_size, q, 0.5)
    with pytest.raises(RuntimeError):
        ops.mesh_winding_query(t.node_box, mo, t.n_leaves, t.tris, t.leaf_size, q.cpu(), 2.0)


def test_signed_distance_on_the_open_torus_matches_brute():
    verts, faces = wr.mesh('open')
    p = wr.queries('open', 'table')
    ref_mesh = MeshSDF(verts, faces, device=DEV, sign='winding')
    ref, w_brute = ref_mesh(p).cpu().numpy(), ref_mesh.winding(p).cpu().numpy()
    m = tree_of(verts, faces)
    got = m(p).cpu().numpy()
    err = np.abs(np.abs(got) - np.abs(ref)).max()
    held = np.abs(w_brute - 0.5) > wr.guard_band(2.0)
    print('open torus: max |d_bvh - d_brute| = %.3g over %d queries, %d inside the band' % (err, len(p), (~held).sum()))
    assert err <= 1e-10 and (~held).mean() <= 0.01
    assert np.array_equal(np.signbit(got[held]), np.signbit(ref[held]))
    assert np.array_equal(got[held] < 0, wr.inside_count(p, 'open')[held] > 0)
    assert np.array_equal(m(p, signed=False).cpu().numpy(), np.abs(got))                 # the unsigned mode is untouched
    parity = MeshSDF(verts, faces, device=DEV, method='bvh')
    assert parity.sign == 'parity' and torch.equal(parity(p, signed=False), m(p, signed=False))
    assert ((parity(p).cpu().numpy() < 0) != (wr.inside_count(p, 'open') > 0)).sum() >= 1      # what the feature is for


def test_sampler_draws_the_same_positions_under_either_sign():
    verts, faces = wr.mesh('closed')
    s = {k: SDFSampler(None, 4000, device=DEV, mesh=(verts, faces), sign=k) for k in ('parity', 'winding')}
    assert s['winding'].method == 'bvh' and s['winding'].mesh_sdf.sign == 'winding' and s['parity'].mesh_sdf.sign == 'parity'
    pp, dp = s['parity'].sample(torch.Generator().manual_seed(11))
    pw, dw = s['winding'].sample(torch.Generator().manual_seed(11))
    assert torch.equal(pp, pw) and torch.equal(dp.abs(), dw.abs())
    # a closed mesh: the two signs agree (compared as far from the surface as the truncation error was measured)
    far = dp.abs()[:, 0] > wr.CLEAR * s['parity'].scale
    assert far.sum() > 100 and torch.equal(torch.signbit(dp[far]), torch.signbit(dw[far])) and (dw < 0).sum() > 200


def test_geometry_runner_takes_sdf_sign(tmp_path):
    from nefii_amd.training.geometry_train import GeometryTrainRunner
    from test_gpu_renderer import _runner_conf
    verts, faces = wr.mesh('open')
    cfg = _runner_conf(tmp_path)
    r = GeometryTrainRunner(conf=cfg, exps_folder_name=str(tmp_path), expname='s1', new_timestamp='t0', mesh=(verts, faces),
                            scale_to_unit=False, sample_num=256, batch_size=512, max_niters=4, sdf_sign='winding',
                            winding_beta=4.0)
    m = r.train_dataset.sdf_sampler.mesh_sdf
    assert m.sign == 'winding' and m.winding_beta == 4.0 and m.method == 'bvh'
    pts, sdf = next(iter(r.train_dataloader))
    assert pts.shape == (512, 3) and sdf.shape == (512, 1) and pts.is_cuda and m.bvh.node_moment is not None
    loss = r.train_iteration(pts, sdf)
    assert torch.isfinite(loss).item()
    d = GeometryTrainRunner(conf=cfg, exps_folder_name=str(tmp_path), expname='s1', new_timestamp='t1', mesh=(verts, faces),
                            scale_to_unit=False, sample_num=256, batch_size=512, max_niters=4)
    assert d.train_dataset.sdf_sampler.mesh_sdf.sign == 'parity'
