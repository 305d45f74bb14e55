"""The mesh BVH without a GPU: the tree's invariants (nefii_amd/mesh_bvh.py builds on CPU tensors too), the
query kernel's two pruning rules replayed in numpy on the built tree against brute force, the entry point's host-side
argument checks, and the Python-level refusals."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import meshbvh_ref as mr  # noqa: E402
from test_geometry_cpu import box_mesh  # noqa: E402

from nefii_amd.datasets.sdf_dataset import MeshSDF, SDFDataset, SDFSampler  # noqa: E402
from nefii_amd.mesh_bvh import LEAF, build_bvh  # noqa: E402


def corners(verts, faces):
    v = torch.from_numpy(verts)
    f = torch.from_numpy(faces)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def check_invariants(a, b, c):
    F = a.shape[0]
    t = build_bvh(a, b, c)
    N = t.n_leaves
    assert t.leaf_size == LEAF and N & (N - 1) == 0 and N * LEAF >= F and (N == 1 or N * LEAF < 2 * F + 2 * LEAF)
    assert t.node_box.shape == (2 * N - 1, 6) and t.node_box.dtype == torch.float64 and t.tris.shape == (F, 9)
    # the permutation is a permutation, and tris are the faces in that order, bit for bit
    assert torch.equal(torch.sort(t.perm).values, torch.arange(F))
    assert torch.equal(t.tris, torch.cat([a, b, c], 1)[t.perm])
    lo, hi = t.node_box[:, :3], t.node_box[:, 3:]
    # every face is inside its leaf's box
    leaf_of = N - 1 + torch.arange(F) // LEAF
    pts = t.tris.reshape(F, 3, 3)
    assert (pts >= lo[leaf_of][:, None]).all() and (pts <= hi[leaf_of][:, None]).all()
    # every parent contains its children
    for i in range(N - 1):
        for ch in (2 * i + 1, 2 * i + 2):
            assert (lo[i] <= lo[ch]).all() and (hi[i] >= hi[ch]).all(), (i, ch)
    # padding leaves are empty (inverted), the others are not
    used = (F + LEAF - 1) // LEAF
    assert torch.isposinf(lo[N - 1 + used:]).all() and torch.isneginf(hi[N - 1 + used:]).all()
    assert torch.isfinite(t.node_box[N - 1:N - 1 + used]).all() and torch.isfinite(t.node_box[0]).all()
    # two builds are bitwise equal
    u = build_bvh(a, b, c)
    assert torch.equal(t.perm, u.perm) and torch.equal(t.tris, u.tris) and torch.equal(t.node_box, u.node_box)
    return t


@pytest.mark.parametrize('F', [1, 2, 3, 4, 5, 7, 8, 9, 31, 33, 2304])
def test_tree_invariants(F):
    verts, faces = mr.torus_mesh(48, 24)
    a, b, c = corners(verts, faces[:F])
    t = check_invariants(a, b, c)
    assert t.levels == t.n_leaves.bit_length()
    if F == 2304:
        assert t.n_leaves == 1024 and t.levels == 11
        # the Morton order keeps neighbours together: the leaves are far smaller than the mesh
        leaf = t.node_box[t.n_leaves - 1:t.n_leaves - 1 + F // LEAF]
        assert (leaf[:, 3:] - leaf[:, :3]).norm(dim=1).median() < 0.25


def test_degenerate_morton_input():
    verts, faces = mr.equal_morton_mesh()
    a, b, c = corners(verts, faces)
    assert torch.equal((a + b + c), torch.zeros(len(faces), 3, dtype=torch.float64))       # one centroid, exactly
    t = check_invariants(a, b, c)
    assert torch.equal(t.perm, torch.arange(len(faces)))         # equal codes: the stable sort keeps the given order


def test_build_refuses_bad_sizes():
    e = torch.zeros(0, 3, dtype=torch.float64)
    with pytest.raises(ValueError):
        build_bvh(e, e, e)
    one = torch.eye(3, dtype=torch.float64)[None]
    with pytest.raises(ValueError):
        build_bvh(one[:, 0], one[:, 1], one[:, 2], leaf_size=9)


def test_pruning_rules_reproduce_brute_force():
    """The kernel's traversal, replayed in numpy on the built tree of the 2304-face torus, is brute force: the distance
    rule loses no nearest face, the ray rule no crossing - and both do prune."""
    verts, faces = mr.torus_mesh(48, 24)
    m = MeshSDF(verts, faces)
    rng = np.random.default_rng(1)
    p = np.concatenate([mr.surface_points(verts, faces, 32, rng) + rng.normal(0, 0.0025, (32, 3)),
                        rng.uniform(-1, 1, (32, 3))])
    t = build_bvh(m.ra, m.rb, m.rc)
    q = p @ m.R.numpy().T
    d, count, visited = mr.walk_tree(t, q)
    ref = m(p).numpy()
    assert np.abs(d - np.abs(ref)).max() <= 1e-12
    d_np, count_np = mr.brute_numpy(q, t.tris.numpy())
    assert np.abs(d - d_np).max() <= 1e-12
    assert np.array_equal(count, count_np)
    assert np.array_equal(count % 2 == 1, ref < 0)
    analytic = mr.torus_sdf(p)
    clear = np.abs(analytic) > 0.05                         # the inscribed polygon mesh is within 0.002 of the torus
    assert np.array_equal((count % 2 == 1)[clear], (analytic < 0)[clear]) and clear.sum() >= 24 and (ref < 0).sum() > 8
    assert visited.max() < 2304 // 4 and visited[:32].mean() < 64, (visited.max(), visited[:32].mean())


def test_host_side_argument_checks_need_no_gpu():
    from nefii_amd import _lib
    lib = _lib.lib()
    E_ARG, E_SHAPE = -1, -2
    ok = dict(node_box=256, n_leaves=4, tris=512, n_tris=13, leaf=4, points=768, n_points=0, sign=1, out=1024)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.nefii_mesh_sdf_query(a['node_box'], a['n_leaves'], a['tris'], a['n_tris'], a['leaf'], a['points'],
                                        a['n_points'], a['sign'], a['out'], None)

    assert call() == 0                                      # nothing to do: returns before any launch
    for name in ('node_box', 'tris', 'points', 'out'):
        assert call(**{name: None}) == E_ARG, name
    assert call(node_box=264) == E_ARG                      # boxes are read 16 bytes at a time
    for n_tris in (0, -1, 1 << 26):
        assert call(n_tris=n_tris, n_leaves=1 << 26) == E_SHAPE
    assert call(n_tris=(1 << 26) - 1, n_leaves=1 << 24) == 0
    for n_leaves in (0, -4, 3, 6, 2, 1 << 27):              # not a power of two; 2 leaves of 4 hold 8 < 13 faces; too deep
        assert call(n_leaves=n_leaves) == E_SHAPE, n_leaves
    for leaf in (0, -1, 9):
        assert call(leaf=leaf, n_leaves=16) == E_SHAPE
    assert call(leaf=1, n_leaves=16) == 0 and call(leaf=8, n_leaves=2) == 0 and call(leaf=1, n_leaves=8) == E_SHAPE
    assert call(n_points=-1) == E_SHAPE and call(n_points=1 << 31) == E_SHAPE


def test_python_level_refusals():
    v, f, _ = box_mesh((-0.3, -0.2, -0.45), (0.5, 0.35, 0.1))
    with pytest.raises(ValueError):
        MeshSDF(v, f, method='bvh')                         # a CPU mesh: there is no fallback
    with pytest.raises(ValueError):
        MeshSDF(v, f, device='cpu', method='nonsense')
    with pytest.raises(ValueError):
        SDFSampler(None, 8, mesh=(v, f), method='nonsense')
    with pytest.raises(ValueError):
        SDFSampler(None, 8, mesh=(v, f), method='bvh')
    with pytest.raises(ValueError):
        MeshSDF(v, np.array([[0, 0, 1], [2, 2, 2]]))        # nothing left once the zero-area faces are dropped
    from nefii_amd import ops
    t = build_bvh(*corners(v, f))
    with pytest.raises(RuntimeError):
        ops.mesh_sdf_query(t.node_box, t.n_leaves, t.tris, t.leaf_size, torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.mesh_sdf_query(t.node_box, t.n_leaves, t.tris, t.leaf_size, torch.zeros(4, 3))


def test_auto_on_the_cpu_is_brute_force():
    v, f, _ = box_mesh((0.1, 0.0, -0.2), (0.4, 0.2, 0.0))
    got = {}
    for method in ('auto', 'brute'):
        s = SDFSampler(None, 500, mesh=(v, f), method=method)
        assert s.method == 'brute' and s.mesh_sdf.method == 'brute'
        got[method] = s.sample(torch.Generator().manual_seed(5))
    assert torch.equal(got['auto'][0], got['brute'][0]) and torch.equal(got['auto'][1], got['brute'][1])
    ds = SDFDataset(None, 16, 4, mesh=(v, f))
    assert ds.sdf_sampler.method == 'brute'
    m = MeshSDF(v, f)
    p = np.random.default_rng(0).uniform(-0.5, 0.5, (200, 3))
    assert torch.equal(m(p, signed=False), m(p).abs()) and (m(p) < 0).any()


def test_step1_command_line_takes_sdf_method():
    import argparse
    from nefii_amd.training.geometry_train import add_argument
    parse = add_argument(argparse.ArgumentParser()).parse_args
    assert parse(['--conf', 'x']).sdf_method == 'auto' and parse(['--conf', 'x', '--sdf_method', 'bvh']).sdf_method == 'bvh'
    with pytest.raises(SystemExit):
        parse(['--conf', 'x', '--sdf_method', 'octree'])
