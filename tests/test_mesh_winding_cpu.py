"""Winding-number signs without a GPU: the node moments' invariants (mesh_bvh.build_moments runs on CPU tensors
too), the query kernel's traversal replayed in numpy on the built tree against brute force, the truncation error of the dipole
term measured against brute fp64, the two sign tables that motivate the feature as assertions, the entry point's host-side
argument checks and the Python-level refusals."""
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

from nefii_amd.datasets.sdf_dataset import MeshSDF, SDFDataset, SDFSampler  # noqa: E402
from nefii_amd.mesh_bvh import build_bvh, build_moments  # noqa: E402


def corners(verts, faces):
    v = torch.from_numpy(verts)
    f = torch.from_numpy(faces)
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def check_moments(a, b, c):
    t = build_bvh(a, b, c)
    mo = build_moments(t)
    N, leaf, F = t.n_leaves, t.leaf_size, t.n_faces
    assert mo.shape == (2 * N - 1, 8) and mo.dtype == torch.float64 and mo.is_contiguous() and mo.device == t.tris.device
    assert build_moments(t) is mo and t.node_moment is mo                   # cached on the tree
    p, r, n, area = mo[:, 0:3], mo[:, 3], mo[:, 4:7], mo[:, 7]
    # the root holds the direct sums
    nf = 0.5 * torch.cross(b - a, c - a, dim=1)
    assert (n[0] - nf.sum(0)).abs().max() <= 1e-12 and abs(area[0] - nf.norm(dim=1).sum()) <= 1e-12
    pw = (nf.norm(dim=1, keepdim=True) * (a + b + c) / 3).sum(0) / nf.norm(dim=1).sum()
    assert (p[0] - pw).abs().max() <= 1e-12
    # parents are their children's sums: n and area bit for bit (one addition each), area p to rounding
    inner = torch.arange(N - 1)
    assert torch.equal(mo[inner, 4:8], mo[2 * inner + 1, 4:8] + mo[2 * inner + 2, 4:8])
    ap = area[:, None] * p
    assert (ap[inner] - ap[2 * inner + 1] - ap[2 * inner + 2]).abs().max() <= 1e-12 if N > 1 else True
    # empty nodes are exactly the inverted boxes, and their rows are zero; every other node has a positive area and radius
    empty = torch.isposinf(t.node_box[:, 0])
    assert torch.equal(empty, area == 0) and torch.equal(mo[empty], torch.zeros(int(empty.sum()), 8, dtype=torch.float64))
    assert (r[~empty] > 0).all() and torch.isfinite(mo).all()
    # every vertex of a node lies within r of p
    verts = t.tris.reshape(F, 3, 3)
    for node in range(2 * N - 1):
        depth = (node + 1).bit_length() - 1
        span = N >> depth                                                    # leaves under the node
        f0 = (node - ((1 << depth) - 1)) * span * leaf
        v = verts[f0:min(f0 + span * leaf, F)].reshape(-1, 3)
        assert bool(empty[node]) == (v.shape[0] == 0)
        if v.shape[0]:
            assert ((v - p[node]).norm(dim=1) <= r[node]).all(), node
    # two builds are bitwise equal
    assert torch.equal(mo, build_moments(build_bvh(a, b, c)))
    return t, mo


@pytest.mark.parametrize('F', [1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 33, 2304])
def test_moment_invariants(F):
    verts, faces = wr.mesh('closed')
    t, mo = check_moments(*corners(verts, faces[:F]))
    if F == 2304:
        assert mo[0, 4:7].abs().max() <= 1e-12                              # a closed mesh has no net area vector
        # the Morton order keeps neighbours together: a leaf's sphere is far smaller than the mesh's
        assert mo[t.n_leaves - 1:, 3].median() < 0.1 < 1.0 < mo[0, 3]


def test_moments_of_the_equal_morton_mesh():
    verts, faces = mr.equal_morton_mesh()
    check_moments(*corners(verts, faces))


@functools.lru_cache(maxsize=None)
def case(kind):
    """(brute MeshSDF, tree, moments, queries 'walk' in the world frame, the same in the tree's frame, brute-force w in numpy)"""
    verts, faces = wr.mesh(kind)
    m = MeshSDF(verts, faces, sign='winding')
    t = build_bvh(m.ra, m.rb, m.rc)
    p = wr.queries(kind, 'walk')
    q = p @ m.R.numpy().T
    return m, t, build_moments(t), p, q, wr.brute_winding(q, t.tris.numpy())


@pytest.mark.parametrize('kind', ['closed', 'open', 'union'])
def test_exact_walk_is_brute_force(kind):
    m, t, mo, p, q, w_brute = case(kind)
    w, frag, faces = wr.walk_winding(t, mo, q, 0.0)
    err = np.abs(w - w_brute).max()
    print('%s: max |w_walk(0) - w_brute| = %.3g over %d queries' % (kind, err, len(q)))
    assert 600 <= len(q) <= 800 and err <= 1e-12 and not frag.any() and (faces == t.n_faces).all()
    # the dense torch formulation (MeshSDF.winding, world frame) is the same number
    assert np.abs(m.winding(p).numpy() - w_brute).max() <= 1e-12
    off = np.abs(w_brute - np.round(w_brute)).max()
    print('%s: max distance of w from an integer = %.3g' % (kind, off))
    if kind == 'closed':
        assert off <= 1e-12 and set(np.round(w_brute)) == {0.0, 1.0}
    if kind == 'union':
        assert off <= 1e-12 and set(np.round(w_brute)) == {0.0, 1.0, 2.0}
        assert np.array_equal(np.round(w_brute), wr.inside_count(p, kind))
    if kind == 'open':
        assert off > 0.1                                                   # it degrades smoothly near the hole


@pytest.mark.parametrize('beta', [2.0, 4.0])
@pytest.mark.parametrize('kind', ['closed', 'open', 'union'])
def test_approximation_error(kind, beta):
    """The dipole term's truncation error, measured against brute fp64: asserted at twice the measured maximum
    (meshwinding_ref.MEASURED_ERROR), the margin being for other seeds.  The seeded batches hold no decision-fragile query."""
    m, t, mo, p, q, w_brute = case(kind)
    w, frag, faces = wr.walk_winding(t, mo, q, beta)
    err = np.abs(w - w_brute).max()
    print('%s beta %g: max |w_walk - w_brute| = %.4g over %d queries; faces evaluated per query: mean %.1f, max %d of %d; '
          'min |w_brute - 0.5| = %.3g' % (kind, beta, err, len(q), faces.mean(), faces.max(), t.n_faces, np.abs(w_brute - 0.5).min()))
    assert err <= 2.0 * wr.MEASURED_ERROR[kind, beta] <= wr.guard_band(beta)
    assert err > 1e-6 and faces.mean() < t.n_faces / 2                      # it does approximate, and does prune
    assert not frag.any()
    if beta == 2.0:
        assert np.abs(w_brute - 0.5).min() > wr.guard_band(beta)           # no sign of these batches hangs on the approximation


def test_parity_fails_on_the_open_torus_and_winding_does_not():
    verts, faces = wr.mesh('open')
    assert len(faces) == 2232
    p = wr.queries('open', 'table')
    truth = wr.inside_count(p, 'open') > 0
    parity = (MeshSDF(verts, faces)(p) < 0).numpy()
    m = MeshSDF(verts, faces, sign='winding')
    d = m(p)
    winding = (d < 0).numpy()
    print('open torus: %d queries, parity sign wrong on %d, winding sign wrong on %d' % (
        len(p), (parity != truth).sum(), (winding != truth).sum()))
    assert (parity != truth).sum() >= 1 and (winding != truth).sum() == 0
    assert np.array_equal(winding, m.winding(p).numpy() > 0.5)


def test_parity_calls_an_overlap_outside_and_winding_does_not():
    verts, faces = wr.mesh('union')
    assert len(faces) == 4608
    p = wr.queries('union', 'table')
    count = wr.inside_count(p, 'union')
    parity = (MeshSDF(verts, faces)(p) < 0).numpy()
    winding = (MeshSDF(verts, faces, sign='winding')(p) < 0).numpy()
    print('two tori: %d queries, %d in the overlap, parity sign wrong on %d, winding sign wrong on %d' % (
        len(p), (count == 2).sum(), (parity != (count > 0)).sum(), (winding != (count > 0)).sum()))
    assert (count == 2).sum() >= 50
    assert np.array_equal(parity != (count > 0), count == 2) and np.array_equal(winding, count > 0)


def test_an_inside_out_mesh_needs_no_flag():
    verts, faces = wr.mesh('closed')
    _, flipped = wr.mesh('inside_out')
    assert flipped.flags['C_CONTIGUOUS'] and np.array_equal(flipped[:, ::-1], faces)
    p = wr.queries('closed', 'walk')
    a, b = MeshSDF(verts, faces, sign='winding'), MeshSDF(verts, flipped, sign='winding')
    assert a.orientation == 1.0 and b.orientation == -1.0
    assert np.abs(a.winding(p).numpy() + b.winding(p).numpy()).max() <= 1e-12
    da, db = a(p).numpy(), b(p).numpy()
    assert np.abs(da - db).max() <= 1e-12 and np.array_equal(da < 0, mr.torus_sdf(p) < 0) and (da < 0).sum() > 20
    tri = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])                    # a face through the origin: volume 0 -> +1
    assert MeshSDF(tri, np.array([[0, 1, 2]])).orientation == 1.0


def test_host_side_argument_checks_need_no_gpu():
    from nefii_amd import _lib
    lib = _lib.lib()
    E_ARG, E_SHAPE = -1, -2
    ok = dict(node_box=256, node_moment=4096, n_leaves=4, tris=512, n_tris=13, leaf=4, points=768, n_points=0, beta=2.0, out=1024)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.nefii_mesh_winding_query(a['node_box'], a['node_moment'], a['n_leaves'], a['tris'], a['n_tris'], a['leaf'],
                                            a['points'], a['n_points'], a['beta'], a['out'], None)

    assert call() == 0                                      # nothing to do: returns before any launch
    for name in ('node_box', 'node_moment', 'tris', 'points', 'out'):
        assert call(**{name: None}) == E_ARG, name
    assert call(node_box=264) == E_ARG and call(node_moment=4104) == E_ARG             # both are read 16 bytes at a time
    for beta in (float('nan'), -1.0, -0.0 - 1e-300, 1e-300, 0.5, 1.0 - 2.0 ** -53):
        assert call(beta=beta) == E_ARG, beta
    for beta in (0.0, -0.0, 1.0, 2.0, 4.0, 1e6, float('inf')):
        assert call(beta=beta) == 0, beta
    # the shape refusals of nefii_mesh_sdf_query, unchanged
    for n_tris in (0, -1, 1 << 26):
        assert call(n_tris=n_tris, n_leaves=1 << 26) == E_SHAPE
    assert call(n_tris=(1 << 26) - 1, n_leaves=1 << 24) == 0
    for n_leaves in (0, -4, 3, 6, 2, 1 << 27):
        assert call(n_leaves=n_leaves) == E_SHAPE, n_leaves
    for leaf in (0, -1, 9):
        assert call(leaf=leaf, n_leaves=16) == E_SHAPE
    assert call(leaf=1, n_leaves=16) == 0 and call(leaf=8, n_leaves=2) == 0 and call(leaf=1, n_leaves=8) == E_SHAPE
    assert call(n_points=-1) == E_SHAPE and call(n_points=1 << 31) == E_SHAPE


def test_python_level_refusals():
    v, f, _ = box_mesh((-0.3, -0.2, -0.45), (0.5, 0.35, 0.1))
    for bad in (dict(sign='nonsense'), dict(sign=None), dict(sign='winding', winding_beta=0.5), dict(winding_beta=-1.0),
                dict(winding_beta=float('nan'))):
        with pytest.raises(ValueError):
            MeshSDF(v, f, **bad)
        with pytest.raises(ValueError):
            SDFSampler(None, 8, mesh=(v, f), **bad)
        with pytest.raises(ValueError):
            SDFDataset(None, 8, 4, mesh=(v, f), **bad)
    with pytest.raises(ValueError):
        MeshSDF(v, f, method='bvh', sign='winding')         # a CPU mesh: there is still no fallback
    from nefii_amd import ops
    t = build_bvh(*corners(v, f))
    mo = build_moments(t)
    pts = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        ops.mesh_winding_query(t.node_box, mo, t.n_leaves, t.tris, t.leaf_size, pts, 2.0)
    for args in ((t.node_box, mo, t.n_leaves, t.tris, t.leaf_size, pts, 0.5),
                 (t.node_box, mo, t.n_leaves, t.tris, t.leaf_size, pts.float(), 2.0),
                 (t.node_box, mo[:, :6].contiguous(), t.n_leaves, t.tris, t.leaf_size, pts, 2.0)):
        with pytest.raises(ValueError):
            ops.mesh_winding_query(*args)


def test_parity_stays_the_default_bit_for_bit():
    verts, faces = wr.mesh('closed')
    p = wr.queries('closed', 'walk')
    m0, m1, mw = MeshSDF(verts, faces), MeshSDF(verts, faces, sign='parity'), MeshSDF(verts, faces, sign='winding')
    assert m0.sign == 'parity' and m0.winding_beta == 2.0
    bits = lambda x: x.view(torch.int64)
    d = m0(p)
    assert torch.equal(bits(d), bits(m1(p))) and torch.equal(bits(m0(p, signed=False)), bits(mw(p, signed=False)))
    # ... and is still what it was: the crossing parity and the distance of the numpy formulation
    q = p @ m0.R.numpy().T
    d_np, count = mr.brute_numpy(q, torch.cat([m0.ra, m0.rb, m0.rc], 1).numpy())
    assert np.array_equal(d.numpy() < 0, count % 2 == 1) and np.abs(d.abs().numpy() - d_np).max() <= 1e-12
    # the samplers draw the same positions whatever the sign, and the same values by default
    s = {k: SDFSampler(None, 500, mesh=(verts, faces), **kw).sample(torch.Generator().manual_seed(5))
         for k, kw in (('default', {}), ('parity', {'sign': 'parity'}), ('winding', {'sign': 'winding'}))}
    assert torch.equal(s['default'][0], s['parity'][0]) and torch.equal(bits(s['default'][1]), bits(s['parity'][1]))
    assert torch.equal(s['default'][0], s['winding'][0]) and torch.equal(s['default'][1].abs(), s['winding'][1].abs())
    ds = SDFDataset(None, 16, 4, mesh=(verts, faces), sign='winding', winding_beta=4.0)
    assert ds.sdf_sampler.mesh_sdf.sign == 'winding' and ds.sdf_sampler.mesh_sdf.winding_beta == 4.0


def test_step1_command_line_takes_sdf_sign():
    import argparse
    from nefii_amd.training.geometry_train import add_argument
    parse = add_argument(argparse.ArgumentParser()).parse_args
    a = parse(['--conf', 'x'])
    assert a.sdf_sign == 'parity' and a.winding_beta == 2.0
    a = parse(['--conf', 'x', '--sdf_sign', 'winding', '--winding_beta', '4'])
    assert a.sdf_sign == 'winding' and a.winding_beta == 4.0
    with pytest.raises(SystemExit):
        parse(['--conf', 'x', '--sdf_sign', 'normals'])
