"""What the component / aligned-grid export needs no GPU for: the host checks of the nefii_mesh_cc_* entry points, the ops
that refuse CPU tensors, mesh.aligned_grid against a numpy restatement of the reference's get_grid, and the torch plumbing
of mesh.component_table / mesh.select_components on CPU tensors with given labels."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import meshcc_ref as ref  # noqa: E402


def test_entry_points_check_their_arguments_on_the_host():
    from nefii_amd import _lib
    lib = _lib.lib()
    E_ARG, E_SHAPE = -1, -2
    p = ctypes.c_void_p(256)                                  # never dereferenced: every call below returns before a launch
    assert lib.nefii_mesh_cc_init(None, 4, p, None) == E_ARG
    assert lib.nefii_mesh_cc_init(p, 4, None, None) == E_ARG
    assert lib.nefii_mesh_cc_round(None, 1, p, 4, p, None) == E_ARG
    assert lib.nefii_mesh_cc_round(p, 1, None, 4, p, None) == E_ARG
    assert lib.nefii_mesh_cc_round(p, 1, p, 4, None, None) == E_ARG
    for bad in (-1, 1 << 31, 1 << 40):
        assert lib.nefii_mesh_cc_init(p, bad, p, None) == E_SHAPE
        assert lib.nefii_mesh_cc_round(p, 1, p, bad, p, None) == E_SHAPE
        assert lib.nefii_mesh_cc_round(p, bad, p, 4, p, None) == E_SHAPE
    assert lib.nefii_mesh_cc_init(p, 0, p, None) == 0         # no vertices: nothing to launch
    assert lib.nefii_mesh_cc_round(p, 0, p, 0, p, None) == 0
    assert lib.nefii_mesh_cc_round(p, 5, p, 0, p, None) == 0


def test_round_cap():
    from nefii_amd import ops
    assert [ops.mesh_cc_round_cap(v) for v in (0, 1, 2, 3, 4, 5, 1 << 20, (1 << 20) + 1)] == [12, 12, 12, 16, 16, 20, 88, 92]


def test_the_gpu_paths_refuse_cpu_tensors():
    from nefii_amd import mesh, ops, synthetic as syn, conf
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        ops.mesh_components(faces, 3)
    with pytest.raises(ValueError):
        mesh.connected_components(faces.long(), 3)
    model = IDRNetwork(conf.from_dict(syn.model_conf('conf')))
    with pytest.raises(ValueError):
        mesh.extract_mesh(model, resolution=8, high_res=True, low_resolution=8)
    with pytest.raises(ValueError):
        mesh.extract_mesh(model, resolution=8, keep='biggest')


def get_grid_restated(lo, hi, resolution, eps):
    """utils/plots.py get_grid, branch by branch: -> [x, y, z]"""
    shortest = int(np.argmin(hi - lo))
    if shortest == 0:
        x = np.linspace(lo[0] - eps, hi[0] + eps, resolution)
        length = np.max(x) - np.min(x)
        y = np.arange(lo[1] - eps, hi[1] + length / (x.shape[0] - 1) + eps, length / (x.shape[0] - 1))
        z = np.arange(lo[2] - eps, hi[2] + length / (x.shape[0] - 1) + eps, length / (x.shape[0] - 1))
    elif shortest == 1:
        y = np.linspace(lo[1] - eps, hi[1] + eps, resolution)
        length = np.max(y) - np.min(y)
        x = np.arange(lo[0] - eps, hi[0] + length / (y.shape[0] - 1) + eps, length / (y.shape[0] - 1))
        z = np.arange(lo[2] - eps, hi[2] + length / (y.shape[0] - 1) + eps, length / (y.shape[0] - 1))
    else:
        z = np.linspace(lo[2] - eps, hi[2] + eps, resolution)
        length = np.max(z) - np.min(z)
        x = np.arange(lo[0] - eps, hi[0] + length / (z.shape[0] - 1) + eps, length / (z.shape[0] - 1))
        y = np.arange(lo[1] - eps, hi[1] + length / (z.shape[0] - 1) + eps, length / (z.shape[0] - 1))
    return [x, y, z], shortest


# (half-extents in world order before the rotation, rotation, local axes stretched by two outliers, shortest local axis)
CLOUDS = [((0.6, 0.35, 0.2), ref.BOX_ROT, (), 0),
          ((0.2, 0.6, 0.35), ref.rot(0, 50.0) @ ref.rot(2, -15.0), (0,), 1),
          ((0.35, 0.2, 0.6), ref.rot(1, 70.0) @ ref.rot(0, 10.0) @ ref.rot(2, 40.0), (0, 1), 2)]


@pytest.mark.parametrize('case', range(3))
def test_aligned_grid_frame_and_axes(case):
    from nefii_amd import mesh
    half, rotation, stretched, shortest = CLOUDS[case]
    resolution, margin = 48 + 7 * case, (0.2, 0.05, 0.11)[case]
    # `stretched` names LOCAL axes (ascending variance): put the outliers along the matching box axes
    by_extent = np.argsort(half)
    pts = ref.box_cloud(half, rotation, ref.BOX_CENTRE, 20000, seed=case, outliers=[by_extent[a] for a in stretched])
    p = torch.from_numpy(pts)
    g = mesh.aligned_grid(p, resolution, margin)
    assert g.vecs.dtype == np.float64 and g.mean.dtype == np.float64
    assert np.abs(g.vecs @ g.vecs.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(g.vecs) - 1.0) < 1e-12
    cosines = np.abs(g.vecs @ rotation)                        # rows: frame axes, columns: box axes
    assert (cosines.max(1) >= 0.999).all(), cosines
    assert sorted(cosines.argmax(1)) == [0, 1, 2] and cosines.argmax(1).tolist() == by_extent.tolist()   # ascending extent
    for r in range(3):
        assert g.vecs[r, np.abs(g.vecs[r]).argmax()] > 0 or r == 0
    local = g.to_local(p)
    assert local.dtype == torch.float64
    want = (pts - pts.mean(0)) @ g.vecs.T
    assert np.abs(local.numpy() - want).max() < 1e-12
    lo, hi = local.numpy().min(0), local.numpy().max(0)
    axes, want_shortest = get_grid_restated(lo, hi, resolution, margin)
    assert want_shortest == shortest == g.shortest_axis
    assert g.shape == tuple(len(a) for a in axes) and len(g.axes[shortest]) == resolution
    for a in range(3):
        assert np.abs(g.axes[a] - axes[a]).max() <= 1e-12
        assert g.axes[a][0] <= lo[a] - margin + 1e-12 and g.axes[a][-1] >= hi[a] + margin - 1e-12
    assert abs(g.spacing - (axes[shortest][-1] - axes[shortest][0]) / (resolution - 1)) < 1e-15
    assert g.origin == tuple(a[0] for a in axes)
    assert (g.to_world(local) - p).abs().max().item() < 1e-12
    # points(): x slowest, world space, float32
    nx, ny, nz = g.shape
    k = np.array([0, 1, nz, ny * nz, nx * ny * nz - 1])
    got = torch.cat([g.points(int(i), int(i) + 1) for i in k])
    assert got.dtype == torch.float32 and got.shape == (5, 3)
    loc = np.stack([g.axes[0][k // (ny * nz)], g.axes[1][(k // nz) % ny], g.axes[2][k % nz]], 1)
    assert np.abs(got.numpy() - (loc @ g.vecs + g.mean)).max() < 1e-6
    assert torch.equal(g.points(0, nz + 3)[nz:nz + 1], g.points(nz, nz + 1))


def test_aligned_grid_refuses_a_grid_of_2_to_the_31_points_without_allocating():
    from nefii_amd import mesh
    pts = torch.from_numpy(ref.box_cloud((0.6, 0.35, 0.2), np.eye(3), (0, 0, 0), 100, seed=0))
    with pytest.raises(ValueError, match=r'\d{10} points'):
        mesh.aligned_grid(pts, 900, 0.0)                       # 900 x 1574 x 2698 = 3.8e9
    with pytest.raises(ValueError):
        mesh.aligned_grid(pts, 1, 0.2)
    with pytest.raises(ValueError):
        mesh.aligned_grid(pts[:, :2], 10, 0.2)


def small_mesh():
    """four components over 12 vertices: a square of area 1 (2 faces), a square of area 1 further up (2 faces), a triangle
    of area 0.125; vertex 10 is in no face.  Vertex numbers interleaved so that selection has to re-index."""
    verts = torch.tensor([[0, 0, 0], [0, 0, 5], [1, 0, 0], [1, 0, 5], [1, 1, 0], [1, 1, 5], [0, 1, 0], [0, 1, 5],
                          [3, 3, 3], [3.5, 3, 3], [9, 9, 9], [3, 3.5, 3]], dtype=torch.float32)
    faces = torch.tensor([[1, 3, 5], [0, 2, 4], [8, 9, 11], [1, 5, 7], [0, 4, 6]], dtype=torch.int64)
    labels = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1, 8, 8, 10, 8], dtype=torch.int64)
    return verts, faces, labels


def test_component_table_on_cpu_tensors():
    from nefii_amd import mesh
    verts, faces, labels = small_mesh()
    assert np.array_equal(ref.labels(faces.numpy(), 12), labels.numpy())
    ids, n_v, n_f, area = mesh.component_table(verts, faces, labels)
    assert ids.tolist() == [0, 1, 8, 10] and n_v.tolist() == [4, 4, 3, 1] and n_f.tolist() == [2, 2, 1, 0]
    assert area.dtype == torch.float64
    v, f = verts.double().numpy(), faces.numpy()
    tri = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    want = [tri[labels.numpy()[f[:, 0]] == i].sum() for i in ids.tolist()]
    assert np.abs(area.numpy() - np.array(want)).max() <= 1e-12 and want[:3] == [1.0, 1.0, 0.125]
    again = mesh.component_table(verts, faces, labels)
    assert all(torch.equal(a, b) for a, b in zip((ids, n_v, n_f, area), again))


def test_select_components_on_cpu_tensors():
    from nefii_amd import mesh
    verts, faces, labels = small_mesh()
    V = verts.shape[0]
    m = mesh.Mesh(verts, faces, normals=verts * 2, roughness=verts[:, :1] + 1, meta={'resolution': 7})
    assert mesh.select_components(m, 'all') is m
    big = mesh.select_components(m, 'largest', labels=labels)
    keep = labels == 0                                          # both squares have area 1: the smaller id wins
    assert torch.equal(big.verts, verts[keep]) and torch.equal(big.normals, verts[keep] * 2)
    assert torch.equal(big.roughness, verts[keep][:, :1] + 1) and big.diffuse_albedo is None
    assert big.faces.dtype == torch.int64 and big.faces.tolist() == [[0, 1, 2], [0, 2, 3]]     # old order, re-indexed
    assert torch.equal(big.verts[big.faces], verts[faces[[1, 4]]])
    assert big.meta['resolution'] == 7 and m.meta == {'resolution': 7}
    table = big.meta['components']
    assert table['count'] == 4 and table['ids'] == [0, 1, 8, 10] and table['area'] == [1.0, 1.0, 0.125, 0.0]
    assert table['n_verts'] == [4, 4, 3, 1] and table['n_faces'] == [2, 2, 1, 0]
    both = mesh.select_components(m, 1.0, labels=labels)
    assert both.verts.shape[0] == 8 and both.faces.tolist() == [[1, 3, 5], [0, 2, 4], [1, 5, 7], [0, 4, 6]]
    three = mesh.select_components(m, 0.125, labels=labels)
    assert three.verts.shape[0] == 11 and torch.equal(three.verts, verts[labels != 10])
    assert three.faces.tolist() == [[1, 3, 5], [0, 2, 4], [8, 9, 10], [1, 5, 7], [0, 4, 6]]
    assert mesh.select_components(m, '0.5', labels=labels).verts.shape[0] == 8          # as the command line passes it
    for bad in (0.0, 1.5, -1, 'most', float('nan')):
        with pytest.raises(ValueError):
            mesh.select_components(m, bad, labels=labels)
    # more components than rows kept in meta
    n = mesh.COMPONENT_ROWS + 4
    tv = torch.rand(4 * n, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64).float()
    tf = torch.from_numpy(ref.tetrahedra(n))
    tl = torch.from_numpy(ref.labels(tf.numpy(), 4 * n))
    out = mesh.select_components(mesh.Mesh(tv, tf), 'largest', labels=tl)
    t = out.meta['components']
    assert t['count'] == n and len(t['ids']) == mesh.COMPONENT_ROWS and t['area'] == sorted(t['area'], reverse=True)
    assert out.verts.shape[0] == 4 and out.faces.tolist() == ref.TETRA.tolist() and V == 12
