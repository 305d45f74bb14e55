"""Mesh simplification on the GPU (csrc/nefii_meshsimplify.hip and the torch layer of nefii_amd/mesh.py) against the fp64
numpy restatement of tests/meshsimplify_ref.py: positions to one fp32 ulp at the coordinate scale, faces, kept faces and
vertex order exactly; then the projection onto a level set, the fitted bowl through extract_mesh, and the command line.
Budget: a few seconds per test (check with --durations)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import meshcc_ref  # noqa: E402
import meshsimplify_ref as ref  # noqa: E402

DEV = torch.device('cuda:0')


def tolerance(verts):
    """one fp32 ulp at the coordinate scale: the one fp32 step is the final rounding (half an ulp); the fp64 sums differ from
    the reference's by their order alone, which the 1 / eps conditioning of the solve leaves below 1e-12 cells"""
    return 2.0 ** -23 * max(1.0, float(np.abs(np.asarray(verts)).max()))


def to_gpu(verts, faces):
    return (torch.from_numpy(np.array(verts, dtype=np.float32)).to(DEV),
            torch.from_numpy(np.array(faces, dtype=np.int64).reshape(-1, 3)).to(DEV))


def gpu_positions(verts, faces, cell, eps=1e-3, clamp=0.5):
    """the kernel's position of EVERY cluster, also of those no face will use -> (pos [C,3] float32 numpy, cluster, C)"""
    from nefii_amd import mesh, ops
    tv, tf = to_gpu(verts, faces)
    cluster, centre, C = mesh.cluster_vertices(tv, tf, cell)
    corners, seg = mesh.corner_runs(tf, cluster, C)
    pos = ops.mesh_cluster_quadrics(tv, tf.int(), cluster.int(), corners, seg, centre, cell, eps, clamp)
    assert pos.dtype == torch.float32 and pos.shape == (C, 3) and pos.is_cuda
    return pos.cpu().numpy(), cluster.cpu().numpy(), C


def check_positions(verts, faces, cell, eps=1e-3, clamp=0.5):
    """every cluster's position against the reference -> (pos, the reference's clusters)"""
    got, cluster, C = gpu_positions(verts, faces, cell, eps, clamp)
    r_cluster, r_centre, r_C = ref.cluster_vertices(verts, faces, cell)
    assert C == r_C and np.array_equal(cluster, r_cluster)
    want = ref.quadric_positions(verts, faces, r_cluster, r_centre, float(cell), eps, clamp)[0]
    err = np.abs(got.astype(np.float64) - want).max()
    tol = tolerance(verts)
    print('%d faces, %d clusters, cell %g: max |pos - reference| %.3e (tolerance %.3e)' % (len(faces), C, cell, err, tol))
    assert np.isfinite(got).all() and err <= tol
    return got, r_cluster


def check_simplify(verts, faces, cell):
    """mesh.simplify_mesh on the GPU against the reference: positions, faces, kept faces, vertex order -> (Mesh, reference)"""
    from nefii_amd import mesh
    tv, tf = to_gpu(verts, faces)
    want = ref.simplify(verts, faces, cell)
    m = mesh.simplify_mesh(mesh.Mesh(tv, tf, normals=tv.clone(), meta={'resolution': 7}), cell)
    assert m.verts.dtype == torch.float32 and m.faces.dtype == torch.int64 and m.verts.is_cuda and m.faces.is_cuda
    assert all(getattr(m, name) is None for name in mesh.VERTEX_ATTRIBUTES)
    assert np.array_equal(m.faces.cpu().numpy().reshape(-1, 3), want['faces'])
    assert m.verts.shape == want['verts'].shape                          # ascending cluster order, the unused ones left out
    err = np.abs(m.verts.double().cpu().numpy() - want['verts']).max() if len(want['verts']) else 0.0
    assert err <= tolerance(verts), err
    cluster = mesh.cluster_vertices(tv, tf, cell)[0]
    nf, kept = mesh.cluster_faces(tf, cluster)
    assert np.array_equal(kept.cpu().numpy(), want['kept_face'])
    assert np.array_equal(cluster.cpu().numpy(), want['cluster'])
    s = m.meta['simplify']
    assert m.meta['resolution'] == 7
    assert (s['cell'], s['clusters'], s['verts_in'], s['faces_in']) == (float(cell), want['clusters'], len(verts), len(faces))
    assert (s['verts'], s['faces'], s['cancelled_sets']) == (len(want['verts']), len(want['faces']), want['cancelled'])
    assert s['simplify_s'] > 0 and abs(s['cluster_s'] + s['kernel_s'] + s['faces_s'] - s['simplify_s']) < 1e-9
    return m, want


# ---- the kernel against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name,k', ref.CASES)
def test_grid_meshes_match_the_reference(name, k):
    """V is no multiple of the block, and of the cluster counts (541, 260, 117, 438, 193, 87, 128) only the last is a
    multiple of the 32 clusters a block holds: the last block is partly idle in six cases and full in one"""
    v, f, sp = ref.grid_mesh(name)
    check_positions(v, f, k * sp)
    m, want = check_simplify(v, f, k * sp)
    assert (want['clusters'] % 32 != 0) == (name != 'thin') and len(v) % 256 != 0
    d = np.abs(ref.field(name)(m.verts.double().cpu().numpy()))
    print('%s at %g spacings: %d -> %d faces, mean |sdf| %.3e' % (name, k, len(f), m.faces.shape[0], d.mean()))


def test_a_cluster_with_a_single_corner():
    v = np.array([[0.1, 0.1, 0.1], [1.2, 0.2, 0.1], [0.3, 1.4, 0.2], [1.3, 1.2, 1.3]], dtype=np.float32)
    f = np.array([[0, 1, 2]])
    pos, cluster = check_positions(v, f, 0.5)                           # three clusters of one corner each; vertex 3 unused
    assert cluster.tolist() == [0, 2, 1, -1]
    assert np.abs(pos[[0, 2, 1]] - v[:3]).max() <= 1e-6                 # a single corner on its plane: the vertex itself
    m, _ = check_simplify(v, f, 0.5)
    assert m.faces.tolist() == [[0, 2, 1]]
    check_positions(v, np.array([[0, 1, 2], [2, 1, 3]]), 0.5)


def test_a_long_fan_in_one_cell_and_over_two_cells():
    """runs of 15 000 and of 11 338 + 3 662 corners: far longer than the 8 lanes that walk a run"""
    v, f = ref.fan(5000)
    pos, cluster = check_positions(v, f, 2.0)
    assert pos.shape == (1, 3) and (cluster == 0).all()                 # C = 1
    m, want = check_simplify(v, f, 2.0)
    assert m.faces.shape == (0, 3) and m.verts.shape == (0, 3) and want['clusters'] == 1
    v, f = ref.fan(5000, scale=(1.0, 0.3, 1.0))
    pos, cluster = check_positions(v, f, 0.6)
    assert pos.shape == (2, 3) and np.bincount(cluster[f.reshape(-1)]).tolist() == [11338, 3662]
    check_simplify(v, f, 0.6)
    check_positions(v, f, 0.6, eps=0.1, clamp=0.05)                     # other parameters, a clamp that bites


def test_65_tetrahedra_each_in_its_own_cell():
    n = 65
    r = np.random.default_rng(3)
    v = (r.uniform(0.0, 0.8, (n, 4, 3)) + np.array([2.0, 0.0, 0.0]) * np.arange(n)[:, None, None]).reshape(-1, 3)
    v = v.astype(np.float32)
    v[0] = 0.0                                                          # the grid of cells starts here: tetrahedron i in cell 2 i
    f = meshcc_ref.tetrahedra(n)
    pos, cluster = check_positions(v, f, 1.0)
    assert pos.shape == (n, 3) and np.array_equal(cluster, np.repeat(np.arange(n), 4))
    m, _ = check_simplify(v, f, 1.0)
    assert m.faces.shape[0] == 0
    m, want = check_simplify(v, f, 0.05)                                # every vertex alone: the mesh comes back
    assert want['clusters'] == 4 * n and m.faces.shape[0] == 4 * n
    order = np.argsort(want['cluster'])
    assert np.abs(m.verts.cpu().numpy() - v[order]).max() <= tolerance(v)


def test_zero_area_faces_mixed_in():
    v, f, sp = ref.grid_mesh('box')
    V = len(v)
    r = np.random.default_rng(5)
    i = r.integers(0, V, 300)
    copies = v[i[:100]]                                                 # vertices V .. V + 99 repeat the places of others
    v2 = np.concatenate([v, copies], 0)
    extra = np.concatenate([np.stack([i[:100], f[i[:100] % len(f), 1], V + np.arange(100)], 1),      # two corners in one place
                            np.stack([i[100:200], i[100:200], i[200:300]], 1),                       # a repeated index
                            np.stack([i[200:300], i[200:300], i[200:300]], 1)], 0)
    f2 = np.concatenate([f[:2000], extra, f[2000:]], 0)
    pos, _ = check_positions(v2, f2, 3 * sp)
    check_simplify(v2, f2, 3 * sp)
    alone = np.array([[0, 0, 1], [1, 1, 1], [2, 3, 2]])                 # nothing but zero-area faces: the corners' means
    pts = np.array([[0.1, 0.1, 0.1], [0.3, 0.2, 0.1], [1.3, 1.2, 0.1], [1.4, 1.4, 0.3]], dtype=np.float32)
    pos, cluster = check_positions(pts, alone, 1.0)
    assert cluster.tolist() == [0, 0, 1, 1]
    want0 = (2 * pts[0].astype(np.float64) + 4 * pts[1]) / 6
    assert np.abs(pos[0] - want0).max() <= 1e-6


# ---- reproducibility ---------------------------------------------------------------------------------------------------
def canonical(faces):
    """every face rotated to start with its least index, the rows sorted"""
    f = np.asarray(faces).reshape(-1, 3)
    k = f.argmin(1)
    g = np.stack([f[np.arange(len(f)), (k + j) % 3] for j in range(3)], 1)
    return g[np.lexsort(g.T[::-1])]


@pytest.mark.parametrize('name,k', [('box', 3.0), ('thin', 4.0)])
def test_reproducible_for_any_order_of_faces_and_vertices(name, k):
    from nefii_amd import mesh
    v, f, sp = ref.grid_mesh(name)
    cell = k * sp
    tol = tolerance(v)
    tv, tf = to_gpu(v, f)
    a = mesh.simplify_mesh(mesh.Mesh(tv, tf), cell)
    b = mesh.simplify_mesh(mesh.Mesh(tv, tf), cell)
    assert torch.equal(a.verts, b.verts) and torch.equal(a.faces, b.faces)              # two calls: the same bits
    p0 = gpu_positions(v, f, cell)[0]
    assert np.array_equal(p0, gpu_positions(v, f, cell)[0])
    r = np.random.default_rng(1)
    shuffled = f[r.permutation(len(f))]
    c = mesh.simplify_mesh(mesh.Mesh(*to_gpu(v, shuffled)), cell)
    assert np.array_equal(canonical(c.faces.cpu().numpy()), canonical(a.faces.cpu().numpy()))   # the same face set
    assert (c.verts - a.verts).abs().max().item() <= tol
    perm = r.permutation(len(v))                                                        # old vertex number -> new
    v2 = np.empty_like(v)
    v2[perm] = v
    d = mesh.simplify_mesh(mesh.Mesh(*to_gpu(v2, perm[f])), cell)
    # clusters are numbered by their cells and the corners keep their order: the kernel adds the same numbers in the same
    # order, so renumbering the vertices leaves every bit where it was
    assert torch.equal(d.faces, a.faces) and torch.equal(d.verts, a.verts)
    assert np.array_equal(gpu_positions(v2, perm[f], cell)[0], p0)


# ---- bad input ---------------------------------------------------------------------------------------------------------
def test_bad_indices_and_clusters_are_refused_and_never_followed():
    from nefii_amd import mesh, ops
    v, f, sp = ref.grid_mesh('sphere')
    cell = 3 * sp
    tv, tf = to_gpu(v, f)
    cluster, centre, C = mesh.cluster_vertices(tv, tf, cell)
    corners, seg = mesh.corner_runs(tf, cluster, C)
    f32, c32 = tf.int(), cluster.int()
    good = ops.mesh_cluster_quadrics(tv, f32, c32, corners, seg, centre, cell)
    used_vertex = int(f[1234, 0])
    for bad_index in (-1, len(v), 2 ** 31 - 1, -2 ** 31):
        bad = f32.clone()
        bad[777, 2] = bad_index
        with pytest.raises(ValueError, match='index'):
            ops.mesh_cluster_quadrics(tv, bad, c32, corners, seg, centre, cell)
        assert torch.equal(ops.mesh_cluster_quadrics(tv, f32, c32, corners, seg, centre, cell), good)   # still right
    for bad_cluster in (-1, C, 2 ** 31 - 1):
        bad = c32.clone()
        bad[used_vertex] = bad_cluster
        with pytest.raises(ValueError, match='cluster'):
            ops.mesh_cluster_quadrics(tv, f32, bad, corners, seg, centre, cell)
        assert torch.equal(ops.mesh_cluster_quadrics(tv, f32, c32, corners, seg, centre, cell), good)
    bad = c32.clone()
    bad[used_vertex] = (int(c32[used_vertex]) + 1) % C                   # in range, but not what the corner list was built on
    with pytest.raises(ValueError, match='cluster'):
        ops.mesh_cluster_quadrics(tv, f32, bad, corners, seg, centre, cell)
    bad = corners.clone()
    bad[5] = 3 * len(f)
    with pytest.raises(ValueError, match='index'):
        ops.mesh_cluster_quadrics(tv, f32, c32, bad, seg, centre, cell)
    bad = seg.clone()
    bad[-1] = 3 * len(f) + 1
    with pytest.raises(ValueError, match='cluster'):
        ops.mesh_cluster_quadrics(tv, f32, c32, corners, bad, centre, cell)
    assert torch.equal(ops.mesh_cluster_quadrics(tv, f32, c32, corners, seg, centre, cell), good)
    with pytest.raises(ValueError):
        ops.mesh_cluster_quadrics(tv, tf, c32, corners, seg, centre, cell)              # the op takes int32
    with pytest.raises(ValueError):
        ops.mesh_cluster_quadrics(tv, f32, c32, corners, seg[:-1], centre, cell)
    with pytest.raises(ValueError):
        ops.mesh_cluster_quadrics(tv, f32, c32, corners, seg, centre, 0.0)
    bad = tf.clone()
    bad[10, 1] = len(v)
    with pytest.raises(ValueError, match='index'):
        mesh.simplify_mesh(mesh.Mesh(tv, bad), cell)                    # refused on the host, before any gather


# ---- projection --------------------------------------------------------------------------------------------------------
def test_projection_onto_the_analytic_sphere():
    from nefii_amd import mesh
    v, f, sp = ref.grid_mesh('sphere')
    cell = 4.5 * sp
    m = mesh.simplify_mesh(mesh.Mesh(*to_gpu(v, f)), cell)
    centre = torch.tensor(ref.SPHERE[0], dtype=torch.float64, device=DEV)

    def vg(x):
        d = x.double() - centre
        n = d.norm(dim=1)
        return n - ref.SPHERE[1], d / n[:, None]

    before = vg(m.verts)[0].abs()
    out = mesh.project_to_level_set(vg, m.verts, max_move=0.5 * cell)
    after = vg(out)[0].abs()
    moved = (out - m.verts).abs().max().item()
    print('sphere at 4.5 spacings: |sdf| max %.3e -> %.3e, largest move %.3e of %.3e allowed' % (
        before.max().item(), after.max().item(), moved, 0.5 * cell))
    assert out.dtype == torch.float32 and out.shape == m.verts.shape
    assert after.max().item() <= 1e-6
    assert moved <= 0.5 * cell
    want = ref.project(lambda x: tuple(t.cpu().numpy() for t in vg(torch.from_numpy(x).to(DEV))),
                       m.verts.double().cpu().numpy(), max_move=0.5 * cell)
    assert np.abs(out.cpu().numpy() - want).max() <= tolerance(v)


# ---- the fitted bowl ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def bowl():
    from test_gpu_mesh import scene_model
    return scene_model('bowl_trained', 'conf')[0]


def test_simplified_export_of_the_fitted_bowl(bowl):
    import scenes
    from nefii_amd.mesh import extract_mesh
    res = 96
    plain = extract_mesh(bowl, resolution=res)
    off = extract_mesh(bowl, resolution=res, simplify=0)
    for name in ('verts', 'faces', 'normals', 'diffuse_albedo', 'roughness', 'specular_reflection'):
        assert torch.equal(getattr(plain, name), getattr(off, name)), name             # simplify=0: the same bits
    assert sorted(off.meta) == sorted(plain.meta) and 'simplify' not in off.meta
    raw = extract_mesh(bowl, resolution=res, simplify=3, project=False)
    m = extract_mesh(bowl, resolution=res, simplify=3)
    V, F = m.verts.shape[0], m.faces.shape[0]
    assert 0 < F < plain.faces.shape[0] / 4
    assert torch.equal(m.faces, raw.faces) and m.verts.shape == raw.verts.shape
    s = m.meta['simplify']
    assert sorted(set(m.meta) - set(plain.meta)) == ['simplify']
    assert (s['verts_in'], s['faces_in'], s['verts'], s['faces']) == (plain.verts.shape[0], plain.faces.shape[0], V, F)
    assert s['cell'] == 3 * m.meta['spacing'] and s['clusters'] >= V and s['cancelled_sets'] >= 0 and s['simplify_s'] > 0
    assert s['project'] is True and raw.meta['simplify']['project'] is False
    assert int(m.faces.min()) == 0 and int(m.faces.max()) == V - 1
    assert m.verts.dtype == torch.float32 and m.faces.dtype == torch.int64
    assert m.normals.shape == (V, 3) and m.diffuse_albedo.shape == (V, 3) and m.roughness.shape == (V, 1)
    assert m.specular_reflection.shape == (V, 3)
    assert torch.allclose(m.normals.norm(dim=1), torch.ones(V, device=DEV), atol=1e-5)
    assert (m.verts - raw.verts).abs().max().item() <= 0.5 * s['cell'] + 1e-6
    net = bowl.implicit_network
    with torch.no_grad():
        sdf = [net.value_feature_gradient(x.verts)[0].abs().mean().item() for x in (plain, raw, m)]
    true = [scenes.SCENES['bowl'](x.verts.double().cpu()).abs().mean().item() for x in (plain, raw, m)]
    print('bowl at %d: %d -> %d faces, %d -> %d vertices (%d clusters, %d sets cancelled)' % (
        res, s['faces_in'], F, s['verts_in'], V, s['clusters'], s['cancelled_sets']))
    print('mean |network sdf|: marching cubes %.3e, simplified %.3e, simplified and projected %.3e' % tuple(sdf))
    print('mean distance to the scene: marching cubes %.3e, simplified %.3e, simplified and projected %.3e' % tuple(true))
    assert sdf[2] < sdf[1]
    none = extract_mesh(bowl, resolution=24, simplify=1000)              # the whole surface in one cell: no face is left
    assert none.verts.shape == (0, 3) and none.faces.shape == (0, 3) and none.normals is None
    assert none.meta['simplify']['faces_in'] > 0 and none.meta['simplify']['faces'] == 0
    assert none.meta['simplify']['clusters'] == 1


# ---- the command line --------------------------------------------------------------------------------------------------
def synthetic_checkpoint(tmp_path):
    """the conf and the Step-1 checkpoint of the fitted bowl, as test_cli_high_res_keep_largest builds them -> the command"""
    from test_gpu_mesh import _hocon
    from nefii_amd import synthetic as syn
    mc = syn.model_conf('conf')
    sd = syn.make_state_dict(mc, seed=0, scene='bowl_trained')
    conf_path = tmp_path / 'run.conf'
    conf_path.write_text('train {\n model_class = model.implicit_differentiable_renderer.IDRNetwork\n}\nmodel { %s }\n'
                         % _hocon(mc))
    geo = tmp_path / 'step1.pth'
    torch.save({'epoch': 3, 'model_state_dict': {k: v for k, v in sd.items() if k.startswith('implicit_network')}},
               str(geo))
    return [sys.executable, '-m', 'nefii_amd.scripts.extract_mesh', '--conf', str(conf_path), '--geometry', str(geo)]


def test_cli_simplify_that_leaves_no_face_says_so(tmp_path):
    out = tmp_path / 'none.ply'
    r = subprocess.run(synthetic_checkpoint(tmp_path) + ['--resolution', '24', '--simplify', '1000', '--out', str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and '--simplify' in r.stderr and 'no surface' not in r.stderr, r.stdout + r.stderr
    assert not out.exists()


def test_cli_simplify_keep_largest(tmp_path):
    from nefii_amd.utils.ply import read_ply
    base = synthetic_checkpoint(tmp_path) + ['--resolution', '64', '--keep', 'largest']
    full, small = tmp_path / 'full.ply', tmp_path / 'small.ply'
    r0 = subprocess.run(base + ['--out', str(full)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    assert 'simplified' not in r0.stdout
    r = subprocess.run(base + ['--out', str(small), '--simplify', '3'], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    p0, p = read_ply(str(full)), read_ply(str(small))
    V0, F0, V, F = len(p0['vertex']['x']), len(p0['faces']), len(p['vertex']['x']), len(p['faces'])
    line = re.search(r'extract_mesh: simplified (\d+) vertices, (\d+) faces -> (\d+), (\d+) \(cell ([0-9.e+-]+), [0-9.]+ s\)',
                     r.stdout)
    assert line, r.stdout
    assert [int(g) for g in line.groups()[:4]] == [V0, F0, V, F]
    assert abs(float(line.group(5)) / (3 * 2.0 / 63) - 1.0) < 1e-4       # the synthetic model's bounding sphere is 1
    assert 0 < F < F0 / 4 and '%d vertices, %d faces' % (V, F) in r.stdout
    assert list(p['vertex']) == ['x', 'y', 'z', 'nx', 'ny', 'nz']
    assert any(c.startswith('simplify 3.0 cell ') and c.endswith('project yes') for c in p['comments'])
    assert not any(c.startswith('simplify') for c in p0['comments'])
    assert ref.unbalanced_edges(p['faces']) == 0
