"""Connected components on the GPU (csrc/nefii_meshcc.hip) against the union-find of tests/meshcc_ref.py - every label
comparison is exact -, the selection built on them, and the aligned high-resolution export: on analytic fields, on the
fitted bowl, and through the command line.  Budget: a few seconds per test (check with --durations)."""
import math
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
import mc_ref  # noqa: E402
import meshcc_ref as ref  # noqa: E402

DEV = torch.device('cuda:0')


def gpu_labels(faces, n_verts):
    from nefii_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))).to(DEV).int()
    label, rounds = ops.mesh_components(t, n_verts)
    assert label.dtype == torch.int32 and label.shape == (n_verts,) and label.is_cuda
    return label.cpu().numpy().astype(np.int64), rounds


def check_labels(faces, n_verts, seed=0):
    """the GPU labels against the oracle (exactly), the invariants, and the three kinds of reproducibility -> rounds"""
    from nefii_amd import ops
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    got, rounds = gpu_labels(faces, n_verts)
    want = ref.labels(faces, n_verts)
    assert np.array_equal(got, want), 'first difference at vertex %d' % np.nonzero(got != want)[0][0]
    assert (got <= np.arange(n_verts)).all() and np.array_equal(got[got], got)
    assert 0 <= rounds <= ops.mesh_cc_round_cap(n_verts)
    assert np.array_equal(gpu_labels(faces, n_verts)[0], got)                          # two calls: the same bits
    r = np.random.default_rng(seed)
    assert np.array_equal(gpu_labels(faces[r.permutation(len(faces))], n_verts)[0], got)   # any order of the faces
    perm = r.permutation(n_verts)                                                      # old vertex number -> new
    relabelled, _ = gpu_labels(perm[faces], n_verts)
    assert ref.same_partition(relabelled[perm], got)                                   # the same sets under new numbers
    return rounds


def test_small_cases():
    from nefii_amd import ops
    assert check_labels([[0, 1, 2]], 3) >= 1
    got, rounds = gpu_labels(np.zeros((0, 3)), 5)                       # no faces: every vertex alone, no round
    assert got.tolist() == [0, 1, 2, 3, 4] and rounds == 0
    label, rounds = ops.mesh_components(torch.zeros(0, 3, dtype=torch.int32, device=DEV), 0)
    assert label.shape == (0,) and rounds == 0
    check_labels([[5, 2, 7], [7, 8, 2]], 11)                            # vertices that no face uses
    assert gpu_labels([[5, 2, 7], [7, 8, 2]], 11)[0].tolist() == [0, 1, 2, 3, 4, 2, 6, 2, 2, 9, 10]
    check_labels(ref.tetrahedra(2), 8)
    check_labels(ref.tetrahedra(65), 260)                               # more components than a wave has lanes
    assert len(np.unique(gpu_labels(ref.tetrahedra(65), 260)[0])) == 65
    # duplicates, and faces with repeated indices
    check_labels([[0, 0, 1], [2, 2, 2], [3, 4, 3], [1, 3, 5], [1, 3, 5], [5, 3, 1], [6, 7, 8], [6, 7, 8]], 10)


@pytest.mark.parametrize('seed', [None, 1])
def test_long_chain(seed):
    """one component that spans many workgroups through a chain of 4097 triangles; emulated synchronously, the ordered strip
    took 2 rounds and the permuted one 9 to 11; an MI355X took 2 and 8: far inside the cap of 60"""
    from nefii_amd import ops
    faces, n_verts = ref.strip(4097, seed)
    rounds = check_labels(faces, n_verts)
    print('strip of 4097 triangles, seed %r: %d rounds' % (seed, rounds))
    assert ops.mesh_cc_round_cap(n_verts) == 4 * 13 + 8 and 1 <= rounds <= 60


@pytest.fixture(scope='module')
def random_volume():
    return torch.from_numpy(np.random.default_rng(0).random((32, 32, 32), dtype=np.float32)).to(DEV)


@pytest.mark.parametrize('level,min_components', [(0.5, 100), (0.2, 1000)])
def test_many_components_of_a_random_volume(random_volume, level, min_components):
    from nefii_amd import mesh
    verts, faces = mesh.marching_cubes(random_volume, level)
    V = verts.shape[0]
    rounds = check_labels(faces.cpu().numpy(), V)
    labels = mesh.connected_components(faces, V)                        # int64 faces, as marching_cubes returns them
    assert labels.dtype == torch.int64 and np.array_equal(labels.cpu().numpy(), ref.labels(faces.cpu().numpy(), V))
    n = len(torch.unique(labels))
    print('level %g: %d vertices, %d faces, %d components, %d rounds' % (level, V, faces.shape[0], n, rounds))
    assert V > 20000 and n > min_components
    ids, n_v, n_f, area = mesh.component_table(verts, faces, labels)
    assert len(ids) == n and int(n_v.sum()) == V and int(n_f.sum()) == faces.shape[0]
    assert abs(area.sum().item() - mc_ref.area_volume(verts.cpu().numpy(), faces.cpu().numpy())[0]) < 1e-9 * area.sum().item()
    again = mesh.component_table(verts, faces, labels)
    assert torch.equal(area, again[3])                                  # no float atomics: the same bits


def test_an_index_out_of_range_is_refused_and_never_followed():
    from nefii_amd import mesh, ops
    faces, n_verts = ref.strip(700)
    good = torch.from_numpy(faces).to(DEV).int()
    for bad_index in (-1, n_verts, 2 ** 31 - 1, -2 ** 31):
        bad = good.clone()
        bad[333, 1] = bad_index
        with pytest.raises(ValueError):
            ops.mesh_components(bad, n_verts)
        label, _ = ops.mesh_components(good, n_verts)                   # the next call on good input is still right
        assert not label.any()
    bad = good.long()
    bad[5, 2] = 2 ** 32 + 1                                             # would wrap to a legal index in int32
    with pytest.raises(ValueError):
        mesh.connected_components(bad, n_verts)
    with pytest.raises(ValueError):
        ops.mesh_components(good.long(), n_verts)                       # the op takes int32
    with pytest.raises(ValueError):
        ops.mesh_components(good[:, :2].contiguous(), n_verts)
    with pytest.raises(ValueError):
        ops.mesh_components(good, -1)


def test_three_spheres_table_and_selection():
    from nefii_amd import mesh
    n = 48
    p = ref.grid_points(n)
    fields = [torch.from_numpy(ref.sphere_sdf(p, c, r).astype(np.float32)).to(DEV) for c, r in ref.SPHERES]
    sp = 2.0 / (n - 1)
    kw = dict(spacing=(sp, sp, sp), origin=(-1.0, -1.0, -1.0))
    verts, faces = mesh.marching_cubes(torch.minimum(torch.minimum(fields[0], fields[1]), fields[2]), 0.0, **kw)
    labels = mesh.connected_components(faces, verts.shape[0])
    ids, n_v, n_f, area = mesh.component_table(verts, faces, labels)
    assert len(ids) == 3
    got = sorted(area.tolist(), reverse=True)
    for a, (_, r), tol in zip(got, ref.SPHERES, (0.02, 0.02, 0.08)):
        exact = 4.0 * math.pi * r * r
        print('sphere of radius %g: area %.5f, exact %.5f, off by %.2f %%' % (r, a, exact, 100 * abs(a / exact - 1)))
        assert abs(a / exact - 1.0) <= tol
    m = mesh.Mesh(verts, faces)
    big = mesh.select_components(m, 'largest')
    v0, f0 = mesh.marching_cubes(fields[0], 0.0, **kw)                  # the first sphere alone
    assert torch.equal(big.verts, v0) and torch.equal(big.faces, f0)
    assert big.meta['components']['count'] == 3 and big.meta['cc_rounds'] >= 1 and big.meta['cc_s'] > 0
    assert big.meta['components']['area'] == got
    two = mesh.select_components(m, 0.3)                                # (0.3 / 0.45)^2 = 0.44, (0.1 / 0.45)^2 = 0.05
    assert len(torch.unique(mesh.connected_components(two.faces, two.verts.shape[0]))) == 2
    assert mc_ref.is_closed_oriented(two.faces.cpu().numpy())
    assert mesh.select_components(m, 'all') is m


def torch_box_scene_sdf(x):
    x = x.double()
    rot = torch.as_tensor(ref.BOX_ROT, device=x.device)
    q = ((x - torch.as_tensor(ref.BOX_CENTRE, device=x.device)) @ rot).abs() - torch.as_tensor(ref.BOX_HALF, device=x.device)
    box = q.clamp_min(0).norm(dim=1) + q.max(1)[0].clamp_max(0)
    ball = (x - torch.as_tensor(ref.FLOATER[0], device=x.device, dtype=torch.float64)).norm(dim=1) - ref.FLOATER[1]
    return torch.minimum(box, ball)


def test_analytic_high_resolution_path():
    """the steps of extract_mesh(high_res=True) with a torch field in the network's place"""
    from nefii_amd import mesh
    n = 64
    ax = torch.linspace(-1, 1, n, device=DEV, dtype=torch.float64)
    pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)
    sp = 2.0 / (n - 1)
    lv, lf = mesh.marching_cubes(torch_box_scene_sdf(pts).float().view(n, n, n), 0.0, spacing=(sp, sp, sp),
                                 origin=(-1.0, -1.0, -1.0))
    low = mesh.select_components(mesh.Mesh(lv, lf), 'largest')
    table = low.meta['components']
    print('low resolution: components', table['n_verts'], 'of', lv.shape[0], 'vertices')
    assert table['count'] == 2 and table['n_verts'][0] > 4000 and table['n_verts'][1] < 300
    assert low.verts.shape[0] == table['n_verts'][0]
    grid = mesh.aligned_grid(low.verts, 96)
    print('aligned grid %s, spacing %.6f' % (grid.shape, grid.spacing))
    assert grid.shape == (96, 132, 190)
    assert abs(grid.spacing / 0.00848 - 1.0) <= 0.01
    c = grid.to_local(torch.tensor([ref.FLOATER[0]], dtype=torch.float64))[0].numpy()
    assert any(c[a] < grid.axes[a][0] or c[a] > grid.axes[a][-1] for a in range(3))      # the floater: outside the grid
    N = grid.numel()
    vol = torch.cat([torch_box_scene_sdf(grid.points(s, min(N, s + 2 ** 20), DEV)).float() for s in range(0, N, 2 ** 20)])
    v, f = mesh.marching_cubes(vol.view(*grid.shape), 0.0, spacing=(grid.spacing,) * 3, origin=grid.origin)
    verts = grid.to_world(v).float()
    assert len(torch.unique(mesh.connected_components(f, verts.shape[0]))) == 1
    fn, vn = f.cpu().numpy(), verts.double().cpu().numpy()
    assert mc_ref.is_closed_oriented(fn)
    area, volume = mc_ref.area_volume(vn, fn)
    d = np.abs(ref.box_sdf(vn))
    print('%d vertices, max |sdf| %.3g (spacing %.3g), area %.5f (box %.5f)' % (len(vn), d.max(), grid.spacing, area,
                                                                                 ref.BOX_AREA))
    assert d.max() <= grid.spacing                 # a 1-Lipschitz field changes sign along an edge of that length
    assert abs(area / ref.BOX_AREA - 1.0) <= 0.01 and volume > 0


@pytest.fixture(scope='module')
def bowl():
    from test_gpu_mesh import scene_model
    return scene_model('bowl_trained', 'conf')[0]


def test_high_res_export_of_the_fitted_bowl(bowl):
    import scenes
    from nefii_amd.mesh import extract_mesh
    m = extract_mesh(bowl, resolution=96, high_res=True, low_resolution=48, margin=0.05, keep='largest')
    V = m.verts.shape[0]
    fn = m.faces.cpu().numpy()
    assert V > 1000 and m.verts.dtype == torch.float32 and m.faces.dtype == torch.int64
    assert mc_ref.is_closed_oriented(fn) and mc_ref.area_volume(m.verts.cpu().numpy(), fn)[1] > 0
    cell = m.meta['spacing']
    d = scenes.SCENES['bowl'](m.verts.double().cpu()).abs()
    print('V %d, grid %s, spacing %.5f (uniform %.5f), |sdf| mean %.2e max %.2e, rounds %d, labelling %.4f s' % (
        V, m.meta['grid_shape'], cell, 2.0 * bowl.object_bounding_sphere / 95, d.mean().item(), d.max().item(),
        m.meta['cc_rounds'], m.meta['cc_s']))
    assert d.mean().item() < 2e-3 and d.max().item() < 2e-2 + 0.5 * cell, (d.mean().item(), d.max().item(), cell)
    assert cell < 2.0 * bowl.object_bounding_sphere / 95
    assert min(m.meta['grid_shape']) == 96 and m.meta['cc_rounds'] >= 2 and m.meta['cc_s'] > 0
    assert m.meta['components']['count'] >= 1 and m.meta['low_res_components']['count'] >= 1
    assert m.normals.shape == (V, 3) and m.diffuse_albedo.shape == (V, 3) and m.roughness.shape == (V, 1)
    assert m.specular_reflection.shape == (V, 3)
    assert torch.allclose(m.normals.norm(dim=1), torch.ones(V, device=DEV), atol=1e-5)
    with pytest.raises(ValueError):
        extract_mesh(bowl, resolution=32, high_res=True, low_resolution=16, level=-5.0)       # no crossing at low resolution


def test_the_defaults_are_the_uniform_export_bit_for_bit(bowl):
    from nefii_amd import mesh
    res = 96
    m = mesh.extract_mesh(bowl, resolution=res)
    net, bound = bowl.implicit_network, float(bowl.object_bounding_sphere)
    with torch.no_grad():
        vol = mesh.sdf_grid(net, res, bound, precision=mesh._tracer_precision(bowl))
        sp = 2.0 * bound / (res - 1)
        verts, faces = mesh.marching_cubes(vol, 0.0, spacing=(sp, sp, sp), origin=(-bound, -bound, -bound))
        _, feat, g = net.value_feature_gradient(verts)
        normals = g / g.norm(dim=1, keepdim=True).clamp_min(1e-12)
        out = bowl.envmap_material_network(verts, feat)
    V = verts.shape[0]
    assert torch.equal(m.verts, verts) and torch.equal(m.faces, faces) and torch.equal(m.normals, normals)
    assert torch.equal(m.diffuse_albedo, out['sg_diffuse_albedo'].float().reshape(V, 3))
    assert torch.equal(m.roughness, out['sg_roughness'].float().expand(V, 1))
    spec = bowl.envmap_material_network.specular_inv_remap(out['sg_specular_reflectance']).float()
    assert torch.equal(m.specular_reflection, spec.expand(V, 3))
    assert sorted(m.meta) == sorted(['resolution', 'level', 'bound', 'grid_s', 'mcubes_s', 'grid_shape', 'spacing',
                                     'cc_rounds', 'cc_s'])
    assert m.meta['grid_shape'] == (res, res, res) and m.meta['spacing'] == sp and m.meta['cc_rounds'] == 0
    assert (m.meta['resolution'], m.meta['level'], m.meta['bound']) == (res, 0.0, bound)


def test_cli_high_res_keep_largest(tmp_path):
    from test_gpu_mesh import _hocon
    from nefii_amd import synthetic as syn
    from nefii_amd.utils.ply import read_ply
    mc = syn.model_conf('conf')
    sd = syn.make_state_dict(mc, seed=0, scene='bowl_trained')
    conf_path = tmp_path / 'run.conf'
    conf_path.write_text('train {\n model_class = model.implicit_differentiable_renderer.IDRNetwork\n}\nmodel { %s }\n'
                         % _hocon(mc))
    geo = tmp_path / 'step1.pth'
    torch.save({'epoch': 3, 'model_state_dict': {k: v for k, v in sd.items() if k.startswith('implicit_network')}},
               str(geo))
    out = tmp_path / 'h.ply'
    r = subprocess.run([sys.executable, '-m', 'nefii_amd.scripts.extract_mesh', '--conf', str(conf_path), '--geometry',
                        str(geo), '--out', str(out), '--resolution', '64', '--high_res', '--low_resolution', '32',
                        '--grid_margin', '0.05', '--keep', 'largest'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ply = read_ply(str(out))
    assert list(ply['vertex']) == ['x', 'y', 'z', 'nx', 'ny', 'nz']
    V, F = len(ply['vertex']['x']), len(ply['faces'])
    assert V > 1000 and F > 2000 and mc_ref.is_closed_oriented(ply['faces'])
    assert '%d vertices, %d faces' % (V, F) in r.stdout
    assert 'low-resolution mesh: ' in r.stdout and ' component' in r.stdout and 'vertices      faces' in r.stdout
    shape = re.search(r'grid (\d+) x (\d+) x (\d+), spacing', r.stdout)
    assert shape and min(int(v) for v in shape.groups()) == 64
    assert any('high_res low_resolution 32' in c and 'keep largest' in c for c in ply['comments'])
    r = subprocess.run([sys.executable, '-m', 'nefii_amd.scripts.extract_mesh', '--conf', str(conf_path), '--geometry',
                        str(geo), '--out', str(out), '--keep', 'most'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and 'keep' in r.stderr
