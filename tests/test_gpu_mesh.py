"""Mesh export on the GPU: csrc/nefii_mcubes.hip against the numpy oracle (tests/mc_ref.py), extract_mesh on the fitted
scene nets against the analytic scenes, the CPU oracle's normals / materials and the tracer, and the command line end to
end.  Budget: about a minute in all (check with --durations)."""
import os
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

DEV = torch.device('cuda:0')


def smooth_field(shape, seed, n_waves=6):
    """a sum of random plane waves: many components, saddles and crossings of every cell type"""
    r = np.random.default_rng(seed)
    axes = [np.linspace(0, 1, n, dtype=np.float32) for n in shape]
    X, Y, Z = np.meshgrid(*axes, indexing='ij')
    v = np.zeros(shape, np.float32)
    for _ in range(n_waves):
        k = r.normal(size=3) * 12
        v += np.sin(k[0] * X + k[1] * Y + k[2] * Z + r.uniform(0, 6.3)).astype(np.float32)
    return v


def gpu_vs_ref(vol, level=0.0, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    from nefii_amd import mesh
    t = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(DEV)
    v, f = mesh.marching_cubes(t, level, spacing=spacing, origin=origin)
    rv, rf = mc_ref.marching_cubes(vol, level, origin, spacing)
    assert f.dtype == torch.int64 and v.dtype == torch.float32
    assert tuple(v.shape) == rv.shape and tuple(f.shape) == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    assert np.array_equal(f.cpu().numpy(), rf)
    assert np.array_equal(v.cpu().numpy(), rv)       # bit for bit: mc_ref restates the fp32 expression of csrc/mc_cell.h
    return v, f


def test_marching_cubes_matches_the_oracle_on_random_volumes():
    r = np.random.default_rng(0)
    for shape in ((2, 2, 2), (2, 3, 2), (3, 5, 7), (17, 33, 9), (24, 24, 24), (5, 70, 61)):
        vol = r.integers(-2, 3, shape).astype(np.float32) * 0.5       # exact ties with the level included
        gpu_vs_ref(vol, 0.0)
        gpu_vs_ref(vol, 0.5, origin=(-1.0, 2.0, 0.25), spacing=(0.5, 0.25, 2.0))
    for mask in (1, 105, 150, 254):                                     # one cell, 2 x 2 x 2
        vol = np.array([[[-1.0 if (mask >> (x | y << 1 | z << 2)) & 1 else 1.0 for z in range(2)] for y in range(2)]
                        for x in range(2)], np.float32)
        v, f = gpu_vs_ref(vol)
        assert f.shape[0] == mc_ref.NTRI[mask]


def test_marching_cubes_large_volume_many_tiles_and_bitwise_reproducible():
    from nefii_amd import mesh
    vol = smooth_field((300, 200, 150), seed=1)                         # 9 M points: 4395 tiles, 5 per scan thread
    v, f = gpu_vs_ref(vol, 0.1, origin=(-1.5, -1.0, -0.75), spacing=(0.01, 0.01, 0.01))
    assert f.shape[0] > 500000
    assert f.min().item() >= 0 and f.max().item() == v.shape[0] - 1
    t = torch.from_numpy(vol).to(DEV)
    v2, f2 = mesh.marching_cubes(t, 0.1, spacing=(0.01, 0.01, 0.01), origin=(-1.5, -1.0, -0.75))
    assert torch.equal(v, v2) and torch.equal(f, f2)


def test_marching_cubes_analytic_shapes_and_edge_cases():
    from nefii_amd import mesh
    n = (70, 64, 57)
    axes = [np.linspace(-1, 1, k, dtype=np.float32) for k in n]
    X, Y, Z = np.meshgrid(*axes, indexing='ij')
    sp = tuple(2.0 / (k - 1) for k in n)
    q = np.sqrt(X * X + Y * Y) - 0.6
    torus = np.sqrt(q * q + Z * Z) - 0.25
    v, f = gpu_vs_ref(torus, 0.0, (-1.0, -1.0, -1.0), sp)
    fn = f.cpu().numpy()
    assert mc_ref.is_closed_oriented(fn) and mc_ref.euler(v.cpu().numpy(), fn) == 0
    assert mc_ref.area_volume(v.cpu().numpy(), fn)[1] > 0
    # no crossing
    v, f = mesh.marching_cubes(torch.ones(9, 8, 7, device=DEV))
    assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == torch.int64
    v, f = mesh.marching_cubes(torch.zeros(2, 2, 2, device=DEV))        # all at the level: all outside
    assert v.shape == (0, 3)
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.ones(4, 4, 4))                        # CPU tensor
    bad = torch.ones(4, 4, 4, device=DEV)
    bad[1, 2, 3] = float('nan')
    with pytest.raises(ValueError):
        mesh.marching_cubes(bad)
    bad[1, 2, 3] = float('inf')
    with pytest.raises(ValueError):
        mesh.marching_cubes(bad)
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.ones(1, device=DEV).expand(1300, 1300, 1300))   # 2.2e9 points
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.ones(4, 1, 4, device=DEV))
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.ones(4, 4, 4, device=DEV), level=float('nan'))


def scene_model(scene, model_name):
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    mc = syn.model_conf(model_name)
    sd = syn.make_state_dict(mc, seed=0, scene=scene)
    model = IDRNetwork(conf.from_dict(mc))
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    model.freeze_geometry()
    model.eval()
    return model, mc, sd


@pytest.mark.parametrize('scene,model_name,res', [('bowl_trained', 'conf', 192), ('frame_trained', 'conf', 128),
                                                  ('bowl_trained', 'neus', 128)])
def test_extract_mesh_on_fitted_scenes(scene, model_name, res):
    import scenes
    from nefii_amd.mesh import extract_mesh
    from oracle import nets
    model, mc, sd = scene_model(scene, model_name)
    m = extract_mesh(model, resolution=res)
    V = m.verts.shape[0]
    assert V > 1000 and m.faces.dtype == torch.int64
    assert mc_ref.is_closed_oriented(m.faces.cpu().numpy())
    assert mc_ref.area_volume(m.verts.cpu().numpy(), m.faces.cpu().numpy())[1] > 0
    cell = 2.0 * model.object_bounding_sphere / (res - 1)
    d = scenes.SCENES[scene.split('_')[0]](m.verts.double().cpu()).abs()
    # the fit's own error (tests/test_geometry_cpu.py: mean 5e-4, max 2e-2) plus marching cubes' at sharp features
    assert d.mean().item() < 2e-3 and d.max().item() < 2e-2 + 0.5 * cell, (d.mean().item(), d.max().item(), cell)
    # normals, albedo and roughness at a sample of the vertices against the CPU oracle
    idx = torch.randperm(V, generator=torch.Generator().manual_seed(0))[:1500]
    x = m.verts[idx].cpu()
    cfg = mc['implicit_network']
    g = nets.sdf_gradient(sd, cfg, x)
    g = g / g.norm(dim=1, keepdim=True)
    err = (m.normals[idx].cpu() - g).norm(dim=1)
    assert err.max().item() < 5e-3 and err.mean().item() < 5e-4, (err.max().item(), err.mean().item())
    assert m.diffuse_albedo.shape == (V, 3) and m.roughness.shape == (V, 1) and m.specular_reflection.shape == (V, 3)
    _, feat, _ = model.implicit_network.value_feature_gradient(m.verts[idx])
    ref = nets.material_forward(sd, mc['envmap_material_network'], x, feat.cpu() if feat is not None else None)
    a_err = (m.diffuse_albedo[idx].cpu() - ref['sg_diffuse_albedo']).abs().max().item()
    r_err = (m.roughness[idx].cpu() - ref['sg_roughness'].expand(len(idx), 1)).abs().max().item()
    assert a_err < 2e-3 and r_err < 2e-3, (a_err, r_err)
    s_ref = model.envmap_material_network.specular_inv_remap(ref['sg_specular_reflectance']).expand(len(idx), 3)
    assert (m.specular_reflection[idx].cpu() - s_ref).abs().max().item() < 1e-4
    # a bare ImplicitNetwork with an explicit bound gives the same surface, without materials
    m2 = extract_mesh(model.implicit_network, resolution=res, bound=model.object_bounding_sphere)
    assert torch.equal(m2.verts, m.verts) and torch.equal(m2.faces, m.faces) and m2.diffuse_albedo is None


def test_tracer_hits_lie_on_the_extracted_mesh():
    from nefii_amd import synthetic as syn
    from nefii_amd.datasets.sdf_dataset import MeshSDF
    from nefii_amd.mesh import extract_mesh
    model, _, _ = scene_model('bowl_trained', 'conf')
    res = 160
    m = extract_mesh(model, resolution=res, materials=False)
    cell = 2.0 * model.object_bounding_sphere / (res - 1)
    hits = []
    for k, cam in enumerate(((0.0, 0.3, 2.4), (1.7, -0.9, 1.2))):
        inp, _ = syn.make_inputs(4096, (200, 200), 280.0, cam, -1, seed=3 + k)
        with torch.no_grad():
            out = model.trace_points({kk: v.to(DEV) for kk, v in inp.items()})
        hits.append(out['points'][out['network_object_mask']])
    hits = torch.cat(hits)
    assert hits.shape[0] > 1000
    d = MeshSDF(m.verts, m.faces, device=DEV)(hits).abs()
    assert (d < 0.5 * cell).float().mean().item() > 0.99 and d.max().item() < 1.5 * cell, (d.max().item(), cell)


def _hocon(d):
    out = []
    for k, v in d.items():
        if isinstance(v, dict):
            out.append('%s { %s }' % (k, _hocon(v)))
        elif isinstance(v, (list, tuple)):
            out.append('%s = [%s]' % (k, ', '.join(str(x) for x in v)))
        elif isinstance(v, bool):
            out.append('%s = %s' % (k, 'True' if v else 'False'))
        else:
            out.append('%s = %s' % (k, v))
    return '\n'.join(out)


def test_cli_end_to_end(tmp_path):
    import scenes
    from nefii_amd import mesh, synthetic as syn
    from nefii_amd.utils.ply import read_ply
    mc = syn.model_conf('conf')
    sd = syn.make_state_dict(mc, seed=0, scene='bowl_trained')
    conf_path = tmp_path / 'run.conf'
    conf_path.write_text('train {\n model_class = model.implicit_differentiable_renderer.IDRNetwork\n}\nmodel { %s }\n'
                         % _hocon(mc))
    ck = tmp_path / 'exps' / 'bowl' / '2026_01_01_00_00_00' / 'checkpoints' / 'ModelParameters'
    ck.mkdir(parents=True)
    torch.save({'epoch': 7, 'model_state_dict': sd}, str(ck / 'latest.pth'))
    geo = tmp_path / 'step1.pth'
    torch.save({'epoch': 3, 'model_state_dict': {k: v for k, v in sd.items() if k.startswith('implicit_network')}},
               str(geo))
    # the analytic bowl as an .obj, meshed finely on the GPU
    n = 256
    ax = torch.linspace(-1, 1, n, device=DEV, dtype=torch.float64)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing='ij')
    vol = scenes.bowl(torch.stack([X, Y, Z], -1).reshape(-1, 3)).reshape(n, n, n).float()
    sp = 2.0 / (n - 1)
    bv, bf = mesh.marching_cubes(vol, 0.0, spacing=(sp, sp, sp), origin=(-1.0, -1.0, -1.0))
    obj = tmp_path / 'bowl.obj'
    with open(obj, 'w') as f:
        f.write(''.join('v %.7f %.7f %.7f\n' % tuple(p) for p in bv.cpu().tolist()))
        f.write(''.join('f %d %d %d\n' % tuple(t) for t in (bf + 1).cpu().tolist()))

    base = [sys.executable, '-m', 'nefii_amd.scripts.extract_mesh', '--conf', str(conf_path), '--resolution', '96']
    r = subprocess.run(base + ['--expname', 'bowl', '--exps_folder_name', str(tmp_path / 'exps')], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = tmp_path / 'exps' / 'bowl' / '2026_01_01_00_00_00' / 'plots' / 'surface_7.ply'
    ply = read_ply(str(out))
    assert list(ply['vertex']) == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue', 'albedo_r', 'albedo_g',
                                   'albedo_b', 'roughness', 'specular_r', 'specular_g', 'specular_b']
    V, F = len(ply['vertex']['x']), len(ply['faces'])
    assert V > 1000 and F > 2000 and mc_ref.is_closed_oriented(ply['faces'])
    assert any('resolution 96' in c for c in ply['comments']) and any('latest.pth' in c for c in ply['comments'])
    nrm = np.stack([ply['vertex'][k] for k in ('nx', 'ny', 'nz')], 1)
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-5)
    assert '%d vertices, %d faces' % (V, F) in r.stdout

    r = subprocess.run(base + ['--geometry', str(geo), '--out', str(tmp_path / 's.ply'), '--compare_mesh', str(obj),
                               '--no_scale_to_unit', '--compare_samples', '4000'], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    import json
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    cell = 2.0 / 95
    # Chamfer: below 1e-3 (measured 3e-4); Hausdorff: within 2.5 cells, where the grid cuts the bowl's sharp rim
    assert rec['chamfer'] < 1e-3 and rec['hausdorff'] < 2.5 * cell, (rec, cell)
    assert rec['accuracy_mean'] < 1e-3 and rec['completeness_mean'] < 1e-3
    assert list(read_ply(str(tmp_path / 's.ply'))['vertex']) == ['x', 'y', 'z', 'nx', 'ny', 'nz']
    # a level outside the field's range: no surface, exit status 1
    r = subprocess.run(base + ['--geometry', str(geo), '--out', str(tmp_path / 'n.ply'), '--level', '-5'], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and 'no surface' in r.stderr, r.stdout + r.stderr
