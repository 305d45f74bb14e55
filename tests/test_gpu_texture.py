"""The texture bake on the GPU (csrc/nefii_texbake.hip, nefii_amd/texture.py) against the fp64 numpy restatement
of tests/texbake_ref.py: the raster exactly (owner, covered) and to the final fp32 rounding (barycentrics, positions), the
8-bit levels exactly, the sampler to one fp32 ulp; then a whole bake of the fitted bowl against the CPU oracle of the networks,
what textures gain over per-vertex attributes, and the command line.  Budget: a few seconds per test."""
import json
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
import texbake_ref as ref  # noqa: E402

DEV = torch.device('cuda:0')


def tolerance(values):
    """one fp32 ulp at the scale of the values (the rule of test_gpu_mesh_simplify.py): the one fp32 step is the final
    rounding, half an ulp; the fp64 sums are the reference's own expressions"""
    return 2.0 ** -23 * max(1.0, float(np.abs(np.asarray(values)).max()))


def random_mesh(F, seed):
    rng = np.random.default_rng(seed)
    V = F + 5
    verts = (rng.random((V, 3)) * 1.8 - 0.9).astype(np.float32)
    faces = rng.integers(0, V, size=(F, 3)).astype(np.int32)
    return verts, faces


def gpu_raster(a, verts, faces, chunk=None):
    from nefii_amd import ops
    tv, tf = torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV)
    n_texels = a['T'] ** 2
    parts = [ops.bake_raster(tv, tf, a['T'], a['n'], a['c'], a['p'], first, min(chunk or n_texels, n_texels - first))
             for first in range(0, n_texels, chunk or n_texels)]
    owner, covered, bary, pos = (torch.cat([p[k] for p in parts]) for k in range(4))
    assert (owner.dtype, covered.dtype, bary.dtype, pos.dtype) == (torch.int32, torch.uint8, torch.float32, torch.float32)
    assert owner.shape == (n_texels,) and covered.shape == (n_texels,) and bary.shape == (n_texels, 2) and pos.shape == (n_texels, 3)
    return owner, covered, bary, pos


# ---- the raster against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,T', ref.CASES)
def test_raster_matches_the_reference(F, T):
    """(1, 7): leg 1, the upper half of the cell nobody's; (3, 14): cells 2 and 3 empty; (37, 61): 3721 texels, no multiple of
    the block of 256, a margin of one texel; (200, 160): 100 full cells"""
    a = ref.atlas(F, T)
    verts, faces = random_mesh(F, seed=F)
    owner, covered, bary, pos = (t.cpu().numpy() for t in gpu_raster(a, verts, faces))
    w_owner, w_covered, w_bary, w_pos = ref.raster(a, verts, faces)
    assert np.array_equal(owner.reshape(T, T), w_owner)
    assert np.array_equal(covered.reshape(T, T) != 0, w_covered) and set(np.unique(covered)) <= {0, 1}
    b_err = np.abs(bary.reshape(T, T, 2).astype(np.float64) - w_bary).max()
    err = np.abs(pos.reshape(T, T, 3).astype(np.float64) - w_pos)
    inside = err[w_covered].max() if w_covered.any() else 0.0
    print('%d faces in %d^2: %d owned, %d covered texels; max |bary - reference| %.3e, max |pos - reference| %.3e inside the '
          'charts (tolerance %.3e), %.3e with the gutters (largest |pos| %.3g)' % (
              F, T, (w_owner >= 0).sum(), w_covered.sum(), b_err, inside, tolerance(verts), err.max(), np.abs(w_pos).max()))
    assert b_err <= 1e-6
    # inside a chart the point is a convex combination: one fp32 ulp at the coordinate scale; a gutter texel extrapolates beyond
    # the vertices (by up to (c + p) / s legs), so there the ulp is that of the point itself - per element, the stricter reading
    assert inside <= tolerance(verts)
    assert (err <= 2.0 ** -23 * np.maximum(1.0, np.abs(w_pos))).all()
    unowned = w_owner < 0
    assert not pos.reshape(T, T, 3)[unowned].any() and not bary.reshape(T, T, 2)[unowned].any() and w_covered.sum() > 0
    if (F, T) == (1, 7):
        assert a['s'] == 1 and unowned.sum() == 28
    if (F, T) == (37, 61):
        assert (T * T) % 256 != 0 and a['n'] * a['c'] == T - 1


def test_raster_in_chunks_that_start_mid_row_is_bitwise_the_same():
    a = ref.atlas(37, 61)
    verts, faces = random_mesh(37, seed=37)
    whole = gpu_raster(a, verts, faces)
    parts = gpu_raster(a, verts, faces, chunk=1000)               # 1000, 2000, 3000: none a multiple of 61
    again = gpu_raster(a, verts, faces)
    for w, p, g in zip(whole, parts, again):
        assert torch.equal(w, p) and torch.equal(w, g)


def test_raster_refuses_a_face_index_outside_the_vertices_and_returns():
    from nefii_amd import ops
    a = ref.atlas(37, 61)
    verts, faces = random_mesh(37, seed=1)
    for bad in (len(verts), -1, 2 ** 31 - 1):
        f = faces.copy()
        f[20, 1] = bad
        with pytest.raises(ValueError, match='outside'):
            gpu_raster(a, verts, f)
    v = verts.copy()
    v[faces[3, 0], 2] = np.inf
    with pytest.raises(ValueError, match='finite'):
        gpu_raster(a, v, faces)
    with pytest.raises(ValueError):
        ops.bake_raster(torch.from_numpy(verts).to(DEV), torch.from_numpy(faces).to(DEV), 61, 4, 15, 2)     # 37 faces, 16 cells
    owner = gpu_raster(a, verts, faces)[0]                         # the next call is served as ever
    assert np.array_equal(owner.cpu().numpy().reshape(61, 61), ref.owner_image(a))


# ---- the 8-bit levels -------------------------------------------------------------------------------------------------------
def test_encode_levels_equal_the_reference():
    from nefii_amd import ops
    rng = np.random.default_rng(11)
    N = 5000
    albedo = rng.normal(0.4, 0.5, size=(N, 3)).astype(np.float32)
    albedo[:8] = [[0.0, 1.0, 2.0], [-0.0, 0.5, 1e-30], [1e30, -1e30, 0.999999], [0.2, 0.2, 0.2]] * 2
    roughness = rng.uniform(-0.2, 1.2, size=N).astype(np.float32)
    normal = rng.normal(size=(N, 3))
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    owner = rng.integers(-1, 40, size=N).astype(np.int32)
    owner[rng.random(N) < 0.2] = -1
    assert (albedo < 0).sum() > 500 and (albedo > 1).sum() > 500 and 500 < (owner < 0).sum() < 2000
    w_a, w_n, w_r, before = ref.encode(albedo, roughness, normal, owner)
    near = [np.abs(v - np.round(v)) < 1e-9 for v in before]
    assert not any(m.any() for m in near), 'the seed puts a reference value on a rounding boundary: choose another'
    got = ops.bake_encode(*(torch.from_numpy(t).to(DEV) for t in (albedo, roughness, normal, owner)))
    g_a, g_n, g_r = (t.cpu().numpy() for t in got)
    assert g_a.dtype == np.uint8 and g_a.shape == (N, 4) and g_n.shape == (N, 4) and g_r.shape == (N,)
    wrong = (g_a != w_a).any(1) | (g_n != w_n).any(1) | (g_r != w_r)
    print('%d texels, %d owned: %d differ from the reference (none may: no reference value lies within 1e-9 of a boundary)'
          % (N, (owner >= 0).sum(), wrong.sum()))
    assert wrong.sum() <= N // 10000 and not wrong.any()
    assert (g_a[owner < 0] == 0).all() and (g_n[owner < 0] == 0).all() and (g_r[owner < 0] == 0).all()
    assert (g_a[owner >= 0, 3] == 255).all() and (g_n[owner >= 0, 3] == 255).all()
    assert ops.bake_encode(*(torch.from_numpy(t[:0]).to(DEV) for t in (albedo, roughness, normal, owner)))[2].shape == (0,)


# ---- the sampler -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 3, 4])
def test_sampler_matches_the_reference(C):
    from nefii_amd import ops
    a = ref.atlas(37, 61)
    rng = np.random.default_rng(C)
    face, bary = ref.chart_points(a, rng, 102)                     # corners, edge midpoints, edge and interior points
    face, bary = face[:4097], bary[:4097]
    assert len(face) == 4097 and face.max() == 36
    tex = rng.normal(size=(61, 61, C)).astype(np.float32)
    want = ref.sample(a, tex, face, bary)
    tt = torch.from_numpy(tex).to(DEV)
    got = ops.texture_sample(tt, torch.from_numpy(face.astype(np.int32)).to(DEV), torch.from_numpy(bary).to(DEV), a['n'], a['c'],
                             a['p'])
    assert got.dtype == torch.float32 and got.shape == (4097, C)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print('C = %d: max |lookup - reference| %.3e (tolerance %.3e)' % (C, err, tolerance(tex)))
    assert err <= tolerance(tex)
    # a corner that sits on a texel centre reads that texel alone: corner 0 of face 0 is (2, 2), between four texels; the
    # point half a texel further along both legs is the centre of texel (2, 2)
    b = np.array([[1 - 1.0 / a['s'], 0.5 / a['s'], 0.5 / a['s']]])
    one = ops.texture_sample(tt, torch.zeros(1, dtype=torch.int32, device=DEV), torch.from_numpy(b).to(DEV), a['n'], a['c'], a['p'])
    assert np.abs(one.cpu().numpy()[0] - tex[2, 2]).max() <= tolerance(tex)
    # faces without a cell give zeros; barycentrics far outside the chart are clamped to the image, not followed
    odd = torch.tensor([-1, 2 * a['n'] ** 2, 5, 6], dtype=torch.int32, device=DEV)
    far = torch.tensor([[1., 0, 0], [1., 0, 0], [1e30, -1e30, 1.0], [-1e30, 1e30, 1.0]], dtype=torch.float64, device=DEV)
    out = ops.texture_sample(tt, odd, far, a['n'], a['c'], a['p']).cpu().numpy()
    assert not out[:2].any() and out.shape == (4, C)
    assert ops.texture_sample(tt, odd[:0], far[:0], a['n'], a['c'], a['p']).shape == (0, C)


# ---- a whole bake of the fitted bowl -----------------------------------------------------------------------------------------
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


@pytest.fixture(scope='module')
def bowl():
    from nefii_amd import texture
    from nefii_amd.mesh import extract_mesh
    model, mc, sd = scene_model('bowl_trained', 'conf')
    m = extract_mesh(model, resolution=96, keep='largest', simplify=4)
    F = m.faces.shape[0]
    size = 12 * ref.atlas(F, 8192)['n']                          # the smallest size with cells of 12 texels
    baked = texture.bake_textures(model, m, size)
    return dict(model=model, mc=mc, sd=sd, mesh=m, size=size, baked=baked)


def test_bake_of_the_fitted_bowl_against_the_oracle(bowl):
    from nefii_amd import texture
    from oracle import nets
    model, mc, sd, m, size, baked = (bowl[k] for k in ('model', 'mc', 'sd', 'mesh', 'size', 'baked'))
    T, F = size, m.faces.shape[0]
    a = baked.atlas
    assert (a.size, a.cell, a.leg, a.pad, a.n_faces) == (T, 12, 6, 2, F) and F > 500
    assert baked.owner.shape == (T, T) and baked.owner.dtype == torch.int32 and baked.covered.dtype == torch.bool
    assert baked.diffuse_albedo.shape == (T, T, 3) and baked.roughness.shape == (T, T) and baked.normal.shape == (T, T, 3)
    assert baked.position.shape == (T, T, 3) and baked.specular_reflection.shape == (3,)
    assert all(t.is_cuda and t.dtype == torch.float32 for t in (baked.diffuse_albedo, baked.roughness, baked.normal))
    assert torch.equal(baked.owner.cpu(), texture.texel_owner(a))
    meta = baked.meta
    assert sorted(meta) == sorted(['size', 'cell', 'leg', 'pad', 'owned_texels', 'covered_texels', 'project', 'bake_s', 'raster_s',
                                   'network_s'])
    assert meta['owned_texels'] == int((baked.owner >= 0).sum()) and meta['covered_texels'] == int(baked.covered.sum())
    assert meta['covered_texels'] == F * (6 * 7 // 2) and meta['project'] is True       # leg 6: 21 centres inside every chart
    assert meta['bake_s'] > 0 and abs(meta['raster_s'] + meta['network_s'] - meta['bake_s']) < 1e-9
    assert not baked.diffuse_albedo[baked.owner < 0].any() and not baked.normal[baked.owner < 0].any()
    # the projection moves the texels from their faces towards the level set, by no more than the vertex projection may
    raw = texture.bake_textures(model, m, size, project=False)
    assert raw.meta['project'] is False and torch.equal(raw.owner, baked.owner) and torch.equal(raw.covered, baked.covered)
    cov2 = baked.covered
    with torch.no_grad():
        sdf = model.implicit_network.value_feature_gradient(baked.position[cov2])[0].abs()
        sdf_raw = model.implicit_network.value_feature_gradient(raw.position[cov2])[0].abs()
    moved = (baked.position[cov2] - raw.position[cov2]).abs().max().item()
    print('bowl, %d faces, %d^2: %d owned, %d covered texels; mean |sdf| at the covered texels %.3e on the faces, %.3e projected; '
          'largest move %.3e of %.3e; bake %.4f s (raster %.5f s)' % (
              F, T, meta['owned_texels'], meta['covered_texels'], sdf_raw.mean().item(), sdf.mean().item(), moved,
              0.5 * m.meta['simplify']['cell'], meta['bake_s'], meta['raster_s']))
    assert sdf.mean().item() < sdf_raw.mean().item() and moved <= 0.5 * m.meta['simplify']['cell'] * (1 + 1e-6)
    # 1500 random covered texels against the CPU oracle at the texels' own positions
    cov = baked.covered.reshape(-1).nonzero()[:, 0]
    idx = cov[torch.randperm(cov.shape[0], generator=torch.Generator().manual_seed(0))[:1500].to(DEV)]
    x = baked.position.reshape(-1, 3)[idx]
    g = nets.sdf_gradient(sd, mc['implicit_network'], x.cpu())
    g = g / g.norm(dim=1, keepdim=True)
    n_err = (baked.normal.reshape(-1, 3)[idx].cpu() - g).norm(dim=1)
    with torch.no_grad():
        _, feat, _ = model.implicit_network.value_feature_gradient(x)
    want = nets.material_forward(sd, mc['envmap_material_network'], x.cpu(), feat.cpu() if feat is not None else None)
    a_err = (baked.diffuse_albedo.reshape(-1, 3)[idx].cpu() - want['sg_diffuse_albedo']).abs().max().item()
    r_err = (baked.roughness.reshape(-1)[idx].cpu() - want['sg_roughness'].expand(1500, 1)[:, 0]).abs().max().item()
    print('against the oracle at 1500 covered texels: albedo max %.3e, roughness max %.3e, normals max %.3e mean %.3e'
          % (a_err, r_err, n_err.max().item(), n_err.mean().item()))
    assert a_err < 2e-3 and r_err < 2e-3, (a_err, r_err)
    assert n_err.max().item() < 5e-3 and n_err.mean().item() < 5e-4, (n_err.max().item(), n_err.mean().item())
    s_ref = model.envmap_material_network.specular_inv_remap(want['sg_specular_reflectance'])
    s_ref = s_ref.reshape(-1, s_ref.shape[-1])[0].expand(3)
    assert (baked.specular_reflection.cpu() - s_ref).abs().max().item() < 1e-4
    assert torch.equal(baked.specular_reflection, m.specular_reflection[0])


def test_textures_beat_vertex_attributes_and_finer_textures_beat_coarser(bowl):
    """Measured on the first GPU run: see the printed line and DESIGN.md 6p."""
    from nefii_amd import texture
    model, m, size, baked = (bowl[k] for k in ('model', 'mesh', 'size', 'baked'))
    r1 = texture.verify_textures(model, m, baked, 20000)
    fine = texture.bake_textures(model, m, 2 * size)
    r2 = texture.verify_textures(model, m, fine, 20000)
    for r in (r1, r2):
        print(json.dumps(r))
    assert r1['samples'] == 20000 and (r1['size'], r2['size']) == (size, 2 * size) and fine.atlas.cell == 24
    # the same samples: the per-vertex figures do not depend on the texture
    assert r1['vertex_albedo_mean'] == r2['vertex_albedo_mean'] and r1['vertex_roughness_mean'] == r2['vertex_roughness_mean']
    for name in ('albedo', 'roughness'):
        assert r1['texture_%s_mean' % name] < r1['vertex_%s_mean' % name], (name, r1)
        assert r2['texture_%s_mean' % name] < r1['texture_%s_mean' % name], (name, r1, r2)
    # lookups at the texel centres give the texels back
    a = baked.atlas
    cov = baked.covered.reshape(-1).nonzero()[:, 0][::97]
    face = baked.owner.reshape(-1)[cov]
    i, j = (cov % a.size).double(), (cov // a.size).double()
    xy = texture.corner_xy(a, DEV)[face.long()]
    sign = torch.where(face % 2 == 0, 1.0, -1.0).double()
    b1 = sign * (i + 0.5 - xy[:, 0, 0]) / a.leg
    b2 = sign * (j + 0.5 - xy[:, 0, 1]) / a.leg
    got = texture.sample_textures(baked, face, torch.stack([1 - b1 - b2, b1, b2], 1))
    assert (got['diffuse_albedo'] - baked.diffuse_albedo.reshape(-1, 3)[cov]).abs().max().item() < 1e-6
    assert got['roughness'].shape == (cov.shape[0], 1) and got['normal'].shape == (cov.shape[0], 3)


def test_a_second_bake_gives_the_same_bits(bowl):
    from nefii_amd import texture
    again = texture.bake_textures(bowl['model'], bowl['mesh'], bowl['size'])
    for name in ('owner', 'covered', 'position', 'diffuse_albedo', 'roughness', 'normal', 'specular_reflection'):
        assert torch.equal(getattr(again, name), getattr(bowl['baked'], name)), name
    # in chunks that start mid-row: the same texels, the same points under them
    whole = texture.bake_textures(bowl['model'], bowl['mesh'], bowl['size'], project=False)
    chunk = bowl['size'] ** 2 // 3 + 7                            # three chunks, none a multiple of the row
    parts = texture.bake_textures(bowl['model'], bowl['mesh'], bowl['size'], project=False, chunk=chunk)
    for name in ('owner', 'covered', 'position'):
        assert torch.equal(getattr(parts, name), getattr(whole, name)), name
    assert parts.meta['owned_texels'] == whole.meta['owned_texels'] and chunk % bowl['size'] != 0
    enc, enc2 = texture.encode_textures(bowl['baked']), texture.encode_textures(again)
    for k in ('albedo', 'normal', 'roughness'):
        assert enc[k].dtype == torch.uint8 and torch.equal(enc[k], enc2[k])
    assert int((enc['albedo'][..., 3] == 255).sum()) == bowl['baked'].meta['owned_texels']
    with pytest.raises(ValueError, match='at most'):
        texture.bake_textures(bowl['model'], bowl['mesh'], 64)


# ---- the command line --------------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope='module')
def experiment(tmp_path_factory):
    from nefii_amd import synthetic as syn
    tmp = tmp_path_factory.mktemp('texture_cli')
    mc = syn.model_conf('conf')
    sd = syn.make_state_dict(mc, seed=0, scene='bowl_trained')
    conf_path = tmp / 'run.conf'
    conf_path.write_text('train {\n model_class = model.implicit_differentiable_renderer.IDRNetwork\n}\nmodel { %s }\n' % _hocon(mc))
    ck = tmp / 'exps' / 'bowl' / '2026_01_01_00_00_00' / 'checkpoints' / 'ModelParameters'
    ck.mkdir(parents=True)
    torch.save({'epoch': 7, 'model_state_dict': sd}, str(ck / 'latest.pth'))
    base = [sys.executable, '-m', 'nefii_amd.scripts.extract_mesh', '--conf', str(conf_path), '--resolution', '96', '--expname',
            'bowl', '--exps_folder_name', str(tmp / 'exps')]
    return tmp, base


def test_cli_end_to_end(experiment):
    from PIL import Image
    from nefii_amd.utils.obj import read_mtl, read_obj
    from nefii_amd.utils.ply import read_ply
    tmp, base = experiment
    (tmp / 'a').mkdir()
    (tmp / 'b').mkdir()
    common = ['--simplify', '4', '--keep', 'largest']
    r = subprocess.run(base + common + ['--out', str(tmp / 'a' / 'bowl.ply'), '--texture', '1024', '--verify_texture', '5000',
                                        '--texture_exr'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = subprocess.run(base + common + ['--out', str(tmp / 'b' / 'bowl.ply')], cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    assert (tmp / 'a' / 'bowl.ply').read_bytes() == (tmp / 'b' / 'bowl.ply').read_bytes()
    assert sorted(os.listdir(tmp / 'b')) == ['bowl.ply']
    assert sorted(os.listdir(tmp / 'a')) == ['bowl.mtl', 'bowl.obj', 'bowl.ply', 'bowl_albedo.exr', 'bowl_albedo.png',
                                             'bowl_normal.png', 'bowl_roughness.exr', 'bowl_roughness.png']
    ply = read_ply(str(tmp / 'a' / 'bowl.ply'))
    obj = read_obj(str(tmp / 'a' / 'bowl.obj'))
    F = len(ply['faces'])
    assert np.array_equal(obj['faces'], ply['faces']) and obj['uv'].shape == (3 * F, 2) and obj['mtllib'] == 'bowl.mtl'
    assert np.array_equal(obj['face_uv'], np.arange(3 * F).reshape(F, 3)) and obj['uv'].min() >= 0 and obj['uv'].max() <= 1
    assert np.array_equal(obj['verts'], np.stack([ply['vertex'][k] for k in 'xyz'], 1))
    mtl = read_mtl(str(tmp / 'a' / 'bowl.mtl'))
    images = {}
    for key in ('map_Kd', 'map_Pr', 'norm'):
        with Image.open(str(tmp / 'a' / mtl[key])) as im:
            images[key] = np.array(im)
        assert images[key].shape[:2] == (1024, 1024)
    assert images['map_Kd'].shape == (1024, 1024, 4) and images['norm'].shape == (1024, 1024, 4) and images['map_Pr'].ndim == 2
    assert [float(x) for x in mtl['Ks'].split()] == pytest.approx([float(ply['vertex']['specular_' + k][0]) for k in 'rgb'])
    owned = int(re.search(r'(\d+) owned texels', r.stdout).group(1))
    alpha = images['map_Kd'][..., 3]
    assert owned > 0 and int((alpha == 255).sum()) == owned and set(np.unique(alpha)) <= {0, 255}
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    print(lines[0])
    assert rec['samples'] == 5000 and rec['size'] == 1024 and rec['texture_albedo_mean'] < rec['vertex_albedo_mean']
    from nefii_amd.utils import exr
    lin = exr.imread(str(tmp / 'a' / 'bowl_albedo.exr'))
    assert lin.shape == (1024, 1024, 3) and exr.imread(str(tmp / 'a' / 'bowl_roughness.exr')).shape == (1024, 1024)
    tone = np.floor(255.0 * np.clip(np.maximum(lin.astype(np.float64), 0) ** (1 / 2.2), 0, 1) + 0.5)
    assert np.abs(tone[alpha == 255] - images['map_Kd'][..., :3][alpha == 255]).max() <= 1      # float32 pow against the kernel's fp64


def test_cli_exits_1_when_the_faces_do_not_fit(experiment):
    tmp, base = experiment
    r = subprocess.run(base + ['--out', str(tmp / 'c.ply'), '--texture', '64'], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and '--texture 64' in r.stderr and 'at most 162 faces' in r.stderr, r.stdout + r.stderr
    assert not (tmp / 'c.ply').exists()
