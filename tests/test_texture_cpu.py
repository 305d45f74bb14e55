"""The texture bake without a GPU: the atlas of nefii_amd/texture.py against the fp64 restatement of
tests/texbake_ref.py, the bilinear footprint property that pad >= 2 buys, every host refusal, the OBJ / MTL round trip, the
command line's exit-2 refusals, and the reference's own analytic round trip on a coarse icosphere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import texbake_ref as ref  # noqa: E402


def test_library_exports_the_three_kernels():
    from nefii_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    for name in ('nefii_bake_raster', 'nefii_bake_encode', 'nefii_texture_sample'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert 'nefii_texbake.hip' in build.SOURCES and _lib.ABI_VERSION == 19
    # refused on the host, before anything is enqueued: NULL pointers, then an atlas outside the limits
    assert lib.nefii_bake_raster(None, 0, None, 0, 7, 1, 7, 2, 0, 0, None, None, None, None, None, None) == -1
    assert lib.nefii_bake_encode(None, None, None, None, 0, None, None, None, None) == -1
    assert lib.nefii_texture_sample(None, 7, 1, None, None, 1, 7, 2, 0, None, None) == -1
    for T, n, c, p in ((6, 1, 6, 2), (8193, 1, 7, 2), (7, 1, 7, 1), (7, 1, 6, 2), (13, 2, 7, 2)):
        assert lib.nefii_texture_sample(8, T, 1, 8, 8, n, c, p, 0, 8, None) == -2, (T, n, c, p)
        assert lib.nefii_bake_raster(8, 3, 8, 1, T, n, c, p, 0, 0, 8, 8, 8, 8, 8, None) == -2, (T, n, c, p)
    assert lib.nefii_texture_sample(8, 7, 5, 8, 8, 1, 7, 2, 0, 8, None) == -2              # five channels
    assert lib.nefii_bake_raster(8, 3, 8, 3, 7, 1, 7, 2, 0, 0, 8, 8, 8, 8, 8, None) == -2   # three faces, one cell
    assert lib.nefii_bake_raster(8, 3, 8, 1, 7, 1, 7, 2, 40, 10, 8, 8, 8, 8, 8, None) == -2  # texels 40 .. 49 of 49


@pytest.mark.parametrize('F,T', ref.CASES + [(5000, 2048), (2, 8192)])
def test_atlas_numbers_and_uvs_match_the_reference(F, T):
    from nefii_amd import texture
    a, r = texture.triangle_atlas(F, T), ref.atlas(F, T)
    assert (a.size, a.cells_per_row, a.cell, a.pad, a.leg, a.n_faces) == (r['T'], r['n'], r['c'], r['p'], r['s'], r['F'])
    assert a.cells_per_row ** 2 >= (F + 1) // 2 > (a.cells_per_row - 1) ** 2 and a.cell * a.cells_per_row <= T
    if F <= 200:
        uv = texture.corner_uv(a)
        assert uv.dtype == torch.float64 and uv.shape == (F, 3, 2)
        assert np.array_equal(uv.numpy(), ref.corner_uv(r))
        assert uv.min() >= 0.0 and uv.max() <= 1.0
        xy = texture.corner_xy(a)
        assert np.array_equal(xy.numpy(), np.stack([ref.corners_xy(r, f) for f in range(F)]))
        # every chart a right triangle of legs s, wound the same way in the image
        e1, e2 = xy[:, 1] - xy[:, 0], xy[:, 2] - xy[:, 0]
        assert torch.equal(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0], torch.full((F,), float(a.leg ** 2), dtype=torch.float64))


@pytest.mark.parametrize('F,T', ref.CASES)
def test_owner_image_and_disjoint_charts(F, T):
    from nefii_amd import texture
    a, r = texture.triangle_atlas(F, T), ref.atlas(F, T)
    owner = texture.texel_owner(a).numpy()
    want = ref.owner_image(r)
    assert owner.dtype == np.int32 and np.array_equal(owner, want)
    n, c = r['n'], r['c']
    # -1 exactly where the contract says: the margin, the cells past ceil(F / 2), the odd half of the last cell of an odd F
    jj, ii = np.mgrid[0:T, 0:T]
    q = (jj // c) * n + ii // c
    face = 2 * q + ((ii % c) + (jj % c) + 1 >= c)
    nobody = (ii >= n * c) | (jj >= n * c) | (q >= (F + 1) // 2) | (face >= F)
    assert np.array_equal(owner < 0, nobody) and np.array_equal(owner[~nobody], face[~nobody])
    if (F, T) == (1, 7):
        assert r['s'] == 1 and (owner == 0).sum() == 21 and (owner == -1).sum() == 28       # the upper half is nobody's
    if (F, T) == (3, 14):
        assert (owner[7:, :] == -1).all() and set(np.unique(owner[:7, 7:])) == {-1, 2}      # cells 2, 3 empty; face 3 missing
    if (F, T) == (37, 61):
        assert n * c == 60 and (owner[60, :] == -1).all() and (owner[:, 60] == -1).all()     # a margin of one texel
    # charts pairwise disjoint: every texel centre covered by a chart is covered by its owner's chart and by no other
    _, covered, _, _ = ref.raster(r, np.zeros((3, 3)), np.zeros((F, 3), dtype=np.int64))
    count = np.zeros((T, T), dtype=np.int64)
    for f in range(F):
        C = ref.corners_xy(r, f)
        M = np.array([C[1] - C[0], C[2] - C[0]]).T
        b = np.linalg.solve(M, np.stack([ii.ravel() + 0.5 - C[0, 0], jj.ravel() + 0.5 - C[0, 1]]))
        inside = ((b[0] >= -1e-12) & (b[1] >= -1e-12) & (b[0] + b[1] <= 1 + 1e-12)).reshape(T, T)
        assert (owner[inside] == f).all()
        count += inside
    assert count.max() == 1 and np.array_equal(count == 1, covered)
    # ... and the chart triangles keep a pad between each other: bounding boxes of different cells do not touch
    xy = texture.corner_xy(a)
    assert xy.min() >= a.pad and xy.max() <= n * c - a.pad


@pytest.mark.parametrize('F,T', ref.CASES)
def test_bilinear_footprint_stays_inside_the_owning_chart(F, T):
    """pad >= 2: every texel the reference sampler reads with non-zero weight at a point inside or on a chart - corners,
    edge midpoints, random edge and interior points - belongs to that chart's face"""
    r = ref.atlas(F, T)
    owner = ref.owner_image(r)
    face, bary = ref.chart_points(r, np.random.default_rng(F), 40 if F <= 37 else 12)
    xy = ref.atlas_position(r, face, bary)
    read = 0
    for f, p in zip(face, xy):
        for i, j, w in ref.footprint(r, p):
            if w != 0.0:
                assert owner[j, i] == f, (f, p, i, j, w)
                read += 1
    assert read > 9 * F


def test_pad_one_breaks_the_footprint_property():
    """why pad < 2 is refused: with pad 1 (the reference's formulas taken past the contract) lookups near a chart's long edge
    read texels of the other face of the cell"""
    for c in (7, 8, 13, 20):
        r = dict(T=c, n=1, c=c, p=1, s=c - 3, F=2)
        owner = ref.owner_image(r)
        bad = 0
        face, bary = ref.chart_points(r, np.random.default_rng(c), 200)
        for f, p in zip(face, ref.atlas_position(r, face, bary)):
            bad += sum(1 for i, j, w in ref.footprint(r, p) if w != 0.0 and owner[j, i] != f)
        assert bad > 0, c


def test_refusals():
    from nefii_amd import mesh, ops, texture
    for F, T, pad in ((1, 6, 2), (1, 8193, 2), (1, 7, 1), (1, 7, 0), (0, 64, 2), (3, 7, 2), (1, 9, 3), (1, 64, 22)):
        with pytest.raises(ValueError):
            texture.triangle_atlas(F, T, pad)
    with pytest.raises(ValueError) as e:
        texture.triangle_atlas(201, 70, 2)                # n = 11, c = 6 < 7
    assert 'at most 200 faces' in str(e.value) and '--simplify' in str(e.value) and '--texture' in str(e.value)
    assert texture.atlas_capacity(70, 2) == 200 and texture.triangle_atlas(200, 70).leg == 1
    assert texture.atlas_capacity(8192, 2) == 2 * 1170 ** 2

    class WithMaterials:
        envmap_material_network = object()
        implicit_network = object()
    v, f = torch.rand(4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(ValueError, match='envmap_material_network'):
        texture.bake_textures(object(), mesh.Mesh(v, f), 64)
    with pytest.raises(ValueError, match='CUDA'):
        texture.bake_textures(WithMaterials(), mesh.Mesh(v, f), 64)
    with pytest.raises(ValueError, match='empty'):
        texture.bake_textures(WithMaterials(), mesh.Mesh(v[:0], f[:0]), 64)
    with pytest.raises(ValueError, match='empty'):
        texture.bake_textures(WithMaterials(), mesh.Mesh(v, f[:0]), 64)
    with pytest.raises(ValueError, match='CUDA'):
        texture.verify_textures(WithMaterials(), mesh.Mesh(v, f), None, 10)
    # the ops wrappers: CPU tensors are a RuntimeError, whatever else is wrong with them
    f32 = f.int()
    with pytest.raises(RuntimeError):
        ops.bake_raster(v, f32, 7, 1, 7, 2)
    with pytest.raises(RuntimeError):
        ops.bake_raster(v.double(), f, 6, 1, 7, 1)
    with pytest.raises(RuntimeError):
        ops.bake_encode(torch.zeros(5, 3), torch.zeros(5), torch.zeros(5, 3), torch.zeros(5, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        ops.texture_sample(torch.zeros(7, 7, 3), torch.zeros(5, dtype=torch.int32), torch.zeros(5, 3, dtype=torch.float64), 1, 7, 2)
    with pytest.raises(RuntimeError):
        ops.texture_sample(None, None, None, 1, 7, 2)


def test_sample_faces_is_area_weighted_and_on_the_simplex():
    from nefii_amd import texture
    v = torch.tensor([[0., 0, 0], [1, 0, 0], [0, 1, 0], [3, 0, 0], [0, 3, 0]])
    f = torch.tensor([[0, 1, 2], [0, 3, 4]])
    face, bary = texture.sample_faces(v, f, 20000, torch.Generator().manual_seed(0))
    assert bary.dtype == torch.float64 and bary.min() >= 0 and torch.allclose(bary.sum(1), torch.ones(20000, dtype=torch.float64))
    assert abs((face == 1).float().mean().item() - 0.9) < 0.01
    face2, bary2 = texture.sample_faces(v, f, 20000, torch.Generator().manual_seed(0))
    assert torch.equal(face, face2) and torch.equal(bary, bary2)


def test_obj_and_mtl_round_trip(tmp_path):
    from nefii_amd import texture
    from nefii_amd.utils import obj
    rng = np.random.default_rng(3)
    V, F = 57, 101
    v = rng.normal(size=(V, 3)).astype(np.float32)
    n = rng.normal(size=(V, 3)).astype(np.float32)
    f = rng.integers(0, V, size=(F, 3))
    uv = texture.corner_uv(texture.triangle_atlas(F, 333))
    obj.write_obj(str(tmp_path / 'm.obj'), torch.from_numpy(v), torch.from_numpy(f), n, uv, 'm.mtl')
    got = obj.read_obj(str(tmp_path / 'm.obj'))
    assert np.array_equal(got['verts'], v) and np.array_equal(got['normals'], n) and np.array_equal(got['faces'], f)
    assert got['uv'].shape == (3 * F, 2) and np.array_equal(got['uv'].reshape(F, 3, 2), uv.numpy())
    assert np.array_equal(got['face_uv'], np.arange(3 * F).reshape(F, 3)) and np.array_equal(got['face_normals'], f)
    assert got['mtllib'] == 'm.mtl' and got['usemtl'] == obj.MATERIAL
    text = (tmp_path / 'm.obj').read_text().splitlines()
    assert sum(ln.startswith('vt ') for ln in text) == 3 * F and sum(ln.startswith('f ') for ln in text) == F
    assert text[-1] == 'f %d/%d/%d %d/%d/%d %d/%d/%d' % tuple(int(x) for k in range(3) for x in (f[-1, k] + 1, 3 * F - 2 + k, f[-1, k] + 1))
    obj.write_mtl(str(tmp_path / 'm.mtl'), torch.tensor([0.25, 0.5, 0.125]), 'a.png', 'r.png', 'n.png')
    m = obj.read_mtl(str(tmp_path / 'm.mtl'))
    assert m == {'newmtl': obj.MATERIAL, 'Kd': '1 1 1', 'map_Kd': 'a.png', 'Ks': '0.25 0.5 0.125', 'map_Pr': 'r.png', 'norm': 'n.png'}
    assert 'OBJECT space' in (tmp_path / 'm.mtl').read_text()
    for bad in (dict(normals=n[:5]), dict(corner_uv=uv[:5]), dict(faces=f + V)):
        args = dict(verts=v, faces=f, normals=n, corner_uv=uv)
        args.update(bad)
        with pytest.raises(ValueError):
            obj.write_obj(str(tmp_path / 'bad.obj'), mtl_name='m.mtl', **args)
    # an empty mesh writes and reads
    obj.write_obj(str(tmp_path / 'e.obj'), v[:0], f[:0], n[:0], uv[:0], 'e.mtl')
    assert obj.read_obj(str(tmp_path / 'e.obj'))['faces'].shape == (0, 3)


@pytest.mark.parametrize('flags,named', [
    (['--texture', '6'], '--texture'), (['--texture', '8193'], '--texture'),
    (['--texture', '512', '--texture_pad', '1'], '--texture_pad'),
    (['--texture', '512', '--no_materials'], '--no_materials'),
    (['--texture', '512', '--geometry', 'g.pth', '--out', 'o.ply'], '--geometry'),
    (['--texture', '512', '--geometry_neus', 'g.pth', '--out', 'o.ply'], '--geometry_neus'),
    (['--texture_pad', '2'], '--texture_pad'), (['--no_texture_project'], '--no_texture_project'),
    (['--texture_exr'], '--texture_exr'), (['--verify_texture', '100'], '--verify_texture')])
def test_cli_refusals_exit_2_before_the_gpu(flags, named, tmp_path):
    """none of these reaches the conf, the checkpoint or the device: the conf named here does not exist"""
    r = subprocess.run([sys.executable, '-m', 'nefii_amd.scripts.extract_mesh', '--conf', str(tmp_path / 'none.conf'),
                        '--expname', 'x'] + flags, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stdout + r.stderr
    last = r.stderr.strip().splitlines()[-1]
    assert last.startswith('extract_mesh: ') and named in last and '--texture' in last and 'no conf' not in last, r.stderr


def test_reference_encode_levels():
    ra, rn, grey, _ = ref.encode([[0.0, 1.0, 2.0], [-1.0, 0.5, 0.2], [0.3, 0.3, 0.3]], [0.0, 1.5, 0.5],
                                 [[-1.0, 0.0, 1.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0]], [0, 3, -1])
    assert ra.tolist() == [[0, 255, 255, 255], [0, 186, 123, 255], [0, 0, 0, 0]]
    assert rn.tolist() == [[0, 128, 255, 255], [128, 128, 255, 255], [0, 0, 0, 0]] and grey.tolist() == [0, 255, 0]


def test_reference_round_trip_on_an_analytic_sphere():
    """what the GPU test repeats on the fitted bowl, established here for the reference alone: on an icosphere of 320 faces
    with cells of 12 texels (leg 6), bilinear lookups of a bake of an analytic material are closer to the material than the
    barycentric interpolation of its per-vertex values - and a finer atlas is closer still"""
    verts, faces = ref.icosphere(2)
    a = ref.atlas(len(faces), 13 * 12)
    assert (len(faces), a['n'], a['c'], a['s']) == (320, 13, 12, 6)
    tex_err, vert_err = ref.round_trip_sphere(verts, faces, 13 * 12, 4000)
    tex2_err, vert2_err = ref.round_trip_sphere(verts, faces, 2 * 13 * 12, 4000)
    print('analytic sphere, 320 faces: texture mean error %.3e at c = 12, %.3e at c = 24; per-vertex interpolation %.3e'
          % (tex_err, tex2_err, vert_err))
    assert vert_err == vert2_err
    assert tex_err < vert_err and tex2_err < tex_err
