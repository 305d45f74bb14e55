"""Mesh export without a GPU: the marching-cubes table and conventions (through the numpy oracle tests/mc_ref.py, which
reads the table the kernels compile), the PLY writer / reader, and the command line's argument errors."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import mc_ref  # noqa: E402


def components6(mask):
    """connected groups of the inside corners of one cell, joined along cube edges"""
    ins = [c for c in range(8) if (mask >> c) & 1]
    par = {c: c for c in ins}

    def root(c):
        while par[c] != c:
            c = par[c]
        return c
    for a, b in itertools.combinations(ins, 2):
        if bin(a ^ b).count('1') == 1:
            par[root(a)] = root(b)
    return len({root(c) for c in ins})


def test_table_header_is_the_generator_output():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_mc_table.py'), '--check'])
    assert r.returncode == 0, 'nefii_amd/csrc/mc_tables.h differs from tools/make_mc_table.py'
    assert mc_ref.NTRI.max() <= 5 and mc_ref.NTRI[0] == 0 and mc_ref.NTRI[255] == 0


@pytest.mark.parametrize('mask', range(256))
def test_every_corner_pattern_gives_closed_spheres(mask):
    v = np.ones((4, 4, 4), np.float32)
    for c in range(8):
        v[1 + (c & 1), 1 + ((c >> 1) & 1), 1 + ((c >> 2) & 1)] = -1.0 if (mask >> c) & 1 else 0.5
    verts, faces = mc_ref.marching_cubes(v)
    if mask == 0:
        assert len(faces) == 0 and len(verts) == 0
        return
    assert mc_ref.is_closed_oriented(faces), mask
    assert mc_ref.euler(verts, faces) == 2 * components6(mask), mask
    assert mc_ref.area_volume(verts, faces)[1] > 0


@pytest.mark.parametrize('seed', range(6))
def test_random_fields_with_exact_level_values_are_closed(seed):
    r = np.random.default_rng(seed)
    v = r.integers(-2, 3, (24, 24, 24)).astype(np.float32) * 0.5 + 0.25 * (seed % 2)
    level = 0.25 * (seed % 2)                                      # ties: many grid values equal the level
    v[[0, -1]] = v[:, [0, -1]] = v[:, :, [0, -1]] = level + 1.0     # padded with outside values
    assert (v == level).mean() > 0.1
    verts, faces = mc_ref.marching_cubes(v, level)
    assert len(faces) > 1000
    assert mc_ref.is_closed_oriented(faces)
    assert len(np.unique(faces)) == len(verts)                     # every vertex is used
    assert mc_ref.area_volume(verts, faces)[1] > 0


def _grid(shape, lo=-1.0, hi=1.0):
    axes = [np.linspace(lo, hi, n, dtype=np.float32) for n in shape]
    sp = tuple((hi - lo) / (n - 1) for n in shape)
    return np.meshgrid(*axes, indexing='ij'), sp


def analytic(name, shape=(128, 128, 128)):
    """(volume, level, spacing, origin, euler, area, volume) for the analytic shapes"""
    (X, Y, Z), sp = _grid(shape)
    if name == 'sphere':
        r = 0.7
        return np.sqrt(X * X + Y * Y + Z * Z) - r, 0.0, sp, 2, 4 * np.pi * r * r, 4 / 3 * np.pi * r ** 3
    if name == 'torus':
        R, r = 0.6, 0.25
        q = np.sqrt(X * X + Y * Y) - R
        return np.sqrt(q * q + Z * Z) - r, 0.0, sp, 0, 4 * np.pi ** 2 * R * r, 2 * np.pi ** 2 * R * r * r
    if name == 'two_spheres':
        r = 0.35
        d = np.minimum(np.sqrt((X - 0.45) ** 2 + Y * Y + Z * Z), np.sqrt((X + 0.45) ** 2 + Y * Y + Z * Z)) - r
        return d, 0.0, sp, 4, 2 * 4 * np.pi * r * r, 2 * 4 / 3 * np.pi * r ** 3
    if name == 'sphere_sq':                                         # a non-distance field, level != 0
        r = 0.6
        return X * X + Y * Y + Z * Z, r * r, sp, 2, 4 * np.pi * r * r, 4 / 3 * np.pi * r ** 3
    raise KeyError(name)


@pytest.mark.parametrize('name,shape', [('sphere', (128, 128, 128)), ('torus', (128, 128, 128)),
                                        ('two_spheres', (128, 128, 128)), ('sphere_sq', (120, 136, 128)),
                                        ('torus', (136, 128, 120))])
def test_analytic_shapes(name, shape):
    vol, level, sp, chi, area, volume = analytic(name, shape)
    verts, faces = mc_ref.marching_cubes(vol.astype(np.float32), level, origin=(-1.0, -1.0, -1.0), spacing=sp)
    assert mc_ref.is_closed_oriented(faces)
    assert mc_ref.euler(verts, faces) == chi
    a, v = mc_ref.area_volume(verts, faces)
    assert v > 0                                                   # outward winding
    assert abs(a / area - 1) < 0.01 and abs(v / volume - 1) < 0.01, (a / area, v / volume)
    assert verts.min() >= -1.0 and verts.max() <= 1.0


def test_vertex_order_and_position_conventions():
    v = np.ones((2, 3, 4), np.float32)
    v[0, 1, 2] = -1.0                                              # one inside point on the x = 0 face: five crossing edges
    verts, faces = mc_ref.marching_cubes(v, 0.0, origin=(10.0, 20.0, 30.0), spacing=(1.0, 2.0, 4.0))
    # owned by (0,1,1) along z, by (0,1,2) along x / y / z and by (0,0,2) along y; numbered by owner index, then axis
    want = [(0, 1, 1.5), (0.5, 1, 2), (0, 1.5, 2), (0, 1, 2.5), (0, 0.5, 2)]
    owners = sorted([((0 * 3 + 1) * 4 + 1, 2, want[0]), ((0 * 3 + 1) * 4 + 2, 0, want[1]),
                     ((0 * 3 + 1) * 4 + 2, 1, want[2]), ((0 * 3 + 1) * 4 + 2, 2, want[3]),
                     ((0 * 3 + 0) * 4 + 2, 1, want[4])])
    exp = np.array([[10 + p[0], 20 + 2 * p[1], 30 + 4 * p[2]] for _, _, p in owners], np.float32)
    assert np.array_equal(verts, exp)
    assert len(faces) == 4                                         # an open cap: the surface leaves the grid at x = 0


def test_ply_round_trip(tmp_path):
    from nefii_amd.utils.ply import read_ply, write_ply
    r = np.random.default_rng(0)
    verts = r.standard_normal((50, 3)).astype(np.float32)
    faces = r.integers(0, 50, (70, 3))
    normals = r.standard_normal((50, 3)).astype(np.float32)
    p = str(tmp_path / 'a.ply')
    write_ply(p, verts, faces, comments=['resolution 64 level 0'])
    back = read_ply(p)
    assert list(back['vertex']) == ['x', 'y', 'z'] and back['comments'] == ['resolution 64 level 0']
    assert np.array_equal(np.stack([back['vertex'][k] for k in 'xyz'], 1), verts)
    assert np.array_equal(back['faces'], faces)
    props = {'red': r.integers(0, 256, 50).astype(np.uint8), 'green': np.zeros(50, np.uint8),
             'blue': np.full(50, 255, np.uint8), 'albedo_r': r.random(50), 'roughness': r.random((50, 1))}
    write_ply(p, verts, faces, normals=normals, vertex_props=props)
    back = read_ply(p)
    assert list(back['vertex']) == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue', 'albedo_r', 'roughness']
    assert back['vertex']['red'].dtype == np.uint8 and np.array_equal(back['vertex']['red'], props['red'])
    assert np.array_equal(back['vertex']['nz'], normals[:, 2])
    assert np.allclose(back['vertex']['roughness'], props['roughness'][:, 0].astype(np.float32))
    with open(p, 'rb') as f:
        head = f.read(200)
    assert head.startswith(b'ply\nformat binary_little_endian 1.0\n')
    assert b'property list uchar int vertex_indices' in open(p, 'rb').read()
    write_ply(p, np.zeros((0, 3)), np.zeros((0, 3)))
    back = read_ply(p)
    assert back['faces'].shape == (0, 3) and back['vertex']['x'].shape == (0,)
    with pytest.raises(ValueError):
        write_ply(p, verts, np.array([[0, 1, 50]]))


def test_cli_argument_errors(tmp_path, capsys):
    from nefii_amd.scripts import extract_mesh
    conf = tmp_path / 'a.conf'
    conf.write_text('train { }\nmodel { }\n')
    ck = tmp_path / 'g.pth'
    ck.write_bytes(b'')
    assert extract_mesh.main(['--conf', str(conf), '--geometry', str(ck)]) == 2
    assert '--out' in capsys.readouterr().err
    assert extract_mesh.main(['--conf', str(conf), '--geometry', str(tmp_path / 'none.pth'), '--out', 'x.ply']) == 2
    assert 'no checkpoint' in capsys.readouterr().err
    assert extract_mesh.main(['--conf', str(conf), '--expname', 'e', '--exps_folder_name', str(tmp_path)]) == 2
    assert 'no experiment' in capsys.readouterr().err
    (tmp_path / 'e' / '2026_01_01_00_00_00' / 'checkpoints' / 'ModelParameters').mkdir(parents=True)
    assert extract_mesh.main(['--conf', str(conf), '--expname', 'e', '--exps_folder_name', str(tmp_path),
                              '--checkpoint', '7']) == 2
    assert 'no checkpoint' in capsys.readouterr().err
    assert extract_mesh.main(['--conf', str(conf), '--geometry_neus', str(ck), '--out', 'x.ply',
                              '--resolution', '1']) == 2
    with pytest.raises(SystemExit):
        extract_mesh.main(['--geometry', str(ck)])                 # --conf is required
    assert 'pair_budget' in extract_mesh.build_parser().format_help()
