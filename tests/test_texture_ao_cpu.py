"""The ambient-occlusion bake without a GPU: the ray sequence of tests/texbake_ao_ref.py (range, one sample per
stratum, the cosine law), the restatement's frame and accumulate step on cases worked by hand, every host refusal, the MTL with
and without the occlusion map, and the command line's exit-2 refusals."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import texbake_ao_ref as ref  # noqa: E402

TEXELS = np.concatenate([np.arange(100), 2 ** 26 - 1 - np.arange(50), np.random.default_rng(0).integers(0, 2 ** 26, 50)])


def test_library_exports_the_two_kernels_and_refuses_on_the_host():
    from nefii_amd import _lib, build, ops
    build.build(verbose=False)
    lib = _lib.lib()
    for name in ('nefii_bake_ao_rays', 'nefii_bake_ao_accumulate'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 19 and ops.BAKE_AO_MAX_RAYS == ref.MAX_RAYS == 1024
    # before anything is enqueued: NULL pointers (uniforms alone may be NULL), then K outside 1 .. 1024
    assert lib.nefii_bake_ao_rays(None, 8, 8, 8, 8, 1, 4, 0, 0.0, 8, 8, None, None) == -1
    assert lib.nefii_bake_ao_rays(8, 8, 8, 8, 8, 1, 4, 0, 0.0, 8, None, None, None) == -1
    assert lib.nefii_bake_ao_rays(8, 8, 8, 8, 8, 1, 4, 0, 0.0, 8, 8, 12, None) == -1          # uniforms not 8-byte aligned
    assert lib.nefii_bake_ao_accumulate(8, 8, 8, 8, None, 1, 4, 0.0, 8, 8, None) == -1
    for K in (0, 1025, -1):
        assert lib.nefii_bake_ao_rays(8, 8, 8, 8, 8, 1, K, 0, 0.0, 8, 8, None, None) == -2, K
        assert lib.nefii_bake_ao_accumulate(8, 8, 8, 8, 8, 1, K, 0.0, 8, 8, None) == -2, K
    assert lib.nefii_bake_ao_rays(8, 8, 8, 8, 8, -1, 4, 0, 0.0, 8, 8, None, None) == -2
    assert lib.nefii_bake_ao_rays(8, 8, 8, 8, 8, 0, 4, 0, 0.0, 8, 8, None, None) == 0           # no texel: no launch
    assert lib.nefii_bake_ao_accumulate(8, 8, 8, 8, 8, 0, 1024, 0.0, 8, 8, None) == 0


# ---- the sequence ------------------------------------------------------------------------------------------------------------
def test_lowbias32_and_bit_reversal():
    assert ref.lowbias32(0) == 0
    x = 1
    x ^= x >> 16; x = x * 0x7feb352d % 2 ** 32; x ^= x >> 15; x = x * 0x846ca68b % 2 ** 32; x ^= x >> 16    # noqa: E702
    assert int(ref.lowbias32(1)) == x
    assert ref.brev32([0, 1, 2, 3, 1023]).tolist() == [0, 2 ** 31, 2 ** 30, 2 ** 31 + 2 ** 30, 1023 << 22]


@pytest.mark.parametrize('K', [1, 2, 33, 64])
@pytest.mark.parametrize('seed', [0, 1, 2 ** 32 - 1])
def test_uniforms_lie_in_the_unit_interval_one_per_stratum(K, seed):
    u = ref.uniforms(TEXELS, K, seed)
    assert u.shape == (K, 200, 2) and u.dtype == np.float32
    assert u.min() >= 0.0 and u.max() < 1.0
    # u0: one value in each stratum [j / K, (j + 1) / K) for every texel
    strata = np.floor(u[..., 0].astype(np.float64) * K).astype(np.int64)
    assert np.array_equal(np.sort(strata, axis=0), np.broadcast_to(np.arange(K)[:, None], (K, 200)))
    # u1: the van der Corput points are distinct, and rotated per texel
    if K > 1:
        assert (np.diff(np.sort(u[..., 1], axis=0), axis=0) > 0).all()
        assert len(np.unique(u[0, :, 1])) > 190 and len(np.unique(u[0, :, 0])) > 190
    assert not np.array_equal(u, ref.uniforms(TEXELS, K, seed ^ 5))
    # a function of the texel index alone: a slice of the texels gives the slice of the uniforms
    assert np.array_equal(ref.uniforms(TEXELS[37:91], K, seed), u[:, 37:91])


def test_cosine_law():
    """E[cos theta] = 2 / 3 under the cosine-weighted density: cos theta = sqrt(1 - u0)"""
    u = ref.uniforms(np.arange(1000) * 7919, 64, 0)
    mean = np.sqrt(1.0 - u[..., 0].astype(np.float64)).mean()
    print('mean cos theta over 64 x 1000 samples: %.6f (2 / 3 = %.6f)' % (mean, 2.0 / 3.0))
    assert abs(mean - 2.0 / 3.0) < 1e-3


def test_reference_directions_are_unit_and_above_the_surface():
    rng = np.random.default_rng(1)
    n = ref.unit_normals(300, rng)
    assert n[0].tolist() == [1, 0, 0] and n[2].tolist() == [-1, 0, 0] and n[1, 0] > 0.9 and n[3, 0] < -0.9
    u = ref.uniforms(np.arange(300), 33, 3)
    d = ref.directions(u, n)
    assert np.abs(np.linalg.norm(d, axis=2) - 1.0).max() < 1e-12
    cos = (d * n[None].astype(np.float64)).sum(2)
    assert cos.min() > 0.0
    # the component along the normal is sqrt(1 - u0), whichever frame carried it
    assert np.abs(cos - np.sqrt(1.0 - u[..., 0].astype(np.float64))).max() < 5e-6
    # the pole of the hemisphere is the normal
    pole = ref.directions(np.zeros((1, 300, 2), dtype=np.float32), n)
    assert np.abs(pole[0] - n).max() < 1e-6


def test_reference_origin_and_accumulate_by_hand():
    o = ref.origins([[1.0, 2.0, 3.0]], [[0.0, 0.0, 1.0]], [0.25], [0.5], bias=0.125)
    assert o.dtype == np.float32 and o.tolist() == [[1.0, 2.0, 3.0 + 0.125 - 0.5]]
    dirs = np.zeros((4, 2, 3), dtype=np.float32)
    dirs[:, :, 2] = 0.6
    dirs[0, :, 0], dirs[1, :, 0], dirs[2, :, 1], dirs[3, :, 1] = 0.8, -0.8, 0.8, -0.8
    orig = np.zeros((2, 3), dtype=np.float32)
    normal = np.array([[0, 0, 1], [0, 1, 0]], dtype=np.float32)
    pts = np.stack([dirs * 0.5, dirs * 2.0])[[0, 1, 0, 1], [0, 1, 2, 3]]            # samples 0, 2 near, 1, 3 far
    hit = np.array([[1, 1], [1, 1], [0, 1], [1, 1]], dtype=np.uint8)
    ao, bent, occluded = ref.accumulate(hit, pts, orig, dirs, normal, distance=1.0)
    assert ao.dtype == np.float32 and ao.tolist() == [0.75, 0.5]
    assert occluded.tolist() == [[True, True], [False, False], [False, True], [False, False]]
    want0 = np.array([-0.8, 0.0, 1.8]) / np.hypot(0.8, 1.8)
    assert np.abs(bent[0] - want0).max() < 1e-7 and np.abs(bent[1] - np.array([-0.8, -0.8, 1.2]) / np.sqrt(2.72)).max() < 1e-7
    ao, bent, _ = ref.accumulate(hit, pts, orig, dirs, normal, distance=0.0)           # unbounded: every hit occludes
    assert ao.tolist() == [0.25, 0.0] and np.array_equal(bent[1], [0, 1, 0])           # all occluded: the normal


# ---- refusals and files ------------------------------------------------------------------------------------------------------
def test_bake_occlusion_refusals():
    from nefii_amd import mesh, ops, texture

    class WithMaterials:
        envmap_material_network = object()
        implicit_network = object()
    v, f = torch.rand(4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]])
    m = mesh.Mesh(v, f)
    projected = SimpleNamespace(meta={'project': True})
    for kwargs, named in ((dict(rays=0), 'rays'), (dict(rays=1025), 'rays'), (dict(distance=0.0), 'distance'),
                          (dict(distance=-1.0), 'distance'), (dict(distance=float('nan')), 'distance'), (dict(bias=-1e-3), 'bias'),
                          (dict(seed=-1), 'seed'), (dict(seed=2 ** 32), 'seed'), (dict(rays=64, ray_chunk=63), 'ray_chunk')):
        with pytest.raises(ValueError, match=named):
            texture.bake_occlusion(WithMaterials(), m, projected, **kwargs)
    with pytest.raises(ValueError, match='project'):
        texture.bake_occlusion(WithMaterials(), m, SimpleNamespace(meta={'project': False}))
    with pytest.raises(ValueError, match='envmap_material_network'):
        texture.bake_occlusion(object(), m, projected)
    with pytest.raises(ValueError, match='CUDA'):
        texture.bake_occlusion(WithMaterials(), m, projected)
    with pytest.raises(ValueError, match='empty'):
        texture.bake_occlusion(WithMaterials(), mesh.Mesh(v, f[:0]), projected)
    occ = SimpleNamespace(meta={'distance': None, 'bias': 0.0, 'rays': 8})
    with pytest.raises(ValueError, match='CUDA'):
        texture.verify_occlusion(WithMaterials(), m, projected, occ, 10)
    # the ops wrappers: CPU tensors are a RuntimeError, whatever else is wrong with them
    z3, z1, t = torch.zeros(5, 3), torch.zeros(5), torch.arange(5)
    with pytest.raises(RuntimeError):
        ops.bake_ao_rays(z3, z3, z1, z1, t, 8)
    with pytest.raises(RuntimeError):
        ops.bake_ao_rays(z3, z3, z1, z1, t, 0)
    with pytest.raises(RuntimeError):
        ops.bake_ao_accumulate(torch.zeros(8, 5, dtype=torch.bool), torch.zeros(8, 5, 3), z3, torch.zeros(8, 5, 3), z3)


def test_mtl_with_and_without_the_occlusion_map(tmp_path):
    from nefii_amd.utils import obj
    spec = torch.tensor([0.25, 0.5, 0.125])
    obj.write_mtl(str(tmp_path / 'plain.mtl'), spec, 'a.png', 'r.png', 'n.png')
    obj.write_mtl(str(tmp_path / 'none.mtl'), spec, 'a.png', 'r.png', 'n.png', ao=None)
    obj.write_mtl(str(tmp_path / 'ao.mtl'), spec, 'a.png', 'r.png', 'n.png', ao='m_ao.png')
    plain = (tmp_path / 'plain.mtl').read_bytes()
    assert plain == (b'# nefii_amd baked materials\n# the normal map (norm) is in OBJECT space, not tangent space\n'
                     b'newmtl baked\nKd 1 1 1\nmap_Kd a.png\nKs 0.25 0.5 0.125\nmap_Pr r.png\nnorm n.png\n')
    assert (tmp_path / 'none.mtl').read_bytes() == plain
    with_ao = (tmp_path / 'ao.mtl').read_bytes()
    assert with_ao.startswith(plain) and with_ao.endswith(b'map_Ka m_ao.png\n')
    assert b'AMBIENT OCCLUSION' in with_ao[len(plain):]
    base = {'newmtl': obj.MATERIAL, 'Kd': '1 1 1', 'map_Kd': 'a.png', 'Ks': '0.25 0.5 0.125', 'map_Pr': 'r.png', 'norm': 'n.png'}
    assert obj.read_mtl(str(tmp_path / 'plain.mtl')) == base
    assert obj.read_mtl(str(tmp_path / 'ao.mtl')) == dict(base, map_Ka='m_ao.png')


@pytest.mark.parametrize('flags,named', [
    (['--texture_ao', '16'], '--texture_ao'),
    (['--texture', '512', '--texture_ao', '16', '--no_texture_project'], '--no_texture_project'),
    (['--texture', '512', '--texture_ao', '0'], '--texture_ao'), (['--texture', '512', '--texture_ao', '1025'], '--texture_ao'),
    (['--texture', '512', '--texture_ao', '16', '--ao_distance', '0'], '--ao_distance'),
    (['--texture', '512', '--texture_ao', '16', '--ao_distance', '-0.5'], '--ao_distance'),
    (['--texture', '512', '--texture_ao', '16', '--ao_bias', '-0.001'], '--ao_bias'),
    (['--texture', '512', '--texture_ao', '16', '--ao_seed', '-1'], '--ao_seed'),
    (['--texture', '512', '--texture_ao', '16', '--verify_ao', '0'], '--verify_ao'),
    (['--texture', '512', '--ao_distance', '0.1'], '--ao_distance'), (['--texture', '512', '--ao_bias', '0.01'], '--ao_bias'),
    (['--texture', '512', '--ao_seed', '3'], '--ao_seed'), (['--texture', '512', '--texture_bent_normal'], '--texture_bent_normal'),
    (['--texture', '512', '--texture_orm'], '--texture_orm'), (['--texture', '512', '--verify_ao', '100'], '--verify_ao'),
    (['--texture_orm'], '--texture_orm')])
def test_cli_refusals_exit_2_before_the_gpu(flags, named, tmp_path):
    """none of these reaches the conf, the checkpoint or the device: the conf named here does not exist"""
    r = subprocess.run([sys.executable, '-m', 'nefii_amd.scripts.extract_mesh', '--conf', str(tmp_path / 'none.conf'),
                        '--expname', 'x'] + flags, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stdout + r.stderr
    last = r.stderr.strip().splitlines()[-1]
    assert last.startswith('extract_mesh: ') and named in last and '--texture' in last and 'no conf' not in last, r.stderr
