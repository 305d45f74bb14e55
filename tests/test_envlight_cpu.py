"""CPU checks of the lat-long map light: the fp64 oracle (tests/envlight_ref.py) against itself, the
reference's pdf and the SG fit's grid; the library's entry points and the Python layer's argument checks without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import envlight_ref as er  # noqa: E402


def lognormal_map(H, W, seed, sigma=1.5):
    g = np.random.Generator(np.random.Philox(seed))
    return np.exp(g.normal(size=(H, W, 3)) * sigma)


@pytest.mark.parametrize('coord', er.COORDS)
def test_oracle_pdf_integrates_to_one(coord):
    H, W = 24, 40
    env = lognormal_map(H, W, 1)
    M, C = er.build(env)
    k = 16
    off = (np.arange(k) + 0.5) / k
    v = ((np.arange(H)[:, None] + off[None, :]) / H).reshape(-1)
    u = ((np.arange(W)[:, None] + off[None, :]) / W).reshape(-1)
    vv, uu = np.meshgrid(v, u, indexing='ij')
    d = er.direction(uu, vv, coord).reshape(-1, 3)
    dw = 2. * np.pi ** 2 / (H * W * k * k) * np.sin(np.pi * vv).reshape(-1)
    assert abs((er.pdf(M, C, coord, d) * dw).sum() - 1.) < 1e-4


def test_oracle_sampler_chi_square():
    H, W, n = 8, 12, 10 ** 6
    env = lognormal_map(H, W, 2, sigma=1.0)
    env[3] = 0.                                        # a zero row is never drawn
    M, C = [x.astype(np.float32) for x in er.build(env)]
    g = np.random.Generator(np.random.Philox(3))
    ur, uc = g.random(n, dtype=np.float32), g.random(n, dtype=np.float32)
    i, j, d, p = er.sample(M, C, 'mitsuba', ur, uc)
    assert not (i == 3).any()
    counts = np.bincount(i * W + j, minlength=H * W).astype(np.float64)
    P = er.texel_prob(M, C, *np.meshgrid(np.arange(H), np.arange(W), indexing='ij')).reshape(-1)
    exp = P * n
    live = exp > 0
    assert counts[~live].sum() == 0
    chi2 = ((counts[live] - exp[live]) ** 2 / exp[live]).sum()
    dof = live.sum() - 1
    assert chi2 < dof + 5 * np.sqrt(2 * dof), (chi2, dof)
    # every sample lies in the texel it was drawn from, its pdf is that texel's
    ii, jj, s = er.texel_of(d, H, W, 'mitsuba')
    inside = er.edge_distance(d, H, W, 'mitsuba') > 1e-9
    assert (ii[inside] == i[inside]).all() and (jj[inside] == j[inside]).all()
    assert np.allclose(p, er.solid_angle_pdf(er.texel_prob(M, C, i, j), H, W, s), rtol=1e-6)


@pytest.mark.parametrize('coord', er.COORDS)
def test_texel_centres_round_trip(coord):
    H, W = 9, 14
    i, j, _ = er.texel_of(er.texel_centres(H, W, coord), H, W, coord)
    I, J = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    assert (i == I).all() and (j == J).all()


@pytest.mark.parametrize('coord', er.COORDS)
def test_texel_centres_near_the_sg_fit_grid(coord):
    """the map light's texel (i, j) and envmap_directions(H, W)[i, j] (the SG fit's sample grid) are within a texel"""
    from nefii_amd.lighting import texel_directions
    from nefii_amd.training.render import envmap_directions
    H, W = 16, 32
    a = texel_directions(H, W, coord).double()
    assert np.allclose(a.numpy(), er.texel_centres(H, W, coord), atol=1e-6)
    b = envmap_directions(H, W, coordinate_type=coord).double()
    ang = torch.acos(torch.clamp((a * b).sum(-1), -1., 1.))
    assert ang.max().item() <= np.hypot(np.pi / H, 2 * np.pi / W) + 1e-6


def test_oracle_pdf_matches_the_reference(golden):
    """the reference's pdf_fn_constant_2d_light on a 16 x 32 map (Blender axes) at texel-interior directions"""
    z = golden('envlight_ref')
    env, d, want = z['envmap'].numpy(), z['dirs'].numpy(), z['pdf'].numpy()
    M, C = er.build(env)
    got = er.pdf(M, C, 'blender', d)
    assert np.allclose(got, want, rtol=1e-5, atol=0)


def test_library_exports_envlight_and_checks_arguments():
    import ctypes
    from nefii_amd import _lib
    lib = _lib.lib()
    for s in ('nefii_envlight_table_bytes', 'nefii_envlight_build', 'nefii_envlight_mis_sample',
              'nefii_envlight_radiance', 'nefii_envlight_pdf'):
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 19 == lib.nefii_abi_version()
    tb = lib.nefii_envlight_table_bytes
    assert tb(0, 4) == 0 and tb(4, 0) == 0 and tb(1 << 16, 1 << 15) == 0
    assert tb(1, 1) > 0 and tb(16, 32) % 256 == 0 and tb(16, 32) >= 16 * 4 + 16 * 32 * 4
    fake = ctypes.c_void_p(256)         # never dereferenced: every call below fails its checks first
    E_ARG, E_SHAPE = -1, -2
    assert lib.nefii_envlight_build(None, 4, 4, fake, None) == E_ARG
    assert lib.nefii_envlight_build(fake, 0, 4, fake, None) == E_SHAPE
    assert lib.nefii_envlight_build(fake, 1 << 16, 1 << 15, fake, None) == E_SHAPE
    args = [fake] * 4
    assert lib.nefii_envlight_mis_sample(fake, None, 4, 4, 0, *args, 8, *args, None) == E_ARG
    assert lib.nefii_envlight_mis_sample(fake, fake, 4, 4, 0, *args, 0, *args, None) == 0
    assert lib.nefii_envlight_mis_sample(fake, fake, -1, 4, 0, *args, 8, *args, None) == E_SHAPE
    assert lib.nefii_envlight_mis_sample(fake, fake, 4, 4, 2, *args, 8, *args, None) == E_ARG
    assert lib.nefii_envlight_radiance(fake, 4, 4, 0, None, 8, fake, None) == E_ARG
    assert lib.nefii_envlight_radiance(fake, 4, 4, 0, fake, -3, fake, None) == 0
    assert lib.nefii_envlight_radiance(fake, 4, 0, 0, fake, 8, fake, None) == E_SHAPE
    assert lib.nefii_envlight_pdf(None, 4, 4, 0, fake, 8, fake, None) == E_ARG
    assert lib.nefii_envlight_pdf(fake, 0, 4, 1, fake, 8, fake, None) == E_SHAPE
    assert lib.nefii_envlight_pdf(fake, 4, 4, 1, fake, 0, fake, None) == 0


def test_envlight_ops_reject_cpu_tensors_and_bad_shapes():
    from nefii_amd import ops
    from nefii_amd.lighting import EnvmapLight
    env = torch.ones(4, 8, 3)
    with pytest.raises(RuntimeError):
        ops.envlight_table(env)
    with pytest.raises(RuntimeError):
        ops.envlight_radiance(env, 'mitsuba', torch.ones(5, 3))
    with pytest.raises(RuntimeError):
        EnvmapLight(env, 'mitsuba', device='cpu')
    for bad in (torch.ones(4, 8), torch.ones(4, 8, 4), torch.ones(0, 8, 3), torch.ones(4, 8, 3, dtype=torch.float64)):
        with pytest.raises(ValueError):
            ops.envlight_table(bad)
    with pytest.raises(ValueError):
        ops.envlight_radiance(env, 'opengl', torch.ones(5, 3))
    with pytest.raises(ValueError):
        ops.envlight_pdf(torch.zeros(10, dtype=torch.uint8), 4, 8, 'mitsuba', torch.ones(5, 3))
    with pytest.raises(ValueError):
        ops.envlight_pdf(torch.zeros(10, dtype=torch.uint8), 0, 8, 'mitsuba', torch.ones(5, 3))


def _conf_file(tmp_path, render_type):
    p = tmp_path / ('%s.conf' % render_type)
    p.write_text('model {\n  render_type = %s\n}\n' % render_type)
    return str(p)


def test_render_cli_rejects_conflicting_light_flags(tmp_path, capsys):
    from nefii_amd.scripts import render
    mc = _conf_file(tmp_path, 'pt_render_indirect_mlp')
    with pytest.raises(SystemExit) as e:
        render.main(['--conf', mc, '--light_sg', 'a.npy', '--light_envmap', 'sky.exr'])
    assert 'exclusive' in str(e.value)
    with pytest.raises(SystemExit) as e:
        render.main(['--conf', _conf_file(tmp_path, 'sg'), '--light_envmap', 'sky.exr'])
    assert 'Monte-Carlo' in str(e.value)
    with pytest.raises(SystemExit) as e:
        render.main(['--conf', mc, '--light_envmap', 'sky.exr', '--envmap_height', '0'])
    assert 'positive' in str(e.value)
