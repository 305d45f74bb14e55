"""CPU checks of the recomputed bounce under a map light: the numpy oracle (tests/bounce_ref.py) is an
unbiased estimator of the exact integral; the library's new entry point, the Python layer's argument checks and the
renderer's / render script's mode switches without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bounce_ref as br  # noqa: E402
import envlight_ref as er  # noqa: E402

DRAWS = 1 << 18
# 12 of the 32 cases of the bright-texel integral test: the first six of either axis convention (every roughness twice)
SUBSET = [c for c in br.integral_cases() if c[1] < 6]


def test_oracle_brdf_is_envlight_refs():
    """bounce_ref.brdf_cos (a normal and view per row) against envlight_ref.brdf_cos (one for all rows)"""
    g = np.random.Generator(np.random.Philox(1))
    for nrm, v, rough in br.cases(6, 7):
        wo = g.normal(size=(500, 3))
        wo /= np.linalg.norm(wo, axis=-1, keepdims=True)
        s, d = er.brdf_cos(nrm, v, wo, rough, br.ALBEDO, br.SPEC)
        m = wo.shape[0]
        s2, d2 = br.brdf_cos(br._rows(nrm, m, np.float64, 3), br._rows(v, m, np.float64, 3), wo,
                             br._rows(rough, m, np.float64), br._rows(br.ALBEDO, m, np.float64, 3), br.SPEC)
        assert np.allclose(s, s2, rtol=1e-12, atol=0) and np.allclose(d, d2, rtol=1e-12, atol=0)


def test_oracle_technique_and_density_floor():
    u0 = np.array([0., 0.3333, 0.33334, 0.6666, 0.66667, 0.99999994], np.float32)
    assert br.technique(u0).tolist() == [0, 0, 1, 1, 2, 2]
    # mix >= 1e-6 / (3 pi) and a finite weight on an all-zero map and along wo = -v
    env = np.zeros((4, 8, 3), np.float32)
    M, C = [x.astype(np.float32) for x in er.build(env)]
    nrm, v, _ = br.cases(1, 3)[0]
    wo = np.stack([-v, nrm, v])
    for dt in (np.float64, np.float32):
        mix, w = br.weight_at(wo, env, M, C, 'mitsuba', nrm, v, 0.089, br.ALBEDO, br.SPEC, dt)
        assert (mix >= dt(1e-6 / (3 * np.pi)) * (1 - 1e-6)).all() and np.isfinite(w).all() and (w == 0).all()


@pytest.mark.parametrize('coord,k', [(c[0], c[1]) for c in SUBSET], ids=lambda x: str(x))
def test_oracle_estimator_is_unbiased(coord, k):
    """|mean of 2^18 fp64 draws - exact integral| <= 5 se per channel on the bright-texel map.  (Over all 32 cases a
    prototype's worst deviation was 2.7 se, relative se 0.15-0.3 %.)"""
    _, _, nrm, v, rough = [c for c in SUBSET if c[0] == coord and c[1] == k][0]
    env = br.bright_texel_map()
    mean, se, _, peak = br.estimate(env, coord, nrm, v, rough, br.ALBEDO, br.SPEC, DRAWS, 1000 + 16 * (coord == 'blender') + k)
    s, d = er.integral(env, coord, nrm, v, rough, br.ALBEDO, br.SPEC, sub=8, fine=64)
    dev = np.abs(mean - (s + d)) / se
    print('%s %d rough %.3f: mean %s integral %s  deviation %s se  rel se %s  max weight %.1f x mean'
          % (coord, k, rough, mean, s + d, dev, se / mean, peak))
    assert (dev <= 5).all(), (coord, k, rough, mean, s + d, se)


def test_library_exports_bounce_sample_and_checks_arguments():
    import ctypes
    from nefii_amd import _lib
    lib = _lib.lib()
    assert hasattr(lib, 'nefii_envlight_bounce_sample') and 'nefii_envlight_bounce_sample' in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 19 == lib.nefii_abi_version()
    fake = ctypes.c_void_p(256)         # never dereferenced: every call below fails its checks first
    E_ARG, E_SHAPE = -1, -2
    f = lib.nefii_envlight_bounce_sample
    ins, outs = [fake] * 6, [fake] * 3
    for bad in range(6):
        a = list(ins)
        a[bad] = None
        assert f(fake, fake, 4, 4, 0, *a, 8, *outs, None) == E_ARG
    assert f(None, fake, 4, 4, 0, *ins, 8, *outs, None) == E_ARG
    assert f(fake, None, 4, 4, 0, *ins, 8, *outs, None) == E_ARG
    assert f(fake, fake, 4, 4, 0, *ins, 8, None, fake, fake, None) == E_ARG
    assert f(fake, fake, 4, 4, 0, *ins, 8, fake, None, fake, None) == E_ARG
    assert f(fake, fake, 4, 4, 2, *ins, 8, *outs, None) == E_ARG
    assert f(fake, fake, 4, 4, -1, *ins, 8, *outs, None) == E_ARG
    assert f(fake, fake, 4, 4, 0, *ins, 0, *outs, None) == 0
    assert f(fake, fake, -1, 4, 1, *ins, -5, fake, fake, None, None) == 0          # m <= 0 first
    assert f(fake, fake, -1, 4, 0, *ins, 8, *outs, None) == E_SHAPE
    assert f(fake, fake, 4, 0, 1, *ins, 8, fake, fake, None, None) == E_SHAPE      # mix_pdf may be NULL
    assert f(fake, fake, 1 << 16, 1 << 15, 0, *ins, 8, *outs, None) == E_SHAPE


def test_bounce_op_rejects_cpu_tensors_and_bad_shapes():
    from nefii_amd import ops
    m = 5
    env, table = torch.ones(4, 8, 3), torch.zeros(10, dtype=torch.uint8)
    good = dict(specular=torch.ones(3), rough=torch.ones(m, 1), albedo=torch.ones(m, 3), normal=torch.ones(m, 3),
                view=torch.ones(m, 3), uniforms=torch.rand(m, 3))
    with pytest.raises(RuntimeError):                    # CPU tensors: no fallback
        ops.envlight_bounce_sample(env, table, 'mitsuba', **good)
    with pytest.raises(ValueError):
        ops.envlight_bounce_sample(env, table, 'opengl', **good)
    for key, bad in (('uniforms', torch.rand(m, 7)), ('uniforms', torch.rand(m + 1, 3)), ('normal', torch.ones(m, 4)),
                     ('view', torch.ones(m + 1, 3)), ('albedo', torch.ones(m)), ('rough', torch.ones(m + 2)),
                     ('specular', torch.ones(2))):
        with pytest.raises(ValueError):
            ops.envlight_bounce_sample(env, table, 'mitsuba', **dict(good, **{key: bad}))
    for bad_env in (torch.ones(4, 8), torch.ones(4, 8, 4), torch.ones(0, 8, 3), torch.ones(4, 8, 3, dtype=torch.float64)):
        with pytest.raises(ValueError):
            ops.envlight_bounce_sample(bad_env, table, 'mitsuba', **good)


def test_set_envmap_light_checks_the_indirect_mode():
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.model import path_tracing_render as ptr
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    model = IDRNetwork(conf.from_dict(syn.model_conf('conf', hidden=64)))
    light = object()                                     # stored, never used here
    assert model.envmap_indirect == 'mlp'
    with pytest.raises(ValueError):
        model.set_envmap_light(light, indirect='nonsense')
    assert model.envmap_light is None
    model.set_envmap_light(light, indirect='bounce')
    assert model.envmap_light is light and model.envmap_indirect == 'bounce'
    model.set_envmap_light(light)
    assert model.envmap_indirect == 'mlp'
    model.set_envmap_light(light, 'bounce')
    model.set_envmap_light(None)
    assert model.envmap_light is None and model.envmap_indirect == 'mlp'
    with pytest.raises(ValueError):
        ptr.pt_render_indirect_mlp_envlight(light, None, None, None, torch.zeros(2, 3), None, None, model,
                                            indirect='nonsense')
    # the bounce's uniforms: [3n, 3] in [0, 1), drawn only when asked for
    torch.manual_seed(0)
    u = ptr.draw_bounce_uniforms(7, torch.device('cpu'))
    assert u.shape == (21, 3) and (u >= 0).all() and (u < 1).all()


def _conf_file(tmp_path, render_type):
    p = tmp_path / ('%s.conf' % render_type)
    p.write_text('model {\n  render_type = %s\n}\n' % render_type)
    return str(p)


def test_render_cli_rejects_bounce_without_a_map_light(tmp_path):
    from nefii_amd.scripts import render
    mc = _conf_file(tmp_path, 'pt_render_indirect_mlp')
    with pytest.raises(SystemExit) as e:
        render.main(['--conf', mc, '--envmap_indirect', 'bounce'])
    assert '--light_envmap' in str(e.value)
    with pytest.raises(SystemExit) as e:
        render.main(['--conf', mc, '--light_sg', 'a.npy', '--envmap_indirect', 'bounce'])
    assert '--light_envmap' in str(e.value)
    with pytest.raises(SystemExit):                      # argparse: not a mode
        render.main(['--conf', mc, '--light_envmap', 'sky.exr', '--envmap_indirect', 'nonsense'])
    # with a map light the closed-form render type is still refused, in either mode
    with pytest.raises(SystemExit) as e:
        render.main(['--conf', _conf_file(tmp_path, 'sg'), '--light_envmap', 'sky.exr', '--envmap_indirect', 'bounce'])
    assert 'Monte-Carlo' in str(e.value)
