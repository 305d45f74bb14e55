"""The irradiance bake without a GPU: the numpy restatement tests/texbake_irradiance_ref.py against the exact
integral under three maps - which is where the statistical bounds of tests/test_gpu_texture_irradiance.py come from - its
sequences and its accumulate step against hand-made cases, and the refusals of the entry points, of the host layer and of the
command line that need no device."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import texbake_ao_ref as ao  # noqa: E402
import texbake_irradiance_ref as ref  # noqa: E402

COUNT = 400


def points(seed):
    rng = np.random.default_rng(seed)
    return ao.unit_normals(COUNT, rng), rng.integers(0, 2 ** 26, size=COUNT).astype(np.int64)


def hdr_map(H, W, seed):
    """a random HDR map: log-normal texels, a few of them zero, one at 1e4"""
    rng = np.random.default_rng(seed)
    m = np.exp(rng.normal(0.0, 1.0, size=(H, W, 3))).astype(np.float32)
    m[rng.integers(0, H, 5), rng.integers(0, W, 5)] = 0.0
    m[H // 3, W // 4] = 1e4
    return m


def test_sequences_are_stratified_and_the_cosine_rows_are_the_occlusion_bakes():
    texel = np.array([0, 1, 12345, 2 ** 26 - 1, 2 ** 40 + 7], dtype=np.int64)
    for K_cos, K_map in ((1, 0), (0, 1), (2, 1), (17, 16), (32, 32)):
        u = ref.uniforms(texel, K_cos, K_map, seed=9)
        assert u.shape == (K_cos + K_map, 5, 2) and u.dtype == np.float32
        assert (u >= 0).all() and (u < 1).all()
        if K_cos:
            assert np.array_equal(u[:K_cos], ao.uniforms(texel, K_cos, 9))
        if K_map:
            strata = np.sort(np.floor(u[K_cos:, :, 0].astype(np.float64) * K_map).astype(int), axis=0)
            # a stratum's edge may round across (r2 + (s + 0.5) / K in fp32): every stratum once, up to one neighbour's slip
            assert (np.abs(strata - np.arange(K_map)[:, None]) <= 1).all()
        if K_cos and K_map > 1:
            assert not np.array_equal(u[K_cos:K_cos + 2, :, 0], ao.uniforms(texel, K_map, 9)[:2, :, 0])   # offsets of its own
    assert not np.array_equal(ref.uniforms(texel, 2, 2, 0)[2:], ref.uniforms(texel, 2, 2, 1)[2:])


def test_inversion_finds_the_texel_and_stays_inside_it():
    envmap = hdr_map(8, 16, 0)
    M32, C32 = ref.stored_table(envmap)
    assert M32[-1] == 1.0 and (C32[:, -1] == 1.0).all()
    rng = np.random.default_rng(1)
    u = rng.random((64, 50, 2)).astype(np.float32)
    u[0, :, 0], u[1, :, 1], u[2] = 0.0, 0.0, np.float32(1.0 - 2.0 ** -24)
    i, j, v, uu = ref.sample_map(u, M32, C32)
    assert ((np.floor(v * 8) == i) & (np.floor(uu * 16) == j)).all()
    Mprev = np.where(i > 0, M32[np.maximum(i - 1, 0)], 0.0)
    assert ((Mprev <= u[..., 0]) & ((u[..., 0] < M32[i]) | (i == 7))).all()
    zero = envmap.mean(-1) == 0
    assert zero.sum() >= 1 and not zero[i, j].any()                       # a texel without light is never drawn


@pytest.mark.parametrize('coord', ref.COORDS)
def test_constant_and_hdr_maps_against_the_exact_integral(coord):
    """The estimator is unbiased under any split of the rays: over 400 normals the mean signed relative error stays within five
    standard errors of zero (the points' sequences are independent: every texel index hashes to offsets of its own).  Under a
    constant map the cosine rays alone are exact - every weight is pi L / K - up to the midpoint rule of exact_irradiance (1 /
    (24 sub^2) of the cosine's second derivative, 1e-4 at sub = 32) and the fp32 directions."""
    n, texel = points(3)
    one = np.ones((8, 16, 3), dtype=np.float32)
    exact = ref.exact_irradiance(one, n, None, coord)
    assert np.abs(exact - np.pi).max() < 1e-3
    assert ref.relative_error(ref.estimate(one, n, texel, 32, 0, coord), exact).max() < 2e-4
    R = ref.rotation_between([1.0, 0.0, 0.0], np.array([0.6, 0.0, 0.8]))
    for envmap, rot in ((one, None), (hdr_map(8, 16, 5), None), (hdr_map(8, 16, 6), R)):
        exact = ref.exact_irradiance(envmap, n, rot, coord)
        assert (exact > 0).all()
        for K_cos, K_map in ((16, 16), (0, 32), (24, 8)):
            est = ref.estimate(envmap, n, texel, K_cos, K_map, coord, seed=2, R=rot)
            signed = (est.mean(-1) - exact.mean(-1)) / exact.mean(-1)
            print('%s, %d + %d rays: mean |relative error| %.4f, mean signed %.5f +- %.5f' % (
                coord, K_cos, K_map, np.abs(signed).mean(), signed.mean(), signed.std() / np.sqrt(COUNT)))
            assert abs(signed.mean()) <= 5.0 * signed.std() / np.sqrt(COUNT)
    # the rotation is world-from-light: the transposed one is another light
    wrong = ref.exact_irradiance(hdr_map(8, 16, 6), n, R.T, coord)
    assert ref.relative_error(wrong, exact).mean() > 0.05


def test_sun_map_the_mix_beats_cosine_sampling():
    """One texel of a 16 x 32 map at 1000, 32 rays: on the normals that see the sun (n . s > 0.3) the 16 + 16 mix misses the
    exact irradiance by 1.20 % .. 1.45 % on average (seeds 0 .. 3, both suns of sun_cases), 32 cosine rays by 138 % .. 164 %.
    The worst, 0.014456, times three is texbake_irradiance_ref.SUN_MIX_BOUND = 0.0434, the bound of the GPU bakes."""
    worst = 0.0
    for name, envmap, R, s in ref.sun_cases():
        for seed in range(4):
            mix = ref.sun_deviation(envmap, R, s, 16, 16, seed)
            cos = ref.sun_deviation(envmap, R, s, 32, 0, seed)
            print('%s sun, seed %d: mean relative error %.5f (16 + 16), %.4f (32 cosine rays)' % (name, seed, mix, cos))
            assert mix < cos
            assert mix <= ref.SUN_MIX_BOUND                                # the reference alone stays inside the bound
            worst = max(worst, mix)
    assert abs(worst - ref.SUN_MIX_WORST) <= 0.02 * ref.SUN_MIX_WORST     # ... and the bound is this run's
    assert ref.SUN_MIX_BOUND == 3.0 * ref.SUN_MIX_WORST


def test_accumulate_against_hand_made_rows():
    w = np.zeros((5, 3, 3), dtype=np.float32)
    w[:, 0] = [[3, 3, 3], [1, 1, 1], [0, 0, 0], [2, 2, 2], [4, 4, 4]]      # texel 0: luminances 3, 1, -, 2, 4
    w[:, 1] = 1.0
    hit = np.zeros((5, 3), dtype=np.uint8)
    hit[2, 0] = 255                                                        # a zero-weight row's hit is never looked at
    hit[:, 1] = 1                                                          # texel 1: all occluded
    hit[4, 0] = 1
    E, noise = ref.accumulate(hit, w, 3, 2)
    assert np.array_equal(E[0], [6, 6, 6]) and np.array_equal(E[1], [0, 0, 0]) and np.array_equal(E[2], [0, 0, 0])
    # texel 0: cosine rows 3, 1, 0 -> (10 - 16 / 3) 3 / 2 = 7; map rows 2, 0 (occluded) -> (4 - 4 / 2) 2 / 1 = 4
    assert abs(noise[0] - np.sqrt(11.0)) < 1e-12 and noise[1] == 0 and noise[2] == 0
    E1, n1 = ref.accumulate(hit[:1], w[:1], 1, 0)                          # one ray: no variance to estimate
    assert np.array_equal(E1[0], [3, 3, 3]) and not n1.any()


def test_entry_points_exist_and_refuse_without_a_device():
    """the refusals come before anything is enqueued, so pointers that are merely not NULL are never followed"""
    from nefii_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    X = 64                                                                 # not NULL, 8-byte aligned, never read
    def rays(K_cos=2, K_map=2, m=5, H=8, W=16, coord=0, pos=X, table=X, weight=X, uniforms=None, rot=None):
        return lib.nefii_bake_irradiance_rays(pos, X, X, X, X, m, K_cos, K_map, 0, 0.0, X, table, H, W, coord, rot, 0, X, X, weight,
                                              uniforms, None)
    assert rays(pos=None) == -1 and rays(table=None) == -1 and rays(weight=None) == -1
    assert rays(uniforms=12) == -1 and rays(coord=2) == -1
    for bad in (dict(K_cos=0, K_map=0), dict(K_cos=1024, K_map=1), dict(K_cos=-1, K_map=4), dict(K_cos=4, K_map=-1),
                dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15), dict(m=-1), dict(m=1 << 31)):
        assert rays(**bad) == -2, bad
    assert rays(m=0) == 0 and rays(m=0, K_cos=1024, K_map=0, uniforms=X, rot=X) == 0
    acc = lib.nefii_bake_irradiance_accumulate
    assert acc(None, X, 5, 2, 2, X, X, None) == -1 and acc(X, X, 5, 2, 2, None, X, None) == -1
    assert acc(X, None, 5, 2, 2, X, X, None) == -1 and acc(X, X, 5, 2, 2, X, None, None) == -1
    for K_cos, K_map in ((0, 0), (1000, 25), (-1, 2), (2, -1)):
        assert acc(X, X, 5, K_cos, K_map, X, X, None) == -2
    assert acc(X, X, -1, 2, 2, X, X, None) == -2 and acc(X, X, 0, 2, 2, X, X, None) == 0
    assert lib.nefii_abi_version() == 19


def test_host_layer_and_ops_refuse_without_a_device():
    import torch
    from nefii_amd import ops, texture
    from nefii_amd.lighting import EnvmapLight
    light = object.__new__(EnvmapLight)                                    # the checks below never reach the map
    light.rotation = None
    for kw, word in ((dict(rays=0), 'rays'), (dict(rays=1025), 'rays'), (dict(map_share=-0.1), 'map_share'),
                     (dict(map_share=1.5), 'map_share'), (dict(bias=-1.0), 'bias'), (dict(seed=-1), 'seed')):
        with pytest.raises(ValueError, match=word):
            texture.bake_irradiance(None, None, None, light, **kw)
    with pytest.raises(ValueError, match='EnvmapLight'):
        texture.bake_irradiance(None, None, None, 'sky.exr')
    assert texture._check_irradiance('x', light, 64, 0.5, 0.0, 0, None)[:2] == (32, 32)
    assert texture._check_irradiance('x', light, 33, 0.5, 0.0, 0, None)[:2] == (33 - round(16.5), round(16.5))
    assert texture._check_irradiance('x', light, 7, 0.0, 0.0, 0, torch.eye(3))[::4] == (7, None)     # the identity is no rotation
    z = torch.zeros(4, 3)
    with pytest.raises(RuntimeError):
        ops.bake_irradiance_rays(z, z, z[:, 0], z[:, 0], torch.zeros(4, dtype=torch.int64), 2, 2, z, z, 'mitsuba')
    with pytest.raises(RuntimeError):
        ops.bake_irradiance_accumulate(torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4, 3), 2, 2)


def test_command_line_refuses_before_the_gpu_is_touched(tmp_path, capsys):
    from nefii_amd.scripts import extract_mesh
    sky = tmp_path / 'sky.exr'
    sky.write_bytes(b'')                                                   # it is there; nothing reads it before the checks
    base = ['--conf', str(tmp_path / 'none.conf'), '--expname', 'bowl']
    cases = [(['--texture_irradiance', str(sky)], '--texture'),
             (['--texture', '64', '--texture_irradiance', str(sky), '--irradiance_rays', '0'], '--irradiance_rays'),
             (['--texture', '64', '--texture_irradiance', str(sky), '--irradiance_rays', '1025'], '--irradiance_rays'),
             (['--texture', '64', '--texture_irradiance', str(sky), '--irradiance_map_share', '1.01'], '--irradiance_map_share'),
             (['--texture', '64', '--texture_irradiance', str(sky), '--irradiance_map_share', '-0.5'], '--irradiance_map_share'),
             (['--texture', '64', '--texture_irradiance', str(sky), '--irradiance_rotate', '1,2'], '--irradiance_rotate'),
             (['--texture', '64', '--texture_irradiance', str(sky), '--coordinate_type', 'maya'], '--coordinate_type'),
             (['--texture', '64', '--texture_irradiance', str(sky), '--no_texture_project'], '--no_texture_project'),
             (['--texture', '64', '--texture_irradiance', str(tmp_path / 'gone.exr')], '--texture_irradiance'),
             (['--texture', '64', '--irradiance_rays', '8'], '--texture_irradiance'),
             (['--texture', '64', '--verify_irradiance', '8'], '--texture_irradiance')]
    for flags, word in cases:
        assert extract_mesh.main(base + flags) == 2, flags
        err = capsys.readouterr().err
        assert err.startswith('extract_mesh: ') and word in err, (flags, err)
