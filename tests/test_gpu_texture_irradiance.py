"""The irradiance bake on the GPU (csrc/nefii_texbake.hip, nefii_amd/texture.py) against the numpy restatement of
tests/texbake_irradiance_ref.py: the ray kernel's uniforms and cosine rows bit for bit, its map rows' texels exactly, directions
and weights to fp32 rounding; the accumulate kernel to one rounding; the refusals; whole bakes of the fitted bowl under a
constant map, suns below and above it and a rotated sun, against the exact integral inside the bound that the reference's own
CPU run sets (tests/test_texture_irradiance_cpu.py); and the command line.  Budget: a few seconds per test."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import envlight_ref as env  # noqa: E402
import texbake_ao_ref as ao  # noqa: E402
import texbake_irradiance_ref as ref  # noqa: E402
import texbake_ref  # noqa: E402

DEV = torch.device('cuda:0')
AXIS = ref.BOWL_AXIS
EPS = 2.0 ** -24
DIR_BOUND = 3e-6 + 27 * EPS + 0.5 * EPS


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ray_inputs(m, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.random((m, 3)) * 1.8 - 0.9).astype(np.float32)
    normal = ao.unit_normals(m, rng)
    sdf = rng.normal(0.0, 5e-3, size=m).astype(np.float32)
    gnorm = rng.uniform(0.5, 1.5, size=m).astype(np.float32)
    texel = rng.integers(0, 2 ** 26, size=m).astype(np.int64)
    return pos, normal, sdf, gnorm, texel


def hdr_map(H, W, seed):
    """a random HDR map: log-normal texels, a few of them zero, one at 1e4"""
    rng = np.random.default_rng(seed)
    m = np.exp(rng.normal(0.0, 1.0, size=(H, W, 3))).astype(np.float32)
    m[rng.integers(0, H, 5), rng.integers(0, W, 5)] = 0.0
    m[H // 3, W // 4] = 1e4
    return m


def stored_table(table, H, W):
    """(M [H], C [H, W]) float32: the CDFs as the kernel stored them"""
    raw = table.cpu().numpy()
    c0 = (4 * H + 255) // 256 * 256
    return raw[:4 * H].view(np.float32).copy(), raw[c0:c0 + 4 * H * W].view(np.float32).reshape(H, W).copy()


SKEW = ref.rotation_between([1.0, 0.0, 0.0], np.array([0.48, 0.6, 0.64]))      # no symmetry of any map


# ---- the ray kernel against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize('K_cos,K_map', [(1, 0), (0, 1), (2, 1), (17, 16), (32, 32)])
@pytest.mark.parametrize('m', [1, 63, 64, 65, 1000])
def test_ray_kernel_matches_the_reference(m, K_cos, K_map):
    """Both coordinate types, with and without a rotation, under a random 8 x 16 HDR map with zero texels and one at 1e4.

    Directions: the cosine rows carry the 6r bound, 3e-6.  A map row's v = (i + dv) / H has dv = (x - prev) / w with three fp32
    roundings (the difference is exact or carries one relative rounding, Sterbenz), the sum one of H and the quotient one: under
    2.4 2^-24 in v and likewise in u; the angles pi v and 2 pi u then carry 7.5 and 14 units of 2^-24, sinpif and cospif two ulp
    each and the product one: 27 2^-24 = 1.6e-6, and the rotation's single rounding 2^-25.  Asserted for every row: 3e-6 + 27.5
    2^-24 = 4.64e-6.
    Weights, relative, against the fp64 weight along the kernel's own fp32 direction: p_map carries texel_prob's three roundings,
    H W / (2 PI_F^2 sin phi) five and PI_F^2's 5.6e-8 (one unit), sin phi = rho / r four; c / PI_F, the two products, the sum,
    the quotient and the product with L seven more with PI_F's half unit: 24 2^-24 covers them.  c = n . w itself carries 3 2^-24
    absolute, so 3 2^-24 / c relative; a map row's sin phi = sinpif(v) carries pi 2.4 2^-24 absolute, 8 2^-24 / sin phi relative.
    Rows with c < 2^-20 are left to the exact-zero check, cosine rows within 1e-5 rad of a texel edge may read the neighbour.
    Measured on an MI355X over all 100 runs: directions within 4.1e-7, weights within 0.22 of their bound (largest relative
    error 2.7e-3, at a grazing ray), uniforms, origins and cosine rows bit for bit."""
    from nefii_amd import ops
    seed, bias = 11 + K_cos, 3e-3
    K = K_cos + K_map
    pos, normal, sdf, gnorm, texel = ray_inputs(m, 100 * K + m)
    args = [gpu(a) for a in (pos, normal, sdf, gnorm, texel)]
    envmap = hdr_map(8, 16, K + m)
    H, W = envmap.shape[:2]
    g_map = gpu(envmap)
    table = ops.envlight_table(g_map)
    M32, C32 = stored_table(table, H, W)
    worst = dict(d=0.0, w=0.0, share=0.0)
    for coord in ref.COORDS:
        for R in (None, SKEW):
            rot = None if R is None else gpu(R)
            origins, dirs, weight, uniforms = ops.bake_irradiance_rays(*args, K_cos, K_map, g_map, table, coord, seed, bias, rot=rot,
                                                                       want_uniforms=True)
            assert origins.shape == (m, 3) and dirs.shape == (K, m, 3) and weight.shape == (K, m, 3) and uniforms.shape == (K, m, 2)
            assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (origins, dirs, weight, uniforms))
            d, w, u = dirs.cpu().numpy(), weight.cpu().numpy(), uniforms.cpu().numpy()
            w_u = ref.uniforms(texel, K_cos, K_map, seed)
            assert np.array_equal(u.view(np.uint32), w_u.view(np.uint32))                             # bit for bit
            o_ao, d_ao, _ = ops.bake_ao_rays(*args, max(K_cos, 1), seed, bias)
            assert torch.equal(origins, o_ao)
            if K_cos:
                assert torch.equal(dirs[:K_cos], d_ao)                                                 # the occlusion bake's rays
            w_d, picked = ref.directions(w_u, normal, K_cos, M32, C32, coord, R)
            d_err = np.abs(d.astype(np.float64) - w_d).max()
            assert d_err <= DIR_BOUND
            assert np.abs(np.linalg.norm(d.astype(np.float64), axis=2) - 1.0).max() <= 2e-6
            w_w, c, sin_phi, ti, tj = ref.weights(d, normal, envmap, M32, C32, coord, K_cos, K_map, picked, R)
            local = d.astype(np.float64) if R is None else d.astype(np.float64) @ R.astype(np.float64)
            clear = env.edge_distance(local, H, W, coord) > 1e-5
            if K_map:      # the texel under a map row's direction is the texel the reference's inversion picked
                li, lj, _ = env.texel_of(local[K_cos:], H, W, coord)
                inside = clear[K_cos:]
                assert np.array_equal(li[inside], picked[0][inside]) and np.array_equal(lj[inside], picked[1][inside])
                assert (envmap[picked[0], picked[1]].mean(-1) > 0).all()
            c32 = ref.cos_f32(d, normal)
            assert not w[c32 <= 0].any()                                                               # exactly 0 below the horizon
            assert np.isfinite(w).all() and (w >= 0).all()
            rel = 24 * EPS + 3 * EPS / np.maximum(c, 2.0 ** -20)
            rel[K_cos:] += 8 * EPS / np.maximum(sin_phi[K_cos:], 1e-30)
            check = c >= 2.0 ** -20
            check[:K_cos] &= clear[:K_cos]
            err = np.abs(w.astype(np.float64) - w_w)
            ok = err <= rel[..., None] * np.abs(w_w) + 1e-300
            assert ok[check].all(), (coord, R is not None, err[check].max())
            lit = check[..., None] & (w_w > 0)
            if lit.any():
                worst['w'] = max(worst['w'], (err[lit] / w_w[lit]).max())
                worst['share'] = max(worst['share'], (err / (rel[..., None] * np.abs(w_w) + 1e-300))[lit].max())
            worst['d'] = max(worst['d'], d_err)
            # without the uniforms: the same rays
            o2, d2, w2, none = ops.bake_irradiance_rays(*args, K_cos, K_map, g_map, table, coord, seed, bias, rot=rot)
            assert none is None and torch.equal(o2, origins) and torch.equal(d2, dirs) and torch.equal(w2, weight)
            if m > 1:      # in two calls that split the texels mid-range: bitwise the one-call result
                cut = m // 3 + 1
                a = ops.bake_irradiance_rays(*(t[:cut].contiguous() for t in args), K_cos, K_map, g_map, table, coord, seed, bias,
                                             rot=rot, want_uniforms=True)
                b = ops.bake_irradiance_rays(*(t[cut:].contiguous() for t in args), K_cos, K_map, g_map, table, coord, seed, bias,
                                             rot=rot, want_uniforms=True)
                assert torch.equal(torch.cat([a[0], b[0]]), origins)
                for k, whole in ((1, dirs), (2, weight), (3, uniforms)):
                    assert torch.equal(torch.cat([a[k], b[k]], 1), whole)
            if K_map:      # another seed changes the map rows
                other = ops.bake_irradiance_rays(*args, K_cos, K_map, g_map, table, coord, seed + 1, bias, rot=rot)
                assert not torch.equal(other[1][K_cos:], dirs[K_cos:])
    # an identity matrix is the unrotated path, bit for bit
    eye = ops.bake_irradiance_rays(*args, K_cos, K_map, g_map, table, 'mitsuba', seed, bias, rot=torch.eye(3, device=DEV))
    plain = ops.bake_irradiance_rays(*args, K_cos, K_map, g_map, table, 'mitsuba', seed, bias)
    assert all(torch.equal(a, b) for a, b in zip(eye[:3], plain[:3]))
    print('m = %d, K = %d + %d: max |dir - reference| %.3e (bound %.3e), max relative weight error %.3e, at most %.3f of its bound'
          % (m, K_cos, K_map, worst['d'], DIR_BOUND, worst['w'], worst['share']))


# ---- the accumulate kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K_cos,K_map', [(3, 0), (0, 5), (17, 16)])
@pytest.mark.parametrize('m', [1, 65, 1000])
def test_accumulate_kernel_matches_the_reference(m, K_cos, K_map):
    """irradiance: an fp64 sum in the restatement's order rounded once, 2^-24 relative; asserted 2^-23.  noise: the same fp64
    operations; were they contracted or reordered, var = sum (Q - S S / n) n / (n - 1) would move by at most 4 2^-53 (Q + S S / n)
    n / (n - 1) <= 2^-49 sum Q per technique, and |sqrt a - sqrt b| <= sqrt |a - b|; with the final rounding: 2^-23 noise + 2^-24
    sqrt(2 sum Q).  Measured on an MI355X over all 9 runs: irradiance within 6.0e-8 relative, noise within 0.29 of its bound."""
    from nefii_amd import ops
    K = K_cos + K_map
    rng = np.random.default_rng(1000 * K + m)
    weight = np.exp(rng.normal(0.0, 2.0, size=(K, m, 3))).astype(np.float32)
    weight[rng.random((K, m)) < 0.3] = 0.0
    hit = (rng.random((K, m)) < 0.5).astype(np.uint8)
    if m > 1:
        hit[:, 1] = 1                                                  # every ray occluded
        hit[:, 2] = 0                                                  # every ray free
    else:
        hit[:] = 1
    hit[~weight.any(-1)] = 0xa5                                        # poison: the hit of a zero-weight row is never traced
    E, noise = ops.bake_irradiance_accumulate(gpu(hit), gpu(weight), K_cos, K_map)
    assert E.shape == (m, 3) and noise.shape == (m,) and E.dtype == torch.float32 and noise.dtype == torch.float32
    w_E, w_noise = ref.accumulate(hit, weight, K_cos, K_map)
    e_err = np.abs(E.cpu().numpy().astype(np.float64) - w_E)
    assert (e_err <= 2.0 ** -23 * np.abs(w_E)).all()
    y = weight.astype(np.float64).mean(-1) * ((hit == 0) & weight.any(-1))
    n_bound = 2.0 ** -23 * w_noise + 2.0 ** -24 * np.sqrt(2.0 * (y * y).sum(0))
    n_err = np.abs(noise.cpu().numpy().astype(np.float64) - w_noise)
    print('m = %d, K = %d + %d: max relative irradiance error %.3e (bound %.3e), max noise error %.3e of its bound' % (
        m, K_cos, K_map, (e_err / np.maximum(np.abs(w_E), 1e-300)).max(), 2.0 ** -23, (n_err / np.maximum(n_bound, 1e-300)).max()))
    assert (n_err <= n_bound).all()
    col = 1 if m > 1 else 0
    assert not E[col].any() and noise[col].item() == 0.0               # all occluded: exactly 0
    if m > 1:
        assert np.abs(E[2].cpu().numpy() - weight[:, 2].astype(np.float64).sum(0)).max() <= 2.0 ** -23 * weight[:, 2].sum(0).max()
    if m > 1:
        assert (w_noise > 0).any()                                      # (more than one ray of a technique in every split)
    E8, n8 = ops.bake_irradiance_accumulate(gpu(hit != 0), gpu(weight), K_cos, K_map)              # a bool mask is the uint8 mask
    assert torch.equal(E8, E) and torch.equal(n8, noise)


def test_kernels_refuse_before_anything_is_enqueued():
    from nefii_amd import _lib, ops
    lib = _lib.lib()
    m = 65
    pos, normal, sdf, gnorm, texel = (gpu(a) for a in ray_inputs(m, 3))
    g_map = gpu(hdr_map(8, 16, 0))
    table = ops.envlight_table(g_map)
    rot = gpu(SKEW)
    origins = torch.full((m, 3), 7.0, device=DEV)
    dirs, weight = torch.full((8, m, 3), 7.0, device=DEV), torch.full((8, m, 3), 7.0, device=DEV)
    uniforms = torch.full((8 * m * 2 + 1,), 7.0, device=DEV)
    E, noise = torch.full((m, 3), 7.0, device=DEV), torch.full((m,), 7.0, device=DEV)
    hit = torch.zeros(8, m, dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else t.data_ptr()                                              # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream

    def rays(K_cos=2, K_map=2, H=8, W=16, coord=0, pos_=pos, map_=g_map, table_=table, weight_=weight, uni=None, count=m):
        return lib.nefii_bake_irradiance_rays(p(pos_), p(normal), p(sdf), p(gnorm), p(texel), count, K_cos, K_map, 0, 0.0, p(map_),
                                              p(table_), H, W, coord, p(rot), 0, p(origins), p(dirs), p(weight_), uni, stream)

    def acc(K_cos=2, K_map=2, hit_=hit, weight_=weight, E_=E, noise_=noise, count=m):
        return lib.nefii_bake_irradiance_accumulate(p(hit_), p(weight_), count, K_cos, K_map, p(E_), p(noise_), stream)

    assert rays(pos_=None) == -1 and rays(map_=None) == -1 and rays(table_=None) == -1 and rays(weight_=None) == -1
    assert rays(uni=uniforms.data_ptr() + 4) == -1 and rays(coord=2) == -1
    for bad in (dict(K_cos=0, K_map=0), dict(K_cos=1000, K_map=25), dict(K_cos=-1, K_map=4), dict(K_cos=4, K_map=-1), dict(H=0),
                dict(W=0), dict(H=-8), dict(H=1 << 16, W=1 << 15), dict(count=-1), dict(count=1 << 31)):
        assert rays(**bad) == -2, bad
    assert acc(hit_=None) == -1 and acc(weight_=None) == -1 and acc(E_=None) == -1 and acc(noise_=None) == -1
    for bad in (dict(K_cos=0, K_map=0), dict(K_cos=1000, K_map=25), dict(K_cos=-1, K_map=4), dict(K_cos=4, K_map=-1),
                dict(count=-1)):
        assert acc(**bad) == -2, bad
    torch.cuda.synchronize()
    for t in (origins, dirs, weight, uniforms, E, noise):              # nothing was written
        assert bool((t == 7.0).all())
    with pytest.raises(ValueError, match='rays'):
        ops.bake_irradiance_rays(pos, normal, sdf, gnorm, texel, 1000, 25, g_map, table, 'mitsuba')
    with pytest.raises(ValueError, match='negative'):
        ops.bake_irradiance_rays(pos, normal, sdf, gnorm, texel, -1, 4, g_map, table, 'mitsuba')
    with pytest.raises(ValueError):
        ops.bake_irradiance_rays(pos, normal, sdf, gnorm, texel, 2, 2, g_map, table[:-1], 'mitsuba')
    with pytest.raises(ValueError):
        ops.bake_irradiance_rays(pos, normal, sdf, gnorm, texel, 2, 2, g_map, table, 'maya')
    with pytest.raises(ValueError):
        ops.bake_irradiance_rays(pos, normal, sdf, gnorm, texel, 2, 2, g_map, table, 'mitsuba', rot=rot[:2])
    with pytest.raises(ValueError):
        ops.bake_irradiance_accumulate(hit, weight, 2, 2)              # 8 rows, 4 rays
    assert rays() == 0 and acc(K_cos=4, K_map=4) == 0                  # the next good call is served
    torch.cuda.synchronize()
    assert torch.isfinite(dirs[:4]).all() and bool((dirs[4:] == 7.0).all()) and torch.isfinite(E).all()
    out = ops.bake_irradiance_rays(pos[:0], normal[:0], sdf[:0], gnorm[:0], texel[:0], 2, 2, g_map, table, 'mitsuba')
    assert out[1].shape == (4, 0, 3) and out[2].shape == (4, 0, 3)


# ---- whole bakes of the fitted bowl ------------------------------------------------------------------------------------------
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
    return model


@pytest.fixture(scope='module')
def bowl():
    """the recipe of test_gpu_texture_ao.py's fixture, the two suns below the bowl of texbake_irradiance_ref.sun_cases and one
    bake of 16 + 16 rays under the plain one that the tests below share"""
    from nefii_amd import texture
    from nefii_amd.lighting import EnvmapLight
    from nefii_amd.mesh import extract_mesh
    model = scene_model('bowl_trained', 'conf')
    m = extract_mesh(model, resolution=96, keep='largest', simplify=4)
    size = 12 * texbake_ref.atlas(m.faces.shape[0], 8192)['n']      # the smallest size with cells of 12 texels
    baked = texture.bake_textures(model, m, size)
    meta = dict(baked.meta)
    suns = {name: dict(map=envmap, R=R, s=s, light=EnvmapLight(gpu(envmap))) for name, envmap, R, s in ref.sun_cases()}
    irr = texture.bake_irradiance(model, m, baked, suns['plain']['light'], rays=32)
    return dict(model=model, mesh=m, size=size, baked=baked, baked_meta=meta, suns=suns, irr=irr)


def shells(baked):
    """(outer, inner) masks [T,T] of the covered texels on the bowl's outer and inner shell, away from the rim"""
    pos = baked.position.double()
    radius = pos.norm(dim=2)
    below = (pos * torch.from_numpy(AXIS).to(DEV)).sum(2) < -0.25
    return baked.covered & below & (radius > 0.64), baked.covered & below & (radius > 0.55) & (radius < 0.60)


def sun_error(baked, irr, sun, R='own'):
    """(the mean relative error of the bake against exact_irradiance over the covered texels of the outer shell whose normals
    have n . s > 0.3, their count); R: the rotation the reference is given (the sun's own unless said)"""
    outer, _ = shells(baked)
    n = baked.normal[outer].cpu().numpy()
    lit = n.astype(np.float64) @ sun['s'] > 0.3
    exact = ref.exact_irradiance(sun['map'], n[lit], sun['R'] if isinstance(R, str) else R)
    with np.errstate(divide='ignore', invalid='ignore'):
        return ref.relative_error(irr.irradiance[outer].cpu().numpy()[lit], exact).mean(), int(lit.sum())


def test_constant_map_gives_pi_times_the_occlusion(bowl):
    """Under a map of ones and cosine rays alone every ray weighs fl(c / fl(32 fl(c / PI_F))): two roundings (the product with 32
    and the sum with 0 p_map are exact) and PI_F's 2.8e-8, under 2.5 2^-24 relative; the fp64 sum rounds once more.  Asserted
    against pi times the occlusion bake's ao, which traces the same rays: 4 2^-24 relative, in every channel of every owned
    texel.  Measured on an MI355X: 1.04e-7 over 181 872 owned texels."""
    from nefii_amd import texture
    from nefii_amd.lighting import EnvmapLight
    model, m, baked = (bowl[k] for k in ('model', 'mesh', 'baked'))
    occ = texture.bake_occlusion(model, m, baked, rays=32)
    irr = texture.bake_irradiance(model, m, baked, EnvmapLight(torch.ones(8, 16, 3, device=DEV)), rays=32, map_share=0)
    assert (irr.meta['rays_cos'], irr.meta['rays_map'], irr.meta['skipped_rays']) == (32, 0, 0)
    assert irr.meta['traced_rays'] == occ.meta['traced_rays']
    owned = baked.owner >= 0
    want = np.pi * occ.ao[owned].double()[:, None].expand(-1, 3)
    err = (irr.irradiance[owned].double() - want).abs()
    rel = (err / want.clamp_min(1e-300))[want > 0].max().item()
    print('constant map: max relative |E - pi ao| %.3e (bound %.3e) over %d owned texels' % (rel, 4 * EPS, int(owned.sum())))
    assert bool((err <= 4 * EPS * want).all())


def test_sun_below_the_bowl(bowl):
    """The bound is texbake_irradiance_ref.SUN_MIX_BOUND = 0.0434: three times the worst mean relative error, 0.01446, of the
    reference estimator itself over seeds 0 .. 3 and both suns (tests/test_texture_irradiance_cpu.py).  Measured on an MI355X:
    0.01365 over 13 245 texels with 16 + 16 rays, 1.528 with 32 cosine rays, 112 times worse; 1 445 605 rays traced, 4 374 299
    skipped."""
    from nefii_amd import texture
    model, m, baked, irr = (bowl[k] for k in ('model', 'mesh', 'baked', 'irr'))
    sun = bowl['suns']['plain']
    mix, count = sun_error(baked, irr, sun)
    cosine = texture.bake_irradiance(model, m, baked, sun['light'], rays=32, map_share=0)
    cos_err, _ = sun_error(baked, cosine, sun)
    print('sun below the bowl: mean relative error %.5f over %d texels with 16 + 16 rays (bound %.4f), %.4f with 32 cosine rays: '
          '%.1f times worse; %d rays traced, %d skipped' % (mix, count, ref.SUN_MIX_BOUND, cos_err, cos_err / mix,
                                                            irr.meta['traced_rays'], irr.meta['skipped_rays']))
    assert count > 1000
    assert mix <= ref.SUN_MIX_BOUND
    assert cos_err > mix
    owned = baked.owner >= 0
    away = owned & ((baked.normal.double() * torch.from_numpy(sun['s']).to(DEV)).sum(2) < -0.3)
    assert int(away.sum()) > 1000 and not irr.irradiance[away].any() and not irr.noise[away].any()


def test_sun_above_the_bowl(bowl):
    from nefii_amd import texture
    from nefii_amd.lighting import EnvmapLight
    model, m, baked = (bowl[k] for k in ('model', 'mesh', 'baked'))
    H, W = ref.SUN_SHAPE
    light = EnvmapLight(gpu(ref.sun_map(H, W, *ref.nearest_texel(H, W, AXIS, 'mitsuba'))))
    irr = texture.bake_irradiance(model, m, baked, light, rays=32)
    outer, inner = shells(baked)
    mean_inner = irr.irradiance[inner].double().mean().item()
    print('sun above the bowl: mean irradiance %.4f over %d covered texels of the inner shell; %d rays traced, %d skipped' % (
        mean_inner, int(inner.sum()), irr.meta['traced_rays'], irr.meta['skipped_rays']))
    assert mean_inner > 0
    assert int(outer.sum()) > 1000 and not irr.irradiance[outer].any()


def test_rotated_sun(bowl):
    """the sun authored at texel (5, 11) and carried to -AXIS by the rotation: the bound of test_sun_below_the_bowl, the reference
    given R; given the transposed rotation it is another light.  Measured on an MI355X: 0.01385 over 13 374 texels; unbounded
    against the transposed rotation, whose lit side is the dark one."""
    from nefii_amd import texture
    model, m, baked = (bowl[k] for k in ('model', 'mesh', 'baked'))
    sun = bowl['suns']['rotated']
    irr = texture.bake_irradiance(model, m, baked, sun['light'], rays=32, rotation=torch.from_numpy(sun['R']))
    err, count = sun_error(baked, irr, sun)
    wrong, _ = sun_error(baked, irr, sun, sun['R'].T)
    print('rotated sun: mean relative error %.5f over %d texels (bound %.4f); against the transposed rotation %s' % (
        err, count, ref.SUN_MIX_BOUND, wrong))
    assert count > 1000 and err <= ref.SUN_MIX_BOUND
    assert not wrong <= ref.SUN_MIX_BOUND
    # the light's own rotation is the same rotation
    own = texture.bake_irradiance(model, m, baked, sun['light'].rotated(torch.from_numpy(sun['R'])), rays=32)
    assert torch.equal(own.irradiance, irr.irradiance) and torch.equal(own.noise, irr.noise)


def test_a_second_bake_and_a_bake_in_chunks_give_the_same_bits(bowl):
    from nefii_amd import texture
    model, m, baked, irr = (bowl[k] for k in ('model', 'mesh', 'baked', 'irr'))
    light = bowl['suns']['plain']['light']
    again = texture.bake_irradiance(model, m, baked, light, rays=32)
    assert torch.equal(again.irradiance, irr.irradiance) and torch.equal(again.noise, irr.noise)
    parts = texture.bake_irradiance(model, m, baked, light, rays=32, ray_chunk=32 * 1000)
    owned = baked.meta['owned_texels']
    assert owned > 3000 and owned % 1000 != 0
    assert torch.equal(parts.irradiance, irr.irradiance) and torch.equal(parts.noise, irr.noise)
    for b in (irr, again, parts):
        assert b.meta['skipped_rays'] > 0 and b.meta['traced_rays'] + b.meta['skipped_rays'] == 32 * owned
    assert parts.meta['traced_rays'] == irr.meta['traced_rays']


def test_fields_encoding_and_report(bowl):
    from nefii_amd import texture
    model, m, baked, irr = (bowl[k] for k in ('model', 'mesh', 'baked', 'irr'))
    T = bowl['size']
    assert irr.irradiance.shape == (T, T, 3) and irr.noise.shape == (T, T)
    assert irr.irradiance.dtype == torch.float32 and irr.noise.dtype == torch.float32 and irr.irradiance.is_cuda and irr.noise.is_cuda
    unowned = baked.owner < 0
    assert unowned.any() and not irr.irradiance[unowned].any() and not irr.noise[unowned].any()
    assert bool((irr.irradiance >= 0).all()) and bool((irr.noise >= 0).all()) and bool(torch.isfinite(irr.irradiance).all())
    meta = irr.meta
    assert sorted(meta) == sorted(['rays', 'rays_cos', 'rays_map', 'bias', 'seed', 'traced_rays', 'skipped_rays',
                                   'off_surface_texels', 'irradiance_s', 'mean_irradiance_covered', 'mean_noise_covered'])
    assert (meta['rays'], meta['rays_cos'], meta['rays_map'], meta['bias'], meta['seed']) == (32, 16, 16, 0.0, 0)
    assert meta['irradiance_s'] > 0
    assert abs(meta['mean_irradiance_covered'] - irr.irradiance[baked.covered].double().mean().item()) < 1e-9
    assert abs(meta['mean_noise_covered'] - irr.noise[baked.covered].double().mean().item()) < 1e-9
    assert baked.meta == bowl['baked_meta']                                                       # the material bake's stays
    with pytest.raises(ValueError, match='project'):
        unprojected = texture.BakedTextures(**{**vars(baked), 'meta': {**baked.meta, 'project': False}})
        texture.bake_irradiance(model, m, unprojected, bowl['suns']['plain']['light'])
    with pytest.raises(ValueError, match='ray_chunk'):
        texture.bake_irradiance(model, m, baked, bowl['suns']['plain']['light'], rays=32, ray_chunk=31)
    # the encoding against its definition in fp64
    for exposure in (1.0, 0.02):
        enc = texture.encode_irradiance(baked, irr, exposure)
        assert sorted(enc) == ['irradiance', 'lit'] and torch.equal(enc['irradiance'], irr.irradiance)
        assert enc['lit'].shape == (T, T, 4) and enc['lit'].dtype == torch.uint8
        x = (exposure * baked.diffuse_albedo.double() * irr.irradiance.double() / np.pi).float().double()   # rounded once
        want = (255.0 * x.clamp_min(0.0).pow(1.0 / 2.2).clamp(0.0, 1.0) + 0.5).floor().to(torch.uint8)
        owned = ~unowned
        assert torch.equal(enc['lit'][..., :3][owned], want[owned]) and not enc['lit'][unowned].any()
        assert torch.equal(enc['lit'][..., 3] == 255, owned)
    assert int(want[owned].max()) > 0
    report = texture.verify_irradiance(model, m, baked, irr, bowl['suns']['plain']['light'], 500, rays=64)
    print(json.dumps(report))
    assert sorted(report) == sorted(['samples', 'size', 'rays', 'bake_rays', 'irradiance_mean', 'irradiance_max', 'direct_mean',
                                     'noise_mean', 'verify_noise_mean'])
    assert report['samples'] == 500 and report['size'] == T and report['rays'] == 64 and report['bake_rays'] == 32
    assert 0.0 <= report['irradiance_mean'] <= report['irradiance_max'] and report['direct_mean'] > 0
    assert report['noise_mean'] == meta['mean_noise_covered']


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


def test_cli_end_to_end(tmp_path):
    from PIL import Image
    from nefii_amd import synthetic as syn
    from nefii_amd.utils import exr
    mc = syn.model_conf('conf')
    sd = syn.make_state_dict(mc, seed=0, scene='bowl_trained')
    conf_path = tmp_path / 'run.conf'
    conf_path.write_text('train {\n model_class = model.implicit_differentiable_renderer.IDRNetwork\n}\nmodel { %s }\n' % _hocon(mc))
    ck = tmp_path / 'exps' / 'bowl' / '2026_01_01_00_00_00' / 'checkpoints' / 'ModelParameters'
    ck.mkdir(parents=True)
    torch.save({'epoch': 7, 'model_state_dict': sd}, str(ck / 'latest.pth'))
    sky = hdr_map(16, 32, 4)
    exr.imwrite(str(tmp_path / 'sky.exr'), sky)
    base = [sys.executable, '-m', 'nefii_amd.scripts.extract_mesh', '--conf', str(conf_path), '--resolution', '96', '--expname',
            'bowl', '--exps_folder_name', str(tmp_path / 'exps'), '--texture', '432', '--simplify', '4', '--keep', 'largest']
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    r = subprocess.run(base + ['--out', str(tmp_path / 'a' / 'bowl.ply'), '--texture_irradiance', str(tmp_path / 'sky.exr'),
                               '--irradiance_rays', '16', '--irradiance_map_share', '0.25', '--irradiance_rotate', '30,10,-20',
                               '--irradiance_exposure', '0.1', '--verify_irradiance', '500'], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = subprocess.run(base + ['--out', str(tmp_path / 'b' / 'bowl.ply')], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    old = ['bowl.mtl', 'bowl.obj', 'bowl.ply', 'bowl_albedo.png', 'bowl_normal.png', 'bowl_roughness.png']
    assert sorted(os.listdir(tmp_path / 'b')) == old
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(old + ['bowl_irradiance.exr', 'bowl_lit.png'])
    for name in old:                                                   # every other file is what it was, byte for byte
        assert (tmp_path / 'a' / name).read_bytes() == (tmp_path / 'b' / name).read_bytes(), name
    E = exr.imread(str(tmp_path / 'a' / 'bowl_irradiance.exr'))
    with Image.open(str(tmp_path / 'a' / 'bowl_lit.png')) as im:
        lit = np.array(im)
    with Image.open(str(tmp_path / 'a' / 'bowl_albedo.png')) as im:
        albedo = np.array(im)
    assert E.shape == (432, 432, 3) and E.dtype == np.float32 and lit.shape == (432, 432, 4) and lit.dtype == np.uint8
    assert np.isfinite(E).all() and (E >= 0).all() and E.max() > 0 and not E[albedo[..., 3] == 0].any()
    assert np.array_equal(lit[..., 3], albedo[..., 3]) and lit[..., :3].max() > 0
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    print(lines[0])
    summary = [ln for ln in r.stdout.splitlines() if ln.startswith('extract_mesh: irradiance')]
    assert len(summary) == 1 and '12 + 4 rays' in summary[0]
    print(summary[0])
    assert rec['samples'] == 500 and rec['size'] == 432 and rec['bake_rays'] == 16
    assert 0.0 <= rec['irradiance_mean'] <= rec['irradiance_max']
