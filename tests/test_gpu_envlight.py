"""The lat-long map light on the GPU: kernels against the fp64 oracle (tests/envlight_ref.py), the
unbiasedness of the Monte-Carlo estimator under it, the renderer, and the render command line."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import envlight_ref as er  # noqa: E402

DEV = torch.device('cuda')
pytestmark = pytest.mark.gpu


def lognormal_map(H, W, seed, sigma=1.5):
    g = np.random.Generator(np.random.Philox(seed))
    return np.exp(g.normal(size=(H, W, 3)) * sigma).astype(np.float32)


def special_map(name):
    if name == 'sun':
        m = lognormal_map(32, 64, 5, 0.5)
        m[9, 40] = 1e5
        return m
    if name == 'zero_rows':
        m = lognormal_map(16, 24, 6)
        m[[0, 5, 6, 15]] = 0.
        m[3, :12] = 0.
        return m
    if name == 'all_zero':
        return np.zeros((8, 16, 3), np.float32)
    H, W = name
    return lognormal_map(H, W, H * 7919 + W)


MAPS = [(1, 1), (1, 2), (7, 13), (256, 512), (1024, 2048), 'sun', 'zero_rows', 'all_zero']


def read_table(table, H, W):
    """(M, C) as the kernel stored them (layout: csrc/nefii_envlight.hip)"""
    b = table.cpu().numpy()
    c0 = (H * 4 + 255) // 256 * 256
    M = b[:H * 4].view(np.float32).copy()
    C = b[c0:c0 + H * W * 4].view(np.float32).reshape(H, W).copy()
    return M, C


def random_dirs(n, seed):
    g = np.random.Generator(np.random.Philox(seed))
    d = g.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)


# ---- 1. kernels against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', MAPS, ids=str)
def test_table_matches_fp64_build_and_is_reproducible(name):
    from nefii_amd import ops
    env = special_map(name)
    H, W = env.shape[:2]
    t = torch.from_numpy(env).to(DEV)
    tab = ops.envlight_table(t)
    tab2 = ops.envlight_table(t)
    assert torch.equal(tab, tab2)
    M, C = read_table(tab, H, W)
    M64, C64 = er.build(env)
    assert np.abs(M - M64).max() <= 3e-7 and np.abs(C - C64).max() <= 3e-7
    assert M[-1] == 1.0 and (C[:, -1] == 1.0).all()
    assert np.isfinite(M).all() and np.isfinite(C).all()
    assert (np.diff(M) >= 0).all() and (np.diff(C, axis=1) >= 0).all()


@pytest.mark.parametrize('coord', er.COORDS)
@pytest.mark.parametrize('name', MAPS, ids=str)
def test_radiance_and_pdf_match_the_oracle(name, coord):
    from nefii_amd.lighting import EnvmapLight
    env = special_map(name)
    H, W = env.shape[:2]
    light = EnvmapLight(torch.from_numpy(env), coord)
    d = random_dirs(20000, 11)
    d = d[er.edge_distance(d, H, W, coord) > 1e-5]
    dt = torch.from_numpy(d).to(DEV)
    rgb = light.radiance(dt).cpu().numpy()
    assert np.array_equal(rgb, er.radiance(env, coord, d))
    M, C = read_table(light.table, H, W)
    want = er.pdf(M, C, coord, d)
    got = light.pdf(dt).cpu().numpy()
    assert np.allclose(got, want, rtol=1e-5, atol=0)
    # unnormalised directions: normalised first
    assert np.array_equal(light.radiance(dt * 3.5).cpu().numpy(), rgb)


def surface_points(n, seed, rough=None):
    g = torch.Generator().manual_seed(seed)
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    t = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    view = torch.nn.functional.normalize(nrm * (0.2 + torch.rand(n, 1, generator=g)) + t, dim=-1)
    view = torch.where((view * nrm).sum(-1, keepdim=True) > 0.05, view, nrm)
    r = rough if rough is not None else 0.05 + 0.95 * torch.rand(n, 1, generator=g)
    uni = torch.rand(n, 7, generator=g)
    return r.to(DEV), nrm.to(DEV), view.to(DEV), uni.to(DEV)


def ggx_pdf64(w, n, v, r):
    h = w + v
    h = h / np.linalg.norm(h, axis=-1, keepdims=True)
    c = np.maximum((h * n).sum(-1), 1e-6)
    r4 = r ** 4
    root = c * c + (1 - c * c) / r4
    return c / (np.pi * r4 * root * root) / (4 * np.maximum((h * v).sum(-1), 1e-6))


@pytest.mark.parametrize('coord', er.COORDS)
@pytest.mark.parametrize('name', [(7, 13), (256, 512), 'sun', 'zero_rows', 'all_zero', (1, 1)], ids=str)
def test_sampler_matches_the_oracle_on_its_own_table(name, coord):
    from nefii_amd import ops
    from nefii_amd.lighting import EnvmapLight
    env = special_map(name)
    H, W = env.shape[:2]
    light = EnvmapLight(torch.from_numpy(env), coord)
    n = 50000
    r, nrm, view, uni = surface_points(n, 3)
    wi, own, tab, L = light.sample(r, nrm, view, uni)
    wi, own, tab, L = [x.cpu().numpy() for x in (wi, own, tab, L)]
    M, C = read_table(light.table, H, W)
    u = uni.cpu().numpy()
    i, j, d, p = er.sample(M, C, coord, u[:, 4], u[:, 5])
    # the map row: the same texel for every draw, its direction, own pdf and radiance
    ii, jj, _ = er.texel_of(wi[2], H, W, coord)
    inside = er.edge_distance(wi[2], H, W, coord) > 1e-5
    assert (ii[inside] == i[inside]).all() and (jj[inside] == j[inside]).all()
    assert np.abs(wi[2] - d).max() < 2e-6
    # v = (i + dv) / H is rounded to fp32 in the kernel: sin(pi v) then carries a relative error of ~2e-7 / sin(phi)
    s = np.sin(np.pi * (i + np.clip((u[:, 4] - np.where(i > 0, M[np.maximum(i - 1, 0)], 0.)) /
                                    np.maximum(M[i] - np.where(i > 0, M[np.maximum(i - 1, 0)], 0.), 1e-30), 0, 1)) / H)
    tol = 1e-5 + 4e-7 / np.maximum(s, 1e-12)
    want = np.maximum(p, 1e-6)
    assert (np.abs(own[2] - want) <= tol * want).all()
    assert np.array_equal(tab[2, :, 2], own[2])
    assert np.array_equal(L[2], env[i, j])
    # the map column of the BRDF rows, and their radiance
    for k in (0, 1):
        ok = er.edge_distance(wi[k], H, W, coord) > 1e-5
        assert np.allclose(tab[k, ok, 2], er.pdf(M, C, coord, wi[k, ok]), rtol=1e-5, atol=0)
        assert np.array_equal(L[k, ok], er.radiance(env, coord, wi[k, ok]))
    # the BRDF columns of the map row (fp32 dot products: an absolute floor; GGX pdf: rel 1e-3 where the lobe is not
    # razor sharp)
    n64, v64, r64 = nrm.cpu().double().numpy(), view.cpu().double().numpy(), r.cpu().double().numpy()[:, 0]
    w2 = wi[2].astype(np.float64)
    assert np.allclose(tab[2, :, 0], np.maximum((w2 * n64).sum(-1), 1e-6) / np.pi, rtol=1e-5, atol=1e-7)
    sel = r64 > 0.3
    assert np.allclose(tab[2, sel, 1], ggx_pdf64(w2[sel], n64[sel], v64[sel], r64[sel]), rtol=1e-3, atol=1e-9)
    # rows 0 and 1 are nefii_mis_sample's, bitwise, under any SG light
    g = torch.Generator().manual_seed(5)
    for M_lobes in (1, 7, 128):
        lgt = torch.randn(M_lobes, 7, generator=g).to(DEV)
        lgt[:, 3] = lgt[:, 3].abs() * 30
        swi, sown, stab = [x.cpu().numpy() for x in ops.mis_sample(lgt, r, nrm, view, uni)]
        assert np.array_equal(swi[:2], wi[:2]) and np.array_equal(sown[:2], own[:2])
        assert np.array_equal(stab[:2, :, :2], tab[:2, :, :2])


# ---- 2. the estimator is unbiased ------------------------------------------------------------------------------------
DRAWS = 1 << 20


def cases(n_cases, seed):
    g = np.random.Generator(np.random.Philox(seed))
    out = []
    for c in range(n_cases):
        nrm = g.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        t = g.normal(size=3)
        t -= (t @ nrm) * nrm
        t /= np.linalg.norm(t)
        cv = g.uniform(0.25, 1.0)
        v = cv * nrm + np.sqrt(1 - cv * cv) * t
        out.append((nrm, v, (0.089, 0.3, 1.0)[c % 3]))
    return out


def mc_estimate(light_sample, nrm, v, rough, albedo, spec, seed, sg=None):
    """mean and standard error of nefii_mc_shade_forward's rgb / specular / diffuse over DRAWS draws (visibility 1)"""
    from nefii_amd import ops
    n = DRAWS
    g = torch.Generator(device=DEV).manual_seed(seed)
    uni = torch.rand(n, 7, device=DEV, generator=g)
    nn = torch.tensor(nrm, dtype=torch.float32, device=DEV).expand(n, 3).contiguous()
    vv = torch.tensor(v, dtype=torch.float32, device=DEV).expand(n, 3).contiguous()
    r = torch.full((n, 1), rough, device=DEV)
    a = torch.tensor(albedo, dtype=torch.float32, device=DEV).expand(n, 3).contiguous()
    s = torch.tensor(spec, dtype=torch.float32, device=DEV).reshape(1, 3)
    if sg is None:
        wi, own, tab, L = light_sample(r, nn, vv, uni)
    else:
        wi, own, tab = ops.mis_sample(sg, r, nn, vv, uni)
        L = ops.EnvRadianceFn.apply(sg, wi.reshape(-1, 3), 1e-6).reshape(3, n, 3)
    with torch.no_grad():
        rgb, srgb, drgb = ops.McShadeFn.apply(s, r, a, nn, vv, wi, own, tab, L, torch.ones(3, n, device=DEV),
                                              torch.zeros(3, n, 3, device=DEV))
    res = {}
    for k, x in (('rgb', rgb), ('spec', srgb), ('diff', drgb)):
        x = x.double()
        res[k] = (x.mean(0).cpu().numpy(), (x.std(0) / np.sqrt(n)).cpu().numpy())
    return res


@pytest.mark.parametrize('coord', er.COORDS)
def test_furnace_diffuse_mean_is_c_times_albedo(coord):
    from nefii_amd.lighting import EnvmapLight
    c = np.array([0.7, 1.3, 2.0], np.float32)
    light = EnvmapLight(torch.from_numpy(np.broadcast_to(c, (16, 32, 3)).copy()), coord)
    albedo = np.array([0.8, 0.5, 0.2])
    for k, (nrm, v, rough) in enumerate(cases(30, 1)):
        m, se = mc_estimate(light.sample, nrm, v, rough, albedo, [0.04] * 3, 100 + k)['diff']
        want = c * albedo
        assert (np.abs(m - want) <= 5 * se).all(), (k, rough, m, want, se)


def test_mean_matches_the_exact_integral_on_a_bright_texel_map():
    from nefii_amd.lighting import EnvmapLight
    env = lognormal_map(32, 64, 9, 0.6)
    env[10, 20] *= 400.
    env[25, 50] *= 50.
    spec, albedo = np.array([0.3, 0.3, 0.3]), np.array([0.6, 0.4, 0.25])
    for coord in er.COORDS:
        light = EnvmapLight(torch.from_numpy(env), coord)
        for k, (nrm, v, rough) in enumerate(cases(16, 2 + (coord == 'blender'))):
            est = mc_estimate(light.sample, nrm, v, rough, albedo, spec, 300 + k)
            s, d = er.integral(env, coord, nrm, v, rough, albedo, spec, sub=8, fine=64)
            m, se = est['rgb']
            assert (np.abs(m - (s + d)) <= 5 * se).all(), (coord, k, rough, m, s + d, se)
            if k < 3:      # the quadrature is converged: doubling it moves it by < 1/10 of the bound
                s2, d2 = er.integral(env, coord, nrm, v, rough, albedo, spec, sub=16, fine=128)
                assert (np.abs((s2 + d2) - (s + d)) < 0.5 * se).all(), (k, rough, s2 + d2, s + d, se)


def test_sg_light_and_its_map_agree():
    from nefii_amd.lighting import EnvmapLight
    g = torch.Generator().manual_seed(12)
    lgt = torch.randn(24, 7, generator=g)
    lgt[:, 3] = lgt[:, 3].abs() * 60 + 5            # sharpness 5 .. ~200
    lgt[:, 3].clamp_(max=200.)
    lgt[:, 4:] = lgt[:, 4:].abs()
    lgt = lgt.to(DEV)
    light = EnvmapLight.from_sg(lgt, 512, 1024, 'mitsuba')
    spec, albedo = np.array([0.2] * 3), np.array([0.5, 0.6, 0.7])
    for k, (nrm, v, rough) in enumerate(cases(12, 4)):
        rough = max(rough, 0.3)
        a = mc_estimate(light.sample, nrm, v, rough, albedo, spec, 500 + k)['rgb']
        b = mc_estimate(None, nrm, v, rough, albedo, spec, 600 + k, sg=lgt)['rgb']
        bound = 5 * np.hypot(a[1], b[1]) + 5e-3 * np.abs(b[0])
        assert (np.abs(a[0] - b[0]) <= bound).all(), (k, rough, a, b)


# ---- 3. renderer -----------------------------------------------------------------------------------------------------
def bowl_model():
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    mc = syn.model_conf('conf')
    sd = syn.make_state_dict(mc, seed=0, scene='bowl_trained')
    model = IDRNetwork(conf.from_dict(mc))
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    model.freeze_geometry()
    model.eval()
    return model


def crop_input(rays=64, size=32, res=64, seed=0):
    """a size x size crop of a res x res view, `rays` jittered rays per pixel, as one flat batch of rays"""
    from nefii_amd import synthetic as syn
    g = np.random.Generator(np.random.Philox(seed))
    y, x = np.meshgrid(np.arange(size) + (res - size) // 2, np.arange(size) + (res - size) // 2, indexing='ij')
    uv = np.stack([x, y], -1).reshape(-1, 1, 2) + g.uniform(-0.5, 0.5, size=(size * size, rays, 2))
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 70.
    K[0, 2] = K[1, 2] = res / 2.
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    return {'uv': f(uv.reshape(1, -1, 2)).to(DEV), 'intrinsics': f(K)[None].to(DEV),
            'pose': f(syn.look_at_origin_pose((0.6, 1.0, 2.2)))[None].to(DEV),
            'object_mask': torch.ones(1, size * size * rays, dtype=torch.bool, device=DEV)}


def render(model, inp, uniforms=None):
    model.uniforms_override = uniforms
    with torch.no_grad():
        out = model(inp)
    model.uniforms_override = None
    return out


def test_renderer_sg_light_versus_its_map():
    from nefii_amd.lighting import EnvmapLight
    model = bowl_model()
    inp = crop_input()
    torch.manual_seed(0)
    sg = render(model, inp)
    lgt = model.envmap_material_network.get_lgtSGs().detach()
    light = EnvmapLight.from_sg(lgt, 512, 1024, 'mitsuba')
    model.set_envmap_light(light)
    torch.manual_seed(1)
    env = render(model, inp)
    hit = sg['network_object_mask']
    assert torch.equal(hit, env['network_object_mask'])
    assert 0.05 < hit.float().mean().item() < 0.95
    a, b = sg['sg_rgb_values'][hit].double(), env['sg_rgb_values'][hit].double()
    se = torch.sqrt(a.var(0) / a.shape[0] + b.var(0) / b.shape[0])
    assert ((a.mean(0) - b.mean(0)).abs() <= 5 * se + 1e-2 * a.mean(0).abs()).all(), (a.mean(0), b.mean(0), se)
    # background rays: the map's texel along the ray
    from nefii_amd.utils import rend_util
    dirs, _ = rend_util.get_camera_params(inp['uv'], inp['pose'], inp['intrinsics'])
    dirs = dirs.reshape(-1, 3)
    bg = ~hit
    assert torch.equal(env['sg_rgb_values'][bg], light.radiance(dirs[bg]))
    # per-pixel means of the background (64 rays per pixel)
    pix = env['sg_rgb_values'].reshape(-1, 64, 3)
    allbg = (~hit).reshape(-1, 64).all(1)
    want = light.radiance(dirs).reshape(-1, 64, 3).mean(1)
    assert torch.allclose(pix[allbg].mean(1), want[allbg], rtol=1e-6, atol=1e-7)


def test_renderer_replay_and_detach():
    from nefii_amd.lighting import EnvmapLight
    from nefii_amd.model.path_tracing_render import draw_uniforms
    model = bowl_model()
    ref = bowl_model()
    inp = crop_input(rays=4, size=24)
    n = inp['uv'].shape[1]
    hit = render(model, inp)['network_object_mask']
    torch.manual_seed(3)
    uni = draw_uniforms(int(hit.sum().item()), DEV)
    before = render(model, inp, uni)['sg_rgb_values']
    light = EnvmapLight(torch.from_numpy(lognormal_map(64, 128, 4, 0.8)), 'mitsuba')
    model.set_envmap_light(light)
    a = render(model, inp, uni)
    b = render(model, inp, uni)
    assert torch.equal(a['sg_rgb_values'], b['sg_rgb_values'])
    assert not torch.equal(a['sg_rgb_values'], before)
    assert set(model.state_dict()) == set(ref.state_dict())
    model.set_envmap_light(None)
    c = render(model, inp, uni)
    d = render(ref, inp, uni)
    assert torch.equal(c['sg_rgb_values'], d['sg_rgb_values']) and torch.equal(c['sg_rgb_values'], before)
    assert n > 0
    # training mode and the closed-form render type refuse a map light
    model.set_envmap_light(light)
    model.train()
    with pytest.raises(RuntimeError):
        model(inp)
    model.eval()
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    physg = IDRNetwork(conf.from_dict(syn.model_conf('physg', hidden=64)))
    with pytest.raises(ValueError):
        physg.set_envmap_light(light)


# ---- 4. the command line ---------------------------------------------------------------------------------------------
def test_render_cli_with_a_map_light(tmp_path):
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.lighting import load_envmap
    from nefii_amd.scripts.render import RenderRunner
    from nefii_amd.utils import exr
    mc = syn.model_conf('conf', hidden=64)
    cfg = conf.from_dict({'train': {'model_class': 'nefii_amd.model.implicit_differentiable_renderer.IDRNetwork',
                                    'dataset_class': 'nefii_amd.datasets.synthetic_dataset.SyntheticSceneDataset'},
                          'model': mc})
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    ck = tmp_path / 'scene' / 't0' / 'checkpoints' / 'ModelParameters'
    os.makedirs(str(ck))
    torch.save({'epoch': 1, 'model_state_dict': sd}, str(ck / 'latest.pth'))
    sky = lognormal_map(24, 48, 8, 1.0)
    exr.imwrite(str(tmp_path / 'sky.exr'), sky)
    kw = dict(conf=cfg, exps_folder_name=str(tmp_path), expname='scene', timestamp='t0', checkpoint='latest',
              memory_capacity_level=10, num_rays=2, dataset_kwargs={'n_views': 2, 'img_res': (16, 16)})
    RenderRunner(new_timestamp='plain', **kw).run()
    RenderRunner(new_timestamp='relit', light_envmap_path=str(tmp_path / 'sky.exr'), envmap_height=12, envmap_width=24,
                 envmap_scale=2.0, **kw).run()
    plain, relit = [str(tmp_path / 'scene' / t / 'plots') for t in ('plain', 'relit')]
    assert sorted(os.listdir(plain)) == sorted(os.listdir(relit))
    want = load_envmap(str(tmp_path / 'sky.exr'), 12, 24) * np.float32(2.0)
    assert np.array_equal(exr.imread(os.path.join(relit, 'envmap.exr')), want)
    for f in os.listdir(relit):
        if f.startswith('rerender_rgb'):
            x = exr.imread(os.path.join(relit, f))
            assert np.isfinite(x).all() and (x >= 0).all()
