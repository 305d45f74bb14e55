"""The recomputed bounce under a map light on the GPU: nefii_envlight_bounce_sample per sample against
the numpy oracle (tests/bounce_ref.py), its mean against the exact integral, the renderer's indirect='bounce' mode
(replay, black map, linearity in the map, the default left as it was) and the render command line."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bounce_ref as br  # noqa: E402
import envlight_ref as er  # noqa: E402
import sg64  # noqa: E402

DEV = torch.device('cuda')
pytestmark = pytest.mark.gpu

# (quantile, floor, cap) of the pointwise relative error where the GGX lobe enters: tests/test_gpu_shading.py's GGX_QS
GGX_QS = ((0.5, 2e-6, 2e-3), (0.99, 2e-4, 2e-2))


def test_ggx_qs_is_the_shading_tests():
    import test_gpu_shading
    assert GGX_QS == test_gpu_shading.GGX_QS


def special_map(name):
    """the maps of tests/test_gpu_envlight.py"""
    if name == 'sun':
        m = br.lognormal_map(32, 64, 5, 0.5)
        m[9, 40] = 1e5
        return m
    if name == 'zero_rows':
        m = br.lognormal_map(16, 24, 6)
        m[[0, 5, 6, 15]] = 0.
        m[3, :12] = 0.
        return m
    if name == 'all_zero':
        return np.zeros((8, 16, 3), np.float32)
    H, W = name
    return br.lognormal_map(H, W, H * 7919 + W)


def read_table(table, H, W):
    """(M, C) as the kernel stored them (layout: csrc/nefii_envlight.hip)"""
    b = table.cpu().numpy()
    c0 = (H * 4 + 255) // 256 * 256
    M = b[:H * 4].view(np.float32).copy()
    C = b[c0:c0 + H * W * 4].view(np.float32).reshape(H, W).copy()
    return M, C


def secondary_hits(n, seed):
    """surface_points of tests/test_gpu_envlight.py with a random albedo and the bounce's 3 uniforms; u0 stays 1e-6
    away from 1/3 and 2/3 (the technique then does not hang on the last bit of 3.f * u0)"""
    g = torch.Generator().manual_seed(seed)
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    t = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    view = torch.nn.functional.normalize(nrm * (0.2 + torch.rand(n, 1, generator=g)) + t, dim=-1)
    view = torch.where((view * nrm).sum(-1, keepdim=True) > 0.05, view, nrm)
    r = 0.05 + 0.95 * torch.rand(n, 1, generator=g)
    albedo = torch.rand(n, 3, generator=g)
    uni = torch.rand(n, 3, generator=g)
    for third in (1. / 3., 2. / 3.):
        near = (uni[:, 0] - third).abs() < 1e-6
        uni[near, 0] = third + 2e-6
    return r, albedo, nrm, view, uni


# ---- 1. per sample, against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize('coord', er.COORDS)
@pytest.mark.parametrize('name', [(7, 13), (256, 512), 'sun', 'zero_rows', 'all_zero', (1, 1)], ids=str)
def test_bounce_sample_matches_the_oracle(name, coord):
    from nefii_amd import ops
    from nefii_amd.lighting import EnvmapLight
    env = special_map(name)
    H, W = env.shape[:2]
    light = EnvmapLight(torch.from_numpy(env), coord)
    n = 50000
    spec = np.array([0.04, 0.5, 0.9])
    r, albedo, nrm, view, uni = secondary_hits(n, 3)
    args = [torch.tensor(spec, dtype=torch.float32, device=DEV)] + [x.to(DEV) for x in (r, albedo, nrm, view, uni)]
    wo, weight, mix = ops.envlight_bounce_sample(light.envmap, light.table, coord, *args, want_mix=True)
    again = ops.envlight_bounce_sample(light.envmap, light.table, coord, *args, want_mix=True)
    assert all(torch.equal(a, b) for a, b in zip((wo, weight, mix), again))                 # no atomics
    wo2, weight2 = light.bounce_sample(*args)
    assert torch.equal(wo2, wo) and torch.equal(weight2, weight)
    wo, weight, mix = [x.cpu().numpy() for x in (wo, weight, mix)]
    J = sg64.Judge('bounce %s %s' % (name, coord))
    J.require('finite', bool(np.isfinite(wo).all() and np.isfinite(weight).all() and np.isfinite(mix).all()), '')
    J.require('density floor', bool((mix >= np.float32(1e-6 / (3 * np.pi)) * (1 - 1e-6)).all()), 'min %.3e' % mix.min())
    if name == 'all_zero':
        J.require('zero map', bool((weight == 0).all()), 'weight is exactly 0')
    M, C = read_table(light.table, H, W)
    n_, v_, r_, a_ = [x.double().numpy() for x in (nrm, view, r, albedo)]
    u = uni.numpy()
    k, w64, _, _, drawn = br.sample_texels(env, M, C, coord, n_, v_, r_, a_, spec, u, np.float64)
    _, w32, _, _, _ = br.sample_texels(env, M, C, coord, n_, v_, r_, a_, spec, u, np.float32)
    assert np.array_equal(k, np.minimum(np.floor(3. * u[:, 0].astype(np.float64)), 2))      # u0 is away from the thirds
    # the direction: the technique k = min((int)(3 u0), 2) drew it
    s2 = k == 2
    d2 = np.abs(wo[s2] - w64[s2]).max()
    J.require('direction 2 (map)', d2 < 2e-6, 'max |wo - oracle| %.3e over %d' % (d2, s2.sum()))
    for kk in (0, 1):
        sel = k == kk
        ok = (np.abs(wo[sel] - w64[sel]).max(-1) < 1e-4) & (np.abs(w32[sel] - w64[sel]).max(-1) < 1e-4)
        J.require('direction %d' % kk, ok.mean() > 0.998, 'agree on %d of %d' % (ok.sum(), sel.sum()))
    # density and weight at the kernel's OWN direction; the texel under a BRDF direction is not decided within 1e-5 rad of
    # an edge (the map rows carry the texel that was drawn)
    keep = s2 | (er.edge_distance(wo, H, W, coord) > 1e-5)
    J.require('texel edges', (~keep).mean() < 0.02, 'left out %d of %d' % ((~keep).sum(), n))
    m64, g64 = br.weight_at(wo, env, M, C, coord, n_, v_, r_, a_, spec, np.float64, drawn)
    m32, g32 = br.weight_at(wo, env, M, C, coord, n_, v_, r_, a_, spec, np.float32, drawn)
    t = torch.from_numpy
    J.quantiles('mix_pdf', t(mix[keep]), t(m64[keep]), t(m32[keep]), qs=GGX_QS)
    J.quantiles('weight', t(weight[keep]), t(g64[keep]), t(g32[keep]), qs=GGX_QS)
    for kk in range(3):
        sel = keep & (k == kk)
        J.quantiles('weight, technique %d' % kk, t(weight[sel]), t(g64[sel]), t(g32[sel]), qs=GGX_QS)
    J.done()


# ---- 2. the mean against the exact integral ----------------------------------------------------------------------------
DRAWS = 1 << 20
ORACLE_DRAWS = 1 << 18


def gpu_mean(light, nrm, v, rough, albedo, spec, seed):
    """mean per channel of the kernel's weight over DRAWS draws at one surface point, in double"""
    n = DRAWS
    g = torch.Generator(device=DEV).manual_seed(seed)
    uni = torch.rand(n, 3, device=DEV, generator=g)
    f = lambda x: torch.tensor(np.asarray(x), dtype=torch.float32, device=DEV)
    wo, weight = light.bounce_sample(f(spec), torch.full((n, 1), float(rough), device=DEV),
                                     f(albedo).expand(n, 3).contiguous(), f(nrm).expand(n, 3).contiguous(),
                                     f(v).expand(n, 3).contiguous(), uni)
    assert torch.isfinite(weight).all()
    return weight.double().mean(0).cpu().numpy()


@pytest.mark.parametrize('coord,k', [(c[0], c[1]) for c in br.integral_cases()], ids=lambda x: str(x))
def test_mean_matches_the_exact_integral(coord, k):
    """|mean of 2^20 kernel draws - integral| <= 5 se, se = the ORACLE estimator's standard deviation (2^18 fp64 draws
    on the CPU) / sqrt(2^20): a noisy kernel cannot widen its own bound"""
    from nefii_amd.lighting import EnvmapLight
    _, _, nrm, v, rough = [c for c in br.integral_cases() if c[0] == coord and c[1] == k][0]
    env = br.bright_texel_map()
    light = EnvmapLight(torch.from_numpy(env), coord)
    _, _, std, _ = br.estimate(env, coord, nrm, v, rough, br.ALBEDO, br.SPEC, ORACLE_DRAWS, 1000 + 16 * (coord == 'blender') + k)
    se = std / np.sqrt(DRAWS)
    s, d = er.integral(env, coord, nrm, v, rough, br.ALBEDO, br.SPEC, sub=8, fine=64)
    m = gpu_mean(light, nrm, v, rough, br.ALBEDO, br.SPEC, 300 + k)
    print('%s %d rough %.3f: mean %s integral %s deviation %s se' % (coord, k, rough, m, s + d, np.abs(m - (s + d)) / se))
    assert (np.abs(m - (s + d)) <= 5 * se).all(), (coord, k, rough, m, s + d, se)


@pytest.mark.parametrize('coord', er.COORDS)
def test_furnace_mean_is_c_times_albedo(coord):
    """On a constant map c the Lambert term integrates to c * albedo in closed form.  With the specular PARAMETER at 0 the
    Schlick term still leaves F = 2^(-(5.55473 vh + 6.8316) vh) > 0, and the kernel returns specular + diffuse in one
    number, so the (small) specular integral - quadrature on the constant map - is taken off the mean first:
    |mean - specular integral - c albedo| <= 5 se, se from the oracle estimator as above."""
    from nefii_amd.lighting import EnvmapLight
    c = np.array([0.7, 1.3, 2.0], np.float32)
    env = np.broadcast_to(c, (16, 32, 3)).copy()
    light = EnvmapLight(torch.from_numpy(env), coord)
    albedo, spec = np.array([0.8, 0.5, 0.2]), np.zeros(3)
    for k, (nrm, v, rough) in enumerate(br.cases(12, 1)):
        _, _, std, _ = br.estimate(env, coord, nrm, v, rough, albedo, spec, ORACLE_DRAWS, 2000 + k)
        se = std / np.sqrt(DRAWS)
        s, _ = er.integral(env, coord, nrm, v, rough, albedo, spec, sub=8, fine=64)
        m = gpu_mean(light, nrm, v, rough, albedo, spec, 100 + k)
        want = c * albedo
        print('%s %d rough %.3f: mean - specular %s want %s deviation %s se' % (coord, k, rough, m - s, want,
                                                                                 np.abs(m - s - want) / se))
        assert (np.abs(m - s - want) <= 5 * se).all(), (k, rough, m, s, want, se)


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


def render(model, inp, uniforms=None, bounce_uniforms=None):
    model.uniforms_override, model.bounce_uniforms_override = uniforms, bounce_uniforms
    with torch.no_grad():
        out = model(inp)
    model.uniforms_override, model.bounce_uniforms_override = None, None
    return out


class Scene:
    """the fitted bowl, a crop of it, one replayable draw of both sets of uniforms, and the share of secondary hits"""

    def __init__(self):
        from nefii_amd.model.path_tracing_render import draw_bounce_uniforms, draw_uniforms
        self.model = bowl_model()
        self.inp = crop_input(rays=4, size=24)
        out = render(self.model, self.inp)
        self.hit = out['network_object_mask']
        n = int(self.hit.sum().item())
        torch.manual_seed(3)
        self.uni = draw_uniforms(n, DEV)
        self.buni = draw_bounce_uniforms(n, DEV)
        assert self.buni.shape == (3 * n, 3)
        self.sec_share = out['secondary_mask'].float().mean().item()
        # precondition of everything below: the bowl is non-convex, its secondary rays do hit it
        assert n > 0 and self.sec_share >= 0.01, (n, self.sec_share)

    def rgb(self, light, mode=None):
        if light is None or mode is None:
            self.model.set_envmap_light(light)
        else:
            self.model.set_envmap_light(light, mode)
        return render(self.model, self.inp, self.uni, self.buni)['sg_rgb_values']


@pytest.fixture(scope='module')
def scene():
    s = Scene()
    yield s
    s.model.set_envmap_light(None)


def sky(scale=1.0):
    return torch.from_numpy(br.lognormal_map(64, 128, 4, 0.8) * np.float32(scale))


def test_renderer_replay_equals_the_composition_of_the_public_pieces(scene):
    from nefii_amd import ops
    from nefii_amd.lighting import EnvmapLight
    model, inp = scene.model, scene.inp
    light = EnvmapLight(sky(), 'mitsuba')
    a = scene.rgb(light, 'bounce')
    b = scene.rgb(light, 'bounce')
    assert torch.equal(a, b)
    print('secondary rays that hit: %.4f' % scene.sec_share)
    # --- the same picture from the pieces, in the order of DESIGN.md 6h
    with torch.no_grad():
        ctx = model.trace_head(inp)
        idx = torch.nonzero(ctx['network_object_mask']).flatten()
        assert ctx['pre'] is not None and torch.equal(ctx['network_object_mask'], scene.hit)
        p, v, nrm, feat = ops.prepare_hits(ctx['points'], ctx['ray_dirs'], ctx['pre'][2], ctx['pre'][1], idx)
        mat = model.envmap_material_network(p, feat, nrm)
        spec, r1, alb = mat['sg_specular_reflectance'], mat['sg_roughness'].reshape(-1, 1), mat['sg_diffuse_albedo']
        n = p.shape[0]
        wi, own, tab, radiance = light.sample(r1, nrm, v, scene.uni)

        def trace(origins, dirs):
            rt = model.ray_tracer
            prev, rt.miss_search = rt.miss_search, False
            try:
                pts, hit, _ = rt(sdf=model.implicit_network, cam_loc=origins,
                                 object_mask=torch.ones(origins.shape[0], dtype=torch.bool, device=DEV),
                                 ray_directions=dirs.reshape(-1, 1, 3))
            finally:
                rt.miss_search = prev
            return pts, hit

        sec_pts, sec_hit = trace(p.unsqueeze(0).expand(3, n, 3).reshape(-1, 3), wi)
        hidx = torch.nonzero(sec_hit).flatten()
        assert hidx.numel() >= 0.01 * 3 * n
        y = sec_pts[hidx]
        _, yf, g = model.implicit_network.value_feature_gradient(y)
        yn = g / (torch.norm(g, dim=-1, keepdim=True) + 1e-6)
        yv = -wi.reshape(-1, 3)[hidx]
        yv = yv / (torch.norm(yv, dim=-1, keepdim=True) + 1e-6)
        ymat = model.envmap_material_network(y, yf, yn)
        m = y.shape[0]
        wo, weight = light.bounce_sample(ymat['sg_specular_reflectance'].expand(1, 3),
                                         ymat['sg_roughness'].reshape(-1, 1).expand(m, 1), ymat['sg_diffuse_albedo'], yn,
                                         yv, scene.buni[hidx])
        _, ter_hit = trace(y, wo)
        print('tertiary rays %d, of which occluded %.4f' % (m, ter_hit.float().mean().item()))
        ind = torch.zeros(3 * n, 3, device=DEV)
        ind[hidx] = weight * (1.0 - ter_hit.float()).unsqueeze(-1)
        rgb, _, _ = ops.McShadeFn.apply(spec, r1, alb, nrm, v, wi, own, tab, radiance,
                                        (1.0 - sec_hit.float()).reshape(3, n), ind.reshape(3, n, 3))
    assert torch.equal(a[scene.hit], rgb)
    # and it is not the radiance-network picture
    assert not torch.equal(a, scene.rgb(light, 'mlp'))


def test_renderer_black_map(scene):
    """under an all-zero map nothing is lit: bounce mode is exactly black at every hit, mode mlp still glows"""
    from nefii_amd.lighting import EnvmapLight
    black = EnvmapLight(torch.zeros(8, 16, 3), 'mitsuba')
    b = scene.rgb(black, 'bounce')[scene.hit]
    assert (b == 0).all()
    a = scene.rgb(black, 'mlp')[scene.hit]
    assert (a > 0).any()                       # the defect: the training light's interreflections


def test_renderer_is_linear_in_the_map(scene):
    """2 x map (a power of two: the CDFs are bitwise equal) with the same uniforms gives exactly 2 x the picture in bounce
    mode; mode mlp does not"""
    from nefii_amd.lighting import EnvmapLight
    one, two = EnvmapLight(sky(), 'mitsuba'), EnvmapLight(sky(2.0), 'mitsuba')
    for x, y in zip(read_table(one.table, 64, 128), read_table(two.table, 64, 128)):      # (the fp64 row sums double)
        assert np.array_equal(x, y)
    a, b = scene.rgb(one, 'bounce'), scene.rgb(two, 'bounce')
    assert torch.isfinite(a).all() and (a[scene.hit] > 0).any()
    assert torch.equal(b, 2.0 * a)
    a, b = scene.rgb(one, 'mlp'), scene.rgb(two, 'mlp')
    assert not torch.equal(b[scene.hit], 2.0 * a[scene.hit])


def test_renderer_default_mode_is_unchanged(scene):
    from nefii_amd.lighting import EnvmapLight
    light = EnvmapLight(sky(), 'mitsuba')
    a = scene.rgb(light)
    b = scene.rgb(light, 'mlp')
    assert torch.equal(a, b) and scene.model.envmap_indirect == 'mlp'
    # the default mode does not draw the bounce's uniforms: the RNG stream is consumed as before
    torch.manual_seed(11)
    scene.model.set_envmap_light(light)
    x = render(scene.model, scene.inp)['sg_rgb_values']
    after_mlp = torch.rand(4, device=DEV)
    torch.manual_seed(11)
    scene.model.set_envmap_light(light, 'bounce')
    render(scene.model, scene.inp)
    after_bounce = torch.rand(4, device=DEV)
    assert not torch.equal(after_mlp, after_bounce)
    from nefii_amd.model.path_tracing_render import draw_uniforms
    torch.manual_seed(11)
    draw_uniforms(int(scene.hit.sum().item()), DEV)
    assert torch.equal(torch.rand(4, device=DEV), after_mlp) and torch.isfinite(x).all()
    # back to the model's own light: a fresh model, bitwise
    scene.rgb(light, 'bounce')
    c = scene.rgb(None)
    assert scene.model.envmap_indirect == 'mlp'
    fresh = bowl_model()
    d = render(fresh, scene.inp, scene.uni, scene.buni)['sg_rgb_values']
    assert torch.equal(c, d)


def test_bounce_mode_is_still_refused_where_a_map_light_is(scene):
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.lighting import EnvmapLight
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    light = EnvmapLight(sky(), 'mitsuba')
    model = scene.model
    model.set_envmap_light(light, 'bounce')
    model.train()
    try:
        with pytest.raises(RuntimeError):
            model(scene.inp)
    finally:
        model.eval()
        model.set_envmap_light(None)
    physg = IDRNetwork(conf.from_dict(syn.model_conf('physg', hidden=64)))
    with pytest.raises(ValueError):
        physg.set_envmap_light(light, 'bounce')
    with pytest.raises(ValueError):
        model.set_envmap_light(light, 'nonsense')


# ---- 4. the command line ---------------------------------------------------------------------------------------------
def test_render_cli_in_bounce_mode(tmp_path):
    from nefii_amd import conf, synthetic as syn
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
    exr.imwrite(str(tmp_path / 'sky.exr'), br.lognormal_map(24, 48, 8, 1.0))
    kw = dict(conf=cfg, exps_folder_name=str(tmp_path), expname='scene', timestamp='t0', checkpoint='latest',
              memory_capacity_level=10, num_rays=2, dataset_kwargs={'n_views': 2, 'img_res': (16, 16)},
              light_envmap_path=str(tmp_path / 'sky.exr'), envmap_height=12, envmap_width=24)
    RenderRunner(new_timestamp='mlp', envmap_indirect='mlp', **kw).run()
    runner = RenderRunner(new_timestamp='bounce', envmap_indirect='bounce', **kw)
    assert runner.model.envmap_indirect == 'bounce'
    runner.run()
    mlp, bounce = [str(tmp_path / 'scene' / t / 'plots') for t in ('mlp', 'bounce')]
    assert sorted(os.listdir(mlp)) == sorted(os.listdir(bounce)) and os.listdir(bounce)
    for f in os.listdir(bounce):
        if f.startswith('rerender_rgb'):
            x = exr.imread(os.path.join(bounce, f))
            assert np.isfinite(x).all() and (x >= 0).all(), f
    with pytest.raises(ValueError):
        RenderRunner(new_timestamp='nolight', envmap_indirect='bounce',
                     **{k: v for k, v in kw.items() if k != 'light_envmap_path'})
