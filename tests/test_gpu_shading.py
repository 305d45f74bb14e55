"""The SG shading kernels (csrc/nefii_shading.hip) against the fp64 oracle on fitted lights, 1 to 512 lobes and edge
geometry: closed-form sg_render forward and backward, background radiance, the MIS sampler, the MC shading sum, and
one relit conf model end to end.  Bounds follow tests/sg64.py: the kernel's error against fp64 may be at most a few
times the fp32 oracle's own error there, with a floor and a hard cap."""
import os

import numpy as np
import pytest
import torch

import sg64
from nefii_amd import ops, synthetic as syn
from oracle import shading

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def fitted_lights():
    return (torch.from_numpy(np.load(os.path.join(GOLDEN, 'envfit_ref.npz'))['ref_sg']).float(),
            torch.from_numpy(np.load(os.path.join(GOLDEN, 'sg_render_fitted.npz'))['envmap1.lgt']).float())


def light(kind, M):
    sunrise, envmap1 = fitted_lights()
    if kind == 'syn':
        return sg64.synthetic_light(M)
    if kind == 'sunrise':
        return sg64.tile_light(sunrise, M)
    if kind == 'envmap1':
        return sg64.tile_light(envmap1, M)
    if kind == 'fitted':
        return sg64.tile_light(torch.cat([envmap1, sunrise]), M)
    assert kind == 'adv'
    return sg64.adversarial_light(M)


def leaf(x, dev, dtype, grad=True):
    """a fresh leaf copy (the inputs are shared by the three runs of a comparison)"""
    return x.detach().to(dev, dtype, copy=True).requires_grad_(grad)


# ---- closed-form SG render ------------------------------------------------------------------------------------------
def sg_run(dev, dtype, lgt0, spec0, rough0, alb0, nrm, view, w=None):
    """forward (w None) or forward + gradients of sum(w0 rgb + w1 spec + w2 diff)"""
    lgt, spec, rough, alb = (leaf(x, dev, dtype) for x in (lgt0, spec0, rough0, alb0))
    n, v = nrm.to(dev, dtype), view.to(dev, dtype)
    if dev == DEV:
        rgb, s, d = ops.SGRenderFn.apply(lgt, spec, rough, alb, n, v)
    else:
        o = shading.sg_closed_form(lgt, spec.expand(1, 3), rough, alb, n, v)
        rgb, s, d = o['sg_rgb'], o['sg_specular_rgb'], o['sg_diffuse_rgb']
    if w is None:
        return rgb.cpu(), s.cpu(), d.cpu()
    w = w.to(dev, dtype)
    (rgb * w[0] + s * w[1] + d * w[2]).sum().backward()
    return [x.grad.cpu() for x in (lgt, spec, rough, alb)]


SG_CASES = [  # M, light, n, specular shape, roughness
    (1, 'syn', 63, 3, 0.35), (32, 'syn', 2049, 1, 0.6), (100, 'envmap1', 513, 3, 1.0), (128, 'sunrise', 513, 3, 0.089),
    (128, 'syn', 1, 1, 0.5), (129, 'adv', 63, 3, 0.089), (255, 'fitted', 63, 1, 1.0), (256, 'adv', 513, 3, 0.35),
    (257, 'fitted', 513, 3, 0.2), (300, 'adv', 513, 1, 0.7), (512, 'adv', 513, 3, 0.089), (512, 'syn', 63, 3, 1.0)]


@pytest.mark.parametrize('M,kind,n,spec_c,rough', SG_CASES)
def test_sg_render_vs_fp64(M, kind, n, spec_c, rough):
    lgt = light(kind, M)
    nrm, view = sg64.edge_geometry(n, seed=M + n)
    g = torch.Generator().manual_seed(M * 7 + n)
    alb = torch.rand(n, 3, generator=g)
    spec = torch.tensor([[0.04, 0.5, 0.9][:spec_c]])
    r = torch.tensor([[rough]])
    w = torch.rand(3, n, 3, generator=g)
    args = (lgt, spec, r, alb, nrm, view)
    J = sg64.Judge('sg_render M=%d %s n=%d' % (M, kind, n))
    got, r64, r32 = sg_run(DEV, torch.float32, *args), sg_run('cpu', torch.float64, *args), \
        sg_run('cpu', torch.float32, *args)
    for i, name in enumerate(('rgb', 'specular', 'diffuse')):
        J.close(name, got[i], r64[i], r32[i])
    flips = sg64.gate_flips(got[1], r64[1]) | sg64.gate_flips(got[2], r64[2])
    # a sum within rounding of 0 (lobes below the horizon) may land on either side: at most a few flips more than twice
    # the fp32 oracle's own
    flips32 = (sg64.gate_flips(r32[1], r64[1]) | sg64.gate_flips(r32[2], r64[2])).sum().item()
    J.require('clamp-gate flips', flips.sum().item() <= max(2, n // 200) + 2 * flips32,
              '%d of %d (fp32 oracle %d)' % (flips.sum().item(), 3 * n, flips32))
    w = w * (~flips).float()                  # a flipped gate is judged above, not through the gradients
    got, r64, r32 = (sg_run(dev, dt, *args, w=w) for dev, dt in ((DEV, torch.float32), ('cpu', torch.float64),
                                                                  ('cpu', torch.float32)))
    names = ('g_lgt', 'g_spec', 'g_rough', 'g_albedo')
    for name, a, b, c in zip(names, got, r64, r32):
        assert a.shape == b.shape, name
        if name == 'g_lgt':
            for part, sl in (('axis', slice(0, 3)), ('lambda', slice(3, 4)), ('mu', slice(4, 7))):
                J.close('g_lgt.' + part, a[:, sl], b[:, sl], c[:, sl], floor=sg64.FLOOR_GRAD)
        else:
            J.close(name, a, b, c, floor=sg64.FLOOR_GRAD)
    zero_mu = lgt[:, 4:] == 0
    J.require('g_mu at mu == 0', bool((got[0][:, 4:][zero_mu] == 0).all()), 'sign(0) = 0: %d zeros' % zero_mu.sum())
    J.done()


# ---- background radiance --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eps', [1e-8, 1e-6])
@pytest.mark.parametrize('M,kind', [(128, 'syn'), (128, 'sunrise'), (100, 'envmap1'), (300, 'adv'), (512, 'adv')])
def test_env_radiance_vs_fp64(M, kind, eps):
    lgt0 = light(kind, M)
    d, _ = sg64.edge_geometry(999, seed=M)
    w = torch.rand(999, 3, generator=torch.Generator().manual_seed(M))
    res = {}
    for dev, dt in ((DEV, torch.float32), ('cpu', torch.float64), ('cpu', torch.float32)):
        lgt = leaf(lgt0, dev, dt)
        if dev == DEV:
            out = ops.EnvRadianceFn.apply(lgt, d.to(dev), eps)
        else:
            out = (shading.env_radiance if eps == 1e-8 else shading.light_radiance)(lgt, d.to(dev, dt))
        (out * w.to(dev, dt)).sum().backward()
        res[dev, dt] = (out.cpu(), lgt.grad.cpu())
    got, r64, r32 = res[DEV, torch.float32], res['cpu', torch.float64], res['cpu', torch.float32]
    J = sg64.Judge('env M=%d %s eps=%g' % (M, kind, eps))
    J.close('rgb', got[0], r64[0], r32[0])
    for part, sl in (('axis', slice(0, 3)), ('lambda', slice(3, 4)), ('mu', slice(4, 7))):
        J.close('g_lgt.' + part, got[1][:, sl], r64[1][:, sl], r32[1][:, sl], floor=sg64.FLOOR_GRAD)
    J.done()


# ---- MIS sampler ------------------------------------------------------------------------------------------------------
def mis_inputs(n, rough_kind, seed):
    nrm, view = sg64.edge_geometry(n, seed)
    g = torch.Generator().manual_seed(seed)
    rough = {'min': torch.full((n, 1), 0.089), 'max': torch.ones(n, 1),
             'random': 0.089 + 0.911 * torch.rand(n, 1, generator=g)}[rough_kind]
    return nrm, view, rough, torch.rand(n, 7, generator=g), g


# (quantile, floor, cap) of the pointwise relative error of a pdf.  The GGX pdf ~ 1/(c^2 + (1-c^2)/r^4)^2 loses digits
# near c = n.h = 1 at small roughness (1-c^2 from a c rounded to fp32): at r = 0.089 the fp32 oracle's own median error
# is 6e-4, so its caps are wider; the 4x-the-fp32-oracle rule still holds it tight
QS = ((0.5, 2e-6, 1e-4), (0.99, 2e-4, 2e-3))
GGX_QS = ((0.5, 2e-6, 2e-3), (0.99, 2e-4, 2e-2))


def oracle_draws(lgt, rough, nrm, view, uni, dtype):
    ws, own, table, _ = shading.draw_mis_directions(lgt.to(dtype), rough.to(dtype), nrm.to(dtype), view.to(dtype),
                                                    uni.to(dtype))
    return (torch.stack(ws), torch.stack([x.reshape(-1) for x in own]),
            torch.stack([torch.cat(table[i], dim=1) for i in range(3)]))


@pytest.mark.parametrize('M,kind,rough_kind', [(128, 'syn', 'random'), (128, 'sunrise', 'min'), (100, 'envmap1', 'max'),
                                               (300, 'adv', 'random'), (512, 'adv', 'min'), (512, 'fitted', 'max')])
def test_mis_sample_vs_fp64(M, kind, rough_kind):
    lgt = light(kind, M)
    n = 1500
    nrm, view, rough, uni, _ = mis_inputs(n, rough_kind, seed=M)
    wi, o, tab = (x.cpu() for x in ops.mis_sample(lgt.to(DEV), rough.to(DEV), nrm.to(DEV), view.to(DEV), uni.to(DEV)))
    w64, o64, t64 = oracle_draws(lgt, rough, nrm, view, uni, torch.float64)
    w32, o32, t32 = oracle_draws(lgt, rough, nrm, view, uni, torch.float32)
    J = sg64.Judge('mis M=%d %s rough=%s' % (M, kind, rough_kind))
    J.require('finite', bool(torch.isfinite(wi).all() and torch.isfinite(tab).all()), '')
    for i in range(3):
        # a uniform within rounding noise of a CDF boundary picks the neighbouring lobe (existing allowance)
        ok = ((wi[i].double() - w64[i]).abs().max(dim=-1)[0] < 1e-4) & ((w32[i].double() - w64[i]).abs().max(dim=-1)[0] < 1e-4)
        J.require('direction %d' % i, ok.float().mean().item() > 0.998, 'agree on %d of %d' % (ok.sum().item(), n))
        J.quantiles('own_pdf %d' % i, o[i][ok], o64[i][ok], o32[i][ok], qs=GGX_QS if i == 1 else QS)
        for j in range(3):
            J.quantiles('pdf[%d][%d]' % (i, j), tab[i, :, j][ok], t64[i, :, j][ok], t32[i, :, j][ok],
                        qs=GGX_QS if j == 1 else QS)
    J.done()


# ---- MC shading -------------------------------------------------------------------------------------------------------
def mc_run(dev, dtype, lgt0, spec0, rough0, alb0, nrm, view, draws, vis, ind0, w, spec_grad):
    wi, own, tab = (x.to(dev, dtype) for x in draws)
    lgt, rough, alb, ind = (leaf(x, dev, dtype) for x in (lgt0, rough0, alb0, ind0))
    spec = leaf(spec0, dev, dtype, spec_grad)
    n_, v_, vis_ = nrm.to(dev, dtype), view.to(dev, dtype), vis.to(dev, dtype)
    if dev == DEV:
        light_ = ops.EnvRadianceFn.apply(lgt, wi.reshape(-1, 3), 1e-6).reshape(3, -1, 3)
        rgb, s, d = ops.McShadeFn.apply(spec, rough, alb, n_, v_, wi, own, tab, light_, vis_, ind)
    else:
        o = shading.mc_shade(lgt, spec, rough, alb, n_, v_, list(wi), [x.reshape(-1, 1) for x in own],
                             [list(tab[i].split(1, dim=1)) for i in range(3)], [x.reshape(-1, 1) for x in vis_],
                             list(ind))
        rgb, s, d = o['sg_rgb'], o['sg_specular_rgb'], o['sg_diffuse_rgb']
    w = w.to(dev, dtype)
    (rgb * w[0] + s * w[1] + d * w[2]).sum().backward()
    grads = [lgt.grad, rough.grad, alb.grad, ind.grad] + ([spec.grad] if spec_grad else [])
    return [x.detach().cpu() for x in (rgb, s, d)], [x.cpu() for x in grads]


@pytest.mark.parametrize('M,kind,vis_kind,spec_grad', [(128, 'sunrise', 'mixed', True), (100, 'envmap1', 'one', False),
                                                       (300, 'adv', 'zero', True), (512, 'fitted', 'mixed', False)])
def test_mc_shade_vs_fp64(M, kind, vis_kind, spec_grad):
    lgt = light(kind, M)
    n = 1000
    nrm, view, rough, uni, g = mis_inputs(n, 'random', seed=M + 1)
    draws = oracle_draws(lgt, rough, nrm, view, uni, torch.float64)     # the directions and pdfs both sides shade
    draws = tuple(x.float() for x in draws)
    alb = torch.rand(n, 3, generator=g)
    vis = {'zero': torch.zeros(3, n), 'one': torch.ones(3, n),
           'mixed': (torch.rand(3, n, generator=g) < 0.5).float()}[vis_kind]
    ind = torch.rand(3, n, 3, generator=g)
    spec = torch.tensor([[0.04, 0.3, 0.9]])
    w = torch.rand(3, n, 3, generator=g)
    args = (lgt, spec, rough, alb, nrm, view, draws, vis, ind, w, spec_grad)
    (got, gg), (r64, g64), (r32, g32) = (mc_run(dev, dt, *args) for dev, dt in (
        (DEV, torch.float32), ('cpu', torch.float64), ('cpu', torch.float32)))
    J = sg64.Judge('mc M=%d %s vis=%s spec_grad=%s' % (M, kind, vis_kind, spec_grad))
    for name, a, b, c in zip(('rgb', 'specular', 'diffuse'), got, r64, r32):
        J.close(name, a, b, c)
    flips = sg64.gate_flips(got[1], r64[1]) | sg64.gate_flips(got[2], r64[2])
    J.require('clamp-gate flips', flips.sum().item() <= 2, '%d of %d' % (flips.sum().item(), 3 * n))
    names = ['g_lgt', 'g_rough', 'g_albedo', 'g_indirect'] + (['g_spec'] if spec_grad else [])
    for name, a, b, c in zip(names, gg, g64, g32):
        assert a.shape == b.shape, name
        if name == 'g_rough':      # d/d roughness runs through the ill-conditioned GGX term
            J.quantiles(name, a, b, c, qs=((0.5, 2e-6, 1e-4), (0.99, 2e-4, 5e-3)))
        elif name == 'g_indirect' and vis_kind == 'one':
            J.require(name, bool((a == 0).all()), 'all zero where every sample is visible')
        else:
            J.close(name, a, b, c, floor=sg64.FLOOR_GRAD)
    J.done()


# ---- lobe-count limit -------------------------------------------------------------------------------------------------
def test_more_than_512_lobes_is_a_value_error():
    lgt = torch.rand(513, 7, device=DEV)
    n = torch.tensor([[0., 0., 1.]], device=DEV)
    with pytest.raises(ValueError, match='512'):
        ops.SGRenderFn.apply(lgt, torch.rand(1, 3, device=DEV), torch.rand(1, 1, device=DEV), n, n, n)
    with pytest.raises(ValueError, match='512'):
        ops.mis_sample(lgt, torch.rand(1, device=DEV), n, n, torch.rand(1, 7, device=DEV))
    with pytest.raises(ValueError, match='512'):
        ops.EnvRadianceFn.apply(lgt, n, 1e-8)


# ---- a relit conf model end to end ------------------------------------------------------------------------------------
def _relit_forward(mc, sd, light_path=None, ref_light=None):
    from nefii_amd import conf
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    from oracle import renderer as orr
    from parity import compare_outputs
    inp, _ = syn.make_inputs(128, (64, 64), 100.0, (0.2, 0.1, 2.0), 2, seed=8)
    g = torch.Generator().manual_seed(5)
    steps1, steps2 = torch.rand(100, generator=g), torch.rand(100, generator=g)
    sdo = {k: v.clone() for k, v in sd.items()}
    if ref_light is not None:
        sdo['envmap_material_network.lgtSGs'] = ref_light.clone()
    R = orr.Renderer(sdo, mc, training=True)
    R.dead_work = False
    with torch.no_grad():
        uniforms = R.forward(inp, steps1, None, steps2)['_uniforms']
        ref = R.forward(inp, steps1, uniforms, steps2)
    m = IDRNetwork(conf.from_dict(mc))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m.freeze_geometry()
    m.train(True)
    if light_path is not None:
        m.envmap_material_network.load_light(light_path)
    m.ray_tracer.minsdf_steps_override = [steps1, steps2]
    m.uniforms_override = uniforms
    with torch.no_grad():
        out = m({k: v.to(DEV) for k, v in inp.items()})
    compare_outputs(out, ref, max_flips=2, what='relit conf', rays_per_pixel=2, ray_hit=m.last_ray_hit,
                    ref_ray_hit=ref['_ray_hit'], max_explained_frac=0.10)
    assert ref['network_object_mask'].sum().item() > 60


def test_relit_conf_model_with_300_lobes_through_the_mc_path():
    mc = syn.model_conf('conf', hidden=64)
    mc['envmap_material_network']['num_lgt_sgs'] = 300
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    sd['envmap_material_network.lgtSGs'] = sg64.tile_light(torch.cat(fitted_lights()[::-1]), 300)
    _relit_forward(mc, sd)


def test_relit_conf_model_with_the_fitted_100_lobe_light_through_load_light(tmp_path):
    mc = syn.model_conf('conf', hidden=64)
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    lgt = fitted_lights()[1]
    path = str(tmp_path / 'sg_100.npy')
    np.save(path, lgt.numpy())
    _relit_forward(mc, sd, light_path=path, ref_light=lgt)
