"""Pin the CPU oracle against golden vectors produced by the reference itself
(tests/golden/make_golden.py).  CPU only; runs in the build container and on the GPU box."""
import pytest
import torch

from nefii_amd import synthetic as syn
from oracle import nets, renderer, shading, tracer


def rel_l2(a, b):
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def test_sg_math(golden):
    g = golden('sg_math')
    assert torch.allclose(shading.hemi_integral(g['lam'], g['cos_beta']), g['hemi'], rtol=1e-6, atol=1e-7)
    ax, lam, mu = shading.sg_product(g['l1'], g['lam1'], g['mu1'], g['l2'], g['lam2'], g['mu2'])
    assert torch.allclose(ax, g['out_lobe'], rtol=1e-6, atol=1e-7)
    assert torch.allclose(lam, g['out_lam'], rtol=1e-6)
    assert torch.allclose(mu, g['out_mu'], rtol=1e-6, atol=1e-9)


def test_sg_render_forward_and_grads(golden):
    g = golden('sg_render')
    albedo = g['albedo'].clone().requires_grad_(True)
    rough = g['rough'].clone().requires_grad_(True)
    spec = g['spec'].clone().requires_grad_(True)
    lgt = g['lgt'].clone().requires_grad_(True)
    out = shading.sg_closed_form(lgt, spec, rough, albedo, g['normal'], g['view'])
    for k in ('sg_rgb', 'sg_specular_rgb', 'sg_diffuse_rgb'):
        assert rel_l2(out[k], g[k]) < 1e-6, k
    ga, gr, gs, gl = torch.autograd.grad((out['sg_rgb'] * g['wts']).sum(), [albedo, rough, spec, lgt])
    assert rel_l2(ga, g['g_albedo']) < 1e-5
    assert rel_l2(gr, g['g_rough']) < 1e-4
    assert rel_l2(gs, g['g_spec']) < 1e-4
    assert rel_l2(gl, g['g_lgt']) < 1e-4


@pytest.mark.parametrize('light', ['sunrise', 'envmap1', 'adv300'])
def test_sg_render_fitted_lights_fp64(golden, light):
    """the fp64 oracle (the yardstick of tests/test_gpu_shading.py) against the reference's render_with_sg run in
    float64 on fitted lights and edge geometry (tests/golden/sg_render_fitted.npz): both are fp64, so the bound is
    rounding-order only"""
    g = golden('sg_render_fitted')
    p = {k.split('.', 1)[1]: v for k, v in g.items() if k.startswith(light + '.')}
    lgt = p['lgt'].clone().requires_grad_(True)
    rough = p['rough'].clone().requires_grad_(True)
    spec = p['spec'].clone().requires_grad_(True)
    albedo = g['albedo'].clone().requires_grad_(True)
    out = shading.sg_closed_form(lgt, spec.expand(1, 3), rough, albedo, g['normal'], g['view'])
    for k in ('sg_rgb', 'sg_specular_rgb', 'sg_diffuse_rgb'):
        assert out[k].dtype == torch.float64
        assert rel_l2(out[k], p[k]) < 1e-9, (k, rel_l2(out[k], p[k]))
    w = p['w']
    loss = (out['sg_rgb'] * w[0] + out['sg_specular_rgb'] * w[1] + out['sg_diffuse_rgb'] * w[2]).sum()
    for got, k in zip(torch.autograd.grad(loss, [albedo, rough, spec, lgt]), ('g_albedo', 'g_rough', 'g_spec', 'g_lgt')):
        assert got.shape == p[k].shape and rel_l2(got, p[k]) < 1e-9, (k, rel_l2(got, p[k]))


def test_camera_and_sphere(golden):
    g = golden('camera')
    dirs, cam = renderer.camera_rays(g['uv'], g['pose'], g['intrinsics'])
    assert torch.allclose(dirs, g['dirs'], atol=1e-7)
    assert torch.equal(cam, g['cam'])
    o = g['o'].expand(g['d'].shape[1], 3)
    t, hit = tracer.sphere_intersection(o, g['d'][0], 1.0)
    assert torch.equal(hit, g['hit'].reshape(-1))
    assert torch.allclose(t, g['t'].reshape(-1, 2), atol=2e-7)


@pytest.mark.parametrize('name,hidden', [('physg', 64), ('conf', 64), ('neus', 64), ('physg', 512), ('conf', 512)])
def test_nets(golden, name, hidden):
    g = golden('nets_%s_h%d' % (name, hidden))
    mc = syn.model_conf(name, hidden=hidden)
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    for k, v in sd.items():
        if not k.startswith('implicit'):
            v.requires_grad_(True)
    x, view = g['x'], g['view']
    y = nets.sdf_forward(sd, mc['implicit_network'], x)
    assert torch.allclose(y[:, :1], g['sdf'], atol=2e-6)
    if 'feat_sub' in g:
        assert torch.allclose(y[:, 1:][:, ::16], g['feat_sub'], atol=1e-5)
    grad = nets.sdf_gradient(sd, mc['implicit_network'], x)
    assert rel_l2(grad, g['grad']) < 1e-5
    normals = grad / (grad.norm(dim=-1, keepdim=True) + 1e-6)
    feats = y[:, 1:].detach() if mc['feature_vector_size'] > 0 else None
    rgb = nets.radiance_forward(sd, mc['rendering_network'], x, normals, view, feats)
    mat = nets.material_forward(sd, mc['envmap_material_network'], x, feats)
    assert rel_l2(rgb, g['rgb']) < 2e-5
    assert rel_l2(mat['sg_diffuse_albedo'], g['albedo']) < 2e-5
    assert rel_l2(mat['sg_roughness'], g['roughness']) < 2e-5
    assert torch.allclose(mat['sg_specular_reflectance'], g['specular'], atol=1e-7)
    loss = (rgb * g['w1']).sum() + (mat['sg_diffuse_albedo'] * g['w2']).sum()
    if mat['sg_roughness'].shape[0] == x.shape[0]:
        loss = loss + mat['sg_roughness'].sum()
    loss.backward()
    for k in g:
        if k.startswith('gnorm.'):
            p = sd[k[6:]]
            assert abs(p.grad.norm().item() - g[k].item()) <= 2e-4 * g[k].item() + 1e-7, k
        if k.startswith('grad.'):
            assert rel_l2(sd[k[5:]].grad, g[k]) < 2e-4, k


def check_trace(sdf, r, o, d, ref_hit, ref_dists):
    """hit mask identical; hit-ray depths within the per-ray/whole-batch bisection difference
    (<= 1e-6-level, oracle/__init__.py); miss rays (argmin over 100 samples of a flat minimum: the
    winner flips on rounding noise) must reach the same SDF value."""
    assert torch.equal(r['hit'], ref_hit)
    h = ref_hit
    assert (r['dists'][h] - ref_dists[h]).abs().max().item() < 5e-6
    m = ~h
    if m.any():
        a = sdf(o[m] + r['dists'][m].unsqueeze(-1) * d[m])
        b = sdf(o[m] + ref_dists[m].unsqueeze(-1) * d[m])
        assert (a - b).abs().max().item() < 2e-6
        assert ((r['dists'][m] - ref_dists[m]).abs() < 5e-6).float().mean().item() > 0.97


@pytest.mark.parametrize('tag,name,hidden,bumpy', [('smooth_h64', 'physg', 64, 0.0), ('bumpy_h64', 'physg', 64, 0.03),
                                                   ('bumpy_h512', 'physg', 512, 0.004), ('neus_h64', 'neus', 64, 0.02)])
def test_tracer(golden, tag, name, hidden, bumpy):
    g = golden('tracer_' + tag)
    mc = syn.model_conf(name, hidden=hidden)
    sd = syn.make_state_dict(mc, seed=0, bumpy=bumpy)
    sdf = lambda x: nets.sdf_forward(sd, mc['implicit_network'], x)[:, 0]
    d = g['dirs'][0]
    o = g['cam'].expand(d.shape[0], 3)
    for mode in ('eval', 'train'):
        r = tracer.trace(sdf, o, d, g['object_mask'], mc['ray_tracer'], mode == 'train', g.get('minsdf_steps'))
        check_trace(sdf, r, o, d, g[mode + '_hit'], g[mode + '_dists'])
    steps2 = g['minsdf_steps2'] if g['minsdf_steps2'].numel() else None
    r = tracer.trace(sdf, g['o2'], g['d2'], torch.ones(g['o2'].shape[0], dtype=torch.bool), mc['ray_tracer'], True, steps2)
    check_trace(sdf, r, g['o2'], g['d2'], g['sec_hit'], g['sec_dists'])


FWD_KEYS = ['points', 'idr_rgb_values', 'sg_rgb_values', 'normal_values', 'sdf_output', 'sg_diffuse_rgb_values',
            'sg_diffuse_albedo_values', 'sg_specular_rgb_values', 'sg_roughness_values',
            'sg_specular_reflection_values']


def forward_case(tag):
    """(fixture name, model conf, state dict, loss conf) of a forward_* fixture (tests/golden/make_golden.py)."""
    if tag in ('conf512', 'neus256'):       # the confs' full widths on the non-convex stand-in scene of configs 3-5
        wl = {'conf512': 'cfg3', 'neus256': 'cfg4'}[tag]
        mc, sd = syn.workload_state_dict(wl, seed=0, scene='bowl')
        return mc, sd, syn.loss_conf(syn.WORKLOADS[wl]['model'])
    mc = syn.model_conf(tag, hidden=64)
    return mc, syn.make_state_dict(mc, seed=0, bumpy=0.02), syn.loss_conf(tag)


@pytest.mark.parametrize('name,mode', [('physg', 'train'), ('physg', 'eval'), ('conf', 'train'), ('conf', 'eval'),
                                       ('neus', 'train'), ('neus', 'eval'), ('conf512', 'train'), ('neus256', 'train')])
def test_forward_and_step(golden, name, mode):
    g = golden('forward_%s_%s' % (name, mode))
    mc, sd, lc = forward_case(name)
    trainable = [k for k in sd if not k.startswith('implicit') and not (
        k.endswith('specular_reflectance') and mc['envmap_material_network'].get('fix_specular_albedo'))]
    for k in trainable:
        sd[k].requires_grad_(True)
    R = renderer.Renderer(sd, mc, training=(mode == 'train'))
    inp = {'uv': g['uv'], 'pose': g['pose'], 'intrinsics': g['intrinsics'], 'object_mask': g['in_object_mask']}
    ctx = torch.enable_grad() if mode == 'train' else torch.no_grad()
    with ctx:
        out = R.forward(inp, g.get('minsdf_steps'), g.get('uniforms'), g.get('minsdf_steps2'))
    assert torch.equal(out['network_object_mask'], g['network_object_mask'])
    assert torch.equal(out['object_mask'], g['object_mask'])
    assert torch.equal(out['_ray_hit'], g['ray_hit'])
    for k in FWD_KEYS:
        tol = 2e-3 if k in ('points', 'sdf_output') else 2e-3
        assert rel_l2(out[k], g[k]) < tol, (k, rel_l2(out[k], g[k]))
    # north_star tolerance: 1e-3 relative L2 on rendered RGB / albedo
    assert rel_l2(out['sg_rgb_values'], g['sg_rgb_values']) < 1e-3
    assert rel_l2(out['sg_diffuse_albedo_values'], g['sg_diffuse_albedo_values']) < 1e-3
    if 'secondary_points' in g:
        assert torch.equal(out['secondary_mask'], g['secondary_mask'])
        assert (out['secondary_points'] - g['secondary_points']).abs().max() < 1e-4
    if mode == 'train':
        lo = renderer.idr_loss(out, g['rgb_gt'], lc)
        for k in ('loss', 'idr_rgb_loss', 'sg_rgb_loss', 'mask_loss', 'normalsmooth_loss', 'background_rgb_loss'):
            assert abs(lo[k].item() - g['loss.' + k].item()) <= 1e-3 * abs(g['loss.' + k].item()) + 1e-6, k
        lo['loss'].backward()
        for k in g:
            if k.startswith('gnorm.') and g[k].item() > 0:
                assert abs(sd[k[6:]].grad.norm().item() - g[k].item()) <= 5e-3 * g[k].item() + 1e-7, k
            if k.startswith('grad.') and g['gnorm.' + k[5:]].item() > 0:
                assert rel_l2(sd[k[5:]].grad, g[k]) < 5e-3, k


def test_forward_with_point(golden):
    g = golden('forward_point_conf')
    mc = syn.model_conf('conf', hidden=64)
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    R = renderer.Renderer(sd, mc, training=True)
    steps2 = g['minsdf_steps2'] if g['minsdf_steps2'].numel() else None
    ret = R.shade(g['points'].reshape(-1, 3), -g['ray_dirs'].reshape(-1, 3), g['uniforms'], steps2)
    N, Rr, _ = g['points'].shape
    assert rel_l2(ret['idr_rgb'].reshape(N, Rr, 3).mean(1), g['idr_rgb_values']) < 1e-4
    assert rel_l2(ret['sg_rgb'].reshape(N, Rr, 3).mean(1), g['sg_rgb_values']) < 1e-3
