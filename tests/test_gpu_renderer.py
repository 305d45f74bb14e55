"""GPU parity tests, renderer level: IDRNetwork.forward (+ loss + backward) through the HIP path against
(1) the reference-generated golden vectors and (2) the CPU oracle on BASELINE.json's configs.

north_star tolerance: relative L2 <= 1e-3 on rendered RGB (sg_rgb_values) and albedo
(sg_diffuse_albedo_values) on identical rays."""
import numpy as np
import pytest
import torch

from nefii_amd import conf, ops, synthetic as syn
from oracle import nets, renderer as orr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

from parity import FLOAT_KEYS, compare_outputs, rel_l2  # noqa: E402  (tests/parity.py)


def build_model(mc, sd, training=True):
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    m = IDRNetwork(conf.from_dict(mc))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    m.freeze_geometry()
    m.train(training)
    return m


def to_dev(inp):
    return {k: v.to(DEV) for k, v in inp.items()}


@pytest.mark.parametrize('mode', ['train', 'eval'])
def test_forward_physg_golden(golden, mode):
    g = golden('forward_physg_' + mode)
    mc = syn.model_conf('physg', hidden=64)
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    m = build_model(mc, sd, mode == 'train')
    if 'minsdf_steps' in g:
        m.ray_tracer.minsdf_steps_override = g['minsdf_steps']
    inp = to_dev({'uv': g['uv'], 'pose': g['pose'], 'intrinsics': g['intrinsics'], 'object_mask': g['in_object_mask']})
    ctx = torch.enable_grad() if mode == 'train' else torch.no_grad()
    with ctx:
        out = m(inp)
    compare_outputs(out, g, what=mode)
    if mode == 'train':
        from nefii_amd.model.loss import IDRLoss
        lo = IDRLoss(**syn.loss_conf('physg'))(out, {'rgb': g['rgb_gt'].to(DEV)})
        for k in ('loss', 'sg_rgb_loss', 'mask_loss', 'normalsmooth_loss'):
            assert abs(lo[k].item() - g['loss.' + k].item()) <= 2e-3 * abs(g['loss.' + k].item()) + 1e-6, k
        lo['loss'].backward()
        for name, p in m.named_parameters():
            key = 'gnorm.' + name
            if key in g and g[key].item() > 0:
                assert p.grad is not None, name
                assert abs(p.grad.norm().item() - g[key].item()) <= 1e-2 * g[key].item() + 1e-7, name
            if 'grad.' + name in g and g[key].item() > 0:
                assert rel_l2(p.grad, g['grad.' + name]) < 1e-2, name


def oracle_step(mc, sd, inp, gt, lc, steps):
    sdo = {k: v.clone() for k, v in sd.items()}
    for k in sdo:
        if not k.startswith('implicit'):
            sdo[k].requires_grad_(True)
    R = orr.Renderer(sdo, mc, training=True)
    out = R.forward(inp, steps)
    lo = orr.idr_loss(out, gt, lc)
    lo['loss'].backward()
    return out, lo, sdo, R


@pytest.mark.parametrize('wl', ['cfg1'])
def test_train_step_full_size_vs_oracle(wl):
    """BASELINE.json config 1 at full network size: forward + loss + backward against the CPU oracle."""
    w = syn.WORKLOADS[wl]
    mc = syn.model_conf(w['model'])
    sd = syn.make_state_dict(mc, seed=0)
    lc = syn.loss_conf(w['model'])
    inp, gt = syn.make_inputs(w['num_pixels'], w['image_hw'], w['focal'], w['cam_pos'], w['num_rays'], seed=1)
    steps = torch.rand(100, generator=torch.Generator().manual_seed(3))
    ref, rlo, sdo, R = oracle_step(mc, sd, inp, gt, lc, steps)
    m = build_model(mc, sd, True)
    m.ray_tracer.minsdf_steps_override = steps
    m.ray_tracer.collect_counters = True
    out = m(to_dev(inp))
    compare_outputs(out, ref, max_flips=2, what=wl)
    from nefii_amd.model.loss import IDRLoss
    lo = IDRLoss(**lc)(out, {'rgb': gt.to(DEV)})
    assert abs(lo['loss'].item() - rlo['loss'].item()) <= 2e-3 * abs(rlo['loss'].item())
    lo['loss'].backward()
    for name, p in m.named_parameters():
        if sdo[name].grad is not None and sdo[name].grad.norm() > 0:
            assert rel_l2(p.grad, sdo[name].grad) < 2e-2, (name, rel_l2(p.grad, sdo[name].grad))
    # the tracer's query counters equal the oracle's SDF evaluation counts (exact algorithmic work, no padding)
    cnt = m.ray_tracer.last_counters.cpu().long()
    gpu_evals = ops.algorithmic_evals(cnt, 100).sum().item()     # algorithmic (header: counters)
    c = R.counters
    cpu_evals = sum(c.get(k, 0) for k in ('sphere_trace', 'sampler', 'bisect', 'min_sdf'))
    assert abs(gpu_evals - cpu_evals) <= 0.01 * cpu_evals, (gpu_evals, cpu_evals)


@pytest.mark.parametrize('hidden,npix,multi', [(64, 512, -1), (64, 64, 4)])
def test_graph_step_matches_eager_step(hidden, npix, multi):
    """TrainStep(graph=True): the captured tail (shading of the padded hit list, IDRLoss, backward, both Adam updates)
    gives the eager step's losses and parameter trajectory; different inputs per iteration change the hit count and
    so the padded size / the graph that replays."""
    from nefii_amd.training.step import TrainStep
    mc = syn.model_conf('physg', hidden=hidden)
    mc['render_background'] = True
    sd = syn.make_state_dict(mc, seed=4, bumpy=0.02)
    lc = syn.loss_conf('physg')
    lc['idr_rgb_weight'] = 1.0
    batches = []
    for it in range(7):
        inp, gt = syn.make_inputs(npix, (64, 64), 100.0 + 7 * it, (0.2, 0.1, 2.0 + 0.05 * it), multi, seed=20 + it)
        batches.append((to_dev(inp), {'rgb': gt.to(DEV)}))
    runs = []
    for graph in (False, True):
        m = build_model(mc, sd, True)
        m.ray_tracer.minsdf_steps_override = [torch.rand(100, generator=torch.Generator().manual_seed(3)) for _ in range(99)]
        st = TrainStep(m, lc, graph=graph, graph_bucket=64, graph_after=2)
        losses = []
        for inp, gt in batches:
            out, lo = st(inp, gt)
            losses.append({k: v.item() for k, v in lo.items()})
        runs.append((losses, {k: v.detach().clone() for k, v in m.state_dict().items()}, st))
    (l0, p0, _), (l1, p1, st1) = runs
    assert len(st1._graphs) >= 2          # the hit count did change the padded size
    for a, b in zip(l0, l1):
        for k in a:
            assert abs(a[k] - b[k]) <= 1e-4 * max(abs(a[k]), 1e-3), (k, a[k], b[k])
    for k in p0:
        if p0[k].dtype.is_floating_point:
            assert rel_l2(p1[k], p0[k]) < 1e-4, (k, rel_l2(p1[k], p0[k]))


def test_state_dict_roundtrip_and_eval_mode():
    mc = syn.model_conf('physg', hidden=64)
    sd = syn.make_state_dict(mc, seed=5, bumpy=0.02)
    m = build_model(mc, sd, False)
    sd2 = m.state_dict()
    assert set(sd2.keys()) == set(sd.keys())
    for k in sd:
        assert torch.equal(sd2[k].cpu(), sd[k]), k
    inp, _ = syn.make_inputs(64, (64, 64), 100.0, (0.2, 0.1, 2.0), -1, seed=2)
    with torch.no_grad():
        o1 = m(to_dev(inp))
        o2 = m(to_dev(inp))
    for k in FLOAT_KEYS:
        assert torch.equal(o1[k], o2[k]), k      # deterministic (no atomics on the forward path)


@pytest.mark.parametrize('tag', ['physg', 'physg_multi', 'conf_mc'])
def test_trainable_geometry_golden(golden, tag):
    """geometry NOT frozen (implicit_differentiable_renderer.py:357-393, SampleNetwork,
    eikonal points, grad_theta) - HIP camera rays and tracer in front of the torch slow path
    (model/trainable_geometry.py) - against the reference-generated fixture: outputs, every loss term incl. the eikonal
    one, and the gradient of every parameter, the SDF network's included; then one TrainStep moves the SDF weights."""
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    from nefii_amd.model.loss import IDRLoss
    from nefii_amd.training.step import TrainStep
    g = golden('forward_trainable_' + tag)
    mcs = tag == 'conf_mc'        # the Monte-Carlo render type (pt_render_indirect_mlp) on the same branch, round 3
    name = 'conf' if mcs else 'physg'
    mc = syn.model_conf(name, hidden=64)
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    m = IDRNetwork(conf.from_dict(mc))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV).train()
    zeros = torch.zeros(100)
    m.ray_tracer.minsdf_steps_override = [g.get('minsdf_steps', zeros), g.get('minsdf_steps2', zeros)] if mcs else g['minsdf_steps']
    m.eikonal_points_override = g['eikonal_points']
    inp = to_dev({'uv': g['uv'], 'pose': g['pose'], 'intrinsics': g['intrinsics'], 'object_mask': g['in_object_mask']})
    if mcs:
        m.uniforms_override = g['uniforms'].to(DEV)
    out = m(inp)
    flips = (out['network_object_mask'].cpu() != g['network_object_mask']).sum().item()
    assert flips <= 1, flips
    agree = out['network_object_mask'].cpu() == g['network_object_mask']
    hit = g['network_object_mask'] & agree
    mc_keys = ('sg_rgb_values', 'sg_diffuse_rgb_values', 'sg_specular_rgb_values')
    if mcs:
        # pixels containing a ray whose sampled direction or secondary hit flag differs DISCRETELY from the reference's
        # (tests/parity.py: a lobe pick at a CDF boundary, a grazing re-hit) are compared apart - counted and bounded
        assert torch.equal(m.last_ray_hit.cpu(), g['ray_hit'])
        from parity import mc_flagged_rays
        R = g['uv'].shape[2] if g['uv'].dim() == 4 else 1
        obj_ray = g['in_object_mask'].reshape(-1, 1).expand(-1, R).reshape(-1)      # the rays that are SHADED: hit & inside the mask
        flagged, n_dir, n_vis = mc_flagged_rays(out, g, m.last_ray_hit.cpu() & obj_ray, g['ray_hit'] & obj_ray)
        flagged_px = flagged.reshape(-1, R).any(1)
        print('[trainable conf_mc] rays with a differing direction %d / secondary hit flag %d' % (n_dir, n_vis))
        assert flagged_px.float().mean().item() <= 0.1
        assert (out['secondary_mask'].cpu() != g['secondary_mask']).float().mean().item() < 0.02
    for k in FLOAT_KEYS:
        a, b = out[k].detach().cpu(), g[k]
        sel = hit if k in ('points', 'sdf_output') else agree
        if mcs and k in mc_keys:
            sel = sel & ~flagged_px
        tol = 2e-4 if k == 'points' else (5e-2 if k == 'sdf_output' else 1e-3)
        if mcs and k == 'sg_specular_rgb_values':
            tol = 1e-2                      # a component of the colour: see tests/parity.py
        if k == 'sdf_output':
            assert (a[sel] - b[sel]).abs().max().item() < 2e-4
        else:
            assert rel_l2(a[sel], b[sel]) < tol, (tag, k, rel_l2(a[sel], b[sel]))
    n_eik = g['eikonal_points'].shape[0]
    assert rel_l2(out['grad_theta'][:n_eik], g['grad_theta'][:n_eik]) < 1e-4
    lc = syn.loss_conf(name)
    lc['idr_rgb_weight'] = 1.0
    lo = IDRLoss(**lc)(out, {'rgb': g['rgb_gt'].to(DEV)})
    ltol = 5e-3
    for k in ('loss', 'idr_rgb_loss', 'sg_rgb_loss', 'eikonal_loss', 'mask_loss', 'normalsmooth_loss'):
        assert abs(lo[k].item() - g['loss.' + k].item()) <= ltol * abs(g['loss.' + k].item()) + 1e-6, k
    lo['loss'].backward()
    sdf_grads = 0
    gtol = 3e-2
    for pname, p in m.named_parameters():
        key = 'gnorm.' + pname
        if key in g and g[key].item() > 0:
            assert p.grad is not None, pname
            assert abs(p.grad.norm().item() - g[key].item()) <= gtol * g[key].item() + 1e-7, pname
            if 'grad.' + pname in g:
                assert rel_l2(p.grad, g['grad.' + pname]) < gtol, (pname, rel_l2(p.grad, g['grad.' + pname]))
            sdf_grads += pname.startswith('implicit_network')
    assert sdf_grads >= 20
    m.uniforms_override = None
    # the whole step with trainable geometry: the SDF network is in the idr optimizer (idr_train.py:188-191) and moves
    before = {k: v.detach().clone() for k, v in m.implicit_network.state_dict().items()}
    st = TrainStep(m, lc)
    _, lo2 = st(inp, {'rgb': g['rgb_gt'].to(DEV)})
    assert all(torch.isfinite(v).all() for v in m.state_dict().values() if v.dtype.is_floating_point)
    assert any(not torch.equal(before[k], v) for k, v in m.implicit_network.state_dict().items())


@pytest.mark.parametrize('name,mode', [('conf', 'train'), ('conf', 'eval'), ('neus', 'train'), ('neus', 'eval'),
                                       ('conf512', 'train'), ('neus256', 'train')])
def test_forward_indirect_golden(golden, name, mode):
    """conf.conf / conf_neus.conf models: MIS sampling + secondary trace + indirect radiance + MC shading,
    replaying the reference's captured random draws.  conf512 / neus256: the confs' FULL network widths on the
    non-convex stand-in scene of configs 3-5 through the workload's camera (59 % of the secondary rays re-hit) - the
    512- / 256-wide kernels against the reference itself, not only against the oracle."""
    g = golden('forward_%s_%s' % (name, mode))
    if name in ('conf512', 'neus256'):
        wl = {'conf512': 'cfg3', 'neus256': 'cfg4'}[name]
        mc, sd = syn.workload_state_dict(wl, seed=0, scene='bowl')      # the embedding the fixture was generated with
        lc = syn.loss_conf(syn.WORKLOADS[wl]['model'])
    else:
        mc = syn.model_conf(name, hidden=64)
        sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
        lc = syn.loss_conf(name)
    m = build_model(mc, sd, mode == 'train')
    d = torch.rand(100)
    m.ray_tracer.minsdf_steps_override = [g.get('minsdf_steps', d), g.get('minsdf_steps2', d)]
    m.uniforms_override = g['uniforms']
    inp = to_dev({'uv': g['uv'], 'pose': g['pose'], 'intrinsics': g['intrinsics'], 'object_mask': g['in_object_mask']})
    ctx = torch.enable_grad() if mode == 'train' else torch.no_grad()
    with ctx:
        out = m(inp)
    nr = g['uv'].shape[2] if g['uv'].dim() == 4 else 1
    compare_outputs(out, g, what='%s-%s golden' % (name, mode), rays_per_pixel=nr, ray_hit=m.last_ray_hit,
                    ref_ray_hit=g['ray_hit'], max_explained_frac=0.10)
    sm, rsm = out['secondary_mask'].cpu(), g['secondary_mask']
    assert (sm != rsm).float().mean().item() < 0.01
    if mode == 'train':
        from nefii_amd.model.loss import IDRLoss
        lo = IDRLoss(**lc)(out, {'rgb': g['rgb_gt'].to(DEV)})
        for k in ('loss', 'idr_rgb_loss', 'sg_rgb_loss', 'mask_loss', 'normalsmooth_loss', 'background_rgb_loss'):
            assert abs(lo[k].item() - g['loss.' + k].item()) <= 3e-3 * abs(g['loss.' + k].item()) + 1e-6, k
        lo['loss'].backward()
        for pname, p in m.named_parameters():
            key = 'gnorm.' + pname
            if key in g and g[key].item() > 0:
                assert p.grad is not None, pname
                assert abs(p.grad.norm().item() - g[key].item()) <= 2e-2 * g[key].item() + 1e-7, pname
            if 'grad.' + pname in g and g[key].item() > 0:
                assert rel_l2(p.grad, g['grad.' + pname]) < 2e-2, pname


def test_forward_with_point_golden(golden):
    g = golden('forward_point_conf')
    mc = syn.model_conf('conf', hidden=64)
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    m = build_model(mc, sd, True)
    m.uniforms_override = g['uniforms']
    m.ray_tracer.minsdf_steps_override = g['minsdf_steps2'] if g['minsdf_steps2'].numel() else torch.rand(100)
    out = m({'points': g['points'].to(DEV), 'ray_dirs': g['ray_dirs'].to(DEV)}, with_point=True)
    assert rel_l2(out['idr_rgb_values'], g['idr_rgb_values']) < 1e-4
    assert rel_l2(out['sg_rgb_values'], g['sg_rgb_values']) < 1e-3


def test_forward_full_size_conf_vs_oracle():
    """conf.conf at full network size (8x512 SDF with feature vector, 8x512 material, 4x512 radiance), multi-ray
    pixels, MC direct + indirect with injected draws, bumpy geometry so that secondary rays do hit."""
    mc = syn.model_conf('conf')
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.004)
    inp, gt = syn.make_inputs(64, (64, 64), 100.0, (0.2, 0.1, 2.0), 4, seed=8)
    g = torch.Generator().manual_seed(5)
    steps1, steps2 = torch.rand(100, generator=g), torch.rand(100, generator=g)
    sdo = {k: v.clone() for k, v in sd.items()}
    R = orr.Renderer(sdo, mc, training=True)
    R.dead_work = False
    with torch.no_grad():
        # first pass only to learn how many hit points there are (uniforms are per hit point)
        probe = R.forward(inp, steps1, None, steps2)
    uniforms = probe['_uniforms']
    with torch.no_grad():
        ref = R.forward(inp, steps1, uniforms, steps2)
    m = build_model(mc, sd, True)
    m.ray_tracer.minsdf_steps_override = [steps1, steps2]
    m.uniforms_override = uniforms
    with torch.no_grad():
        out = m(to_dev(inp))
    compare_outputs(out, ref, max_flips=2, what='conf512 bumpy', rays_per_pixel=4, ray_hit=m.last_ray_hit,
                    ref_ray_hit=ref['_ray_hit'], max_explained_frac=0.10)
    assert (out['secondary_mask'].cpu() != ref['secondary_mask']).float().mean().item() < 0.01
    assert ref['secondary_mask'].float().mean().item() > 0.01      # the indirect branch is exercised


def test_render_frame_chunks_match_direct_forward():
    """H2 counterpart (render.py:267-360): chunked eval-mode rendering of a small frame, merged, equals the
    un-chunked forward; multi-ray pixels; chunk size chosen so that the last chunk is ragged."""
    from nefii_amd.training import render as R
    mc = syn.model_conf('conf', hidden=64)
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    m = build_model(mc, sd, False)
    H = W = 12
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    uv = torch.stack([xs, ys], -1).reshape(1, -1, 1, 2).float() * 5.0 + 2.0
    g = torch.Generator().manual_seed(1)
    uv = uv + torch.rand(1, 1, 3, 2, generator=g) - 0.5           # 3 rays per pixel, shared jitter
    inp, _ = syn.make_inputs(16, (64, 64), 100.0, (0.2, 0.1, 2.0), -1, seed=2)
    full = to_dev({'uv': uv, 'object_mask': torch.ones(1, H * W, dtype=torch.bool), 'pose': inp['pose'],
                   'intrinsics': inp['intrinsics']})
    n_hit_points = None
    with torch.no_grad():
        direct = m(full)
    # the MC sampler draws per hit point: replay the same uniforms per chunk by seeding identically is not
    # possible across different chunkings, so compare the deterministic outputs and the hit mask
    merged = R.render_frame(m, full, H * W, num_rays=3, memory_capacity_level=7)     # 128 // 3 = 42 px per chunk
    assert merged['points'].shape == (H * W, 3)
    assert torch.equal(merged['network_object_mask'], direct['network_object_mask'])
    for k in ('points', 'normal_values', 'sg_diffuse_albedo_values', 'sg_roughness_values', 'idr_rgb_values'):
        assert rel_l2(merged[k], direct[k]) < 1e-5, k


def test_batch_of_two_cameras_and_no_hits():
    """B = 2 poses in one call (rays of both images share the kernels) and a camera that looks away from the
    object (no sphere hit at all: every output keeps its default, the shading kernels see n = 0)."""
    mc = syn.model_conf('physg', hidden=64)
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    a, _ = syn.make_inputs(64, (64, 64), 100.0, (0.2, 0.1, 2.0), -1, seed=2)
    b, _ = syn.make_inputs(64, (64, 64), 100.0, (-1.5, 0.8, 1.6), -1, seed=3)
    both = {k: torch.cat([a[k], b[k]], 0) for k in a}
    steps = torch.rand(100, generator=torch.Generator().manual_seed(0))
    m = build_model(mc, sd, True)
    m.ray_tracer.minsdf_steps_override = steps
    with torch.no_grad():
        out = m(to_dev(both))
    ref = orr.Renderer({k: v.clone() for k, v in sd.items()}, mc, training=True).forward(both, steps)
    compare_outputs(out, ref, max_flips=1, what='B=2')
    # camera far outside, looking away: no ray reaches the unit sphere
    away = dict(a)
    pose = a['pose'].clone()
    pose[0, :3, 3] = torch.tensor([0., 0., 5.0])
    pose[0, :3, 2] = torch.tensor([0., 0., 1.0])
    away['pose'] = pose
    with torch.no_grad():
        out = m(to_dev(away))
    ref = orr.Renderer({k: v.clone() for k, v in sd.items()}, mc, training=True).forward(away, steps)
    assert not out['network_object_mask'].any() and not ref['network_object_mask'].any()
    assert torch.equal(out['sg_rgb_values'].cpu(), torch.ones(64, 3))
    assert (out['points'].cpu() - ref['points']).abs().max().item() < 1e-5
    m.eval()
    with torch.no_grad():
        out = m(to_dev(away))
    # (rays whose LINE meets the sphere behind the camera still count as sphere hits with both depths clamped to
    # 0.01 - rend_util.py:218 - and march one step; the others return the camera centre)
    ref = orr.Renderer({k: v.clone() for k, v in sd.items()}, mc, training=False).forward(away, None)
    assert (out['points'].cpu() - ref['points']).abs().max().item() < 1e-5
    assert not out['network_object_mask'].any()


def test_skip_min_sdf_search_keeps_gradients():
    """RayTracing.skip_min_sdf_search: dropping the training-mode min-SDF search under frozen geometry changes `points`
    / `sdf_output` of miss rays and the value of mask_loss, and nothing that carries gradient."""
    from nefii_amd.model.loss import IDRLoss
    mc = syn.model_conf('physg', hidden=64)
    sd = syn.make_state_dict(mc, seed=6, bumpy=0.02)
    lc = syn.loss_conf('physg')
    lc['idr_rgb_weight'] = 1.0
    inp, gt = syn.make_inputs(512, (64, 64), 100.0, (0.2, 0.1, 2.0), -1, seed=2)
    res = []
    for skip in (False, True):
        m = build_model(mc, sd, True)
        m.ray_tracer.skip_min_sdf_search = skip
        out = m(to_dev(inp))
        lo = IDRLoss(**lc)(out, {'rgb': gt.to(DEV)})
        lo['loss'].backward()
        res.append((out, lo, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}))
    (o0, l0, g0), (o1, l1, g1) = res
    assert torch.equal(o0['network_object_mask'], o1['network_object_mask'])
    for k in ('sg_rgb_values', 'idr_rgb_values', 'normal_values', 'sg_diffuse_albedo_values'):
        assert torch.equal(o0[k], o1[k]), k
    hit = o0['network_object_mask']
    assert torch.equal(o0['points'][hit], o1['points'][hit])
    assert not torch.equal(o0['points'][~hit], o1['points'][~hit])
    for k in ('sg_rgb_loss', 'idr_rgb_loss'):
        assert l0[k].item() == l1[k].item()
    assert set(g0) == set(g1)
    for n in g0:
        assert rel_l2(g1[n], g0[n]) < 1e-5, n


def _runner_conf(tmp, n_pix=256):
    from nefii_amd import conf
    mc = syn.model_conf('physg', hidden=64)
    lc = syn.loss_conf('physg')
    return conf.from_dict({
        'train': {'model_class': 'nefii_amd.model.implicit_differentiable_renderer.IDRNetwork',
                  'loss_class': 'nefii_amd.model.loss.IDRLoss',
                  'dataset_class': 'nefii_amd.datasets.synthetic_dataset.SyntheticSceneDataset',
                  'idr_learning_rate': 5e-4, 'sg_learning_rate': 5e-4, 'num_pixels': n_pix,
                  'idr_sched_milestones': [4, 8], 'idr_sched_factor': 0.5, 'sg_sched_milestones': [6],
                  'sg_sched_factor': 0.5, 'alpha_milestones': [5], 'alpha_factor': 2.0, 'ckpt_freq': 8},
        'loss': lc, 'model': mc})


@pytest.mark.parametrize('graph', [False, True])
def test_runner_checkpoint_layout_and_resume(tmp_path, graph):
    """IDRTrainRunner: the reference's experiment/checkpoint layout (idr_train.py:67-115,329-372); a run that stops at
    a checkpoint and continues from it reproduces the uninterrupted run's parameters."""
    import os
    from nefii_amd.training.idr_train import IDRTrainRunner, SUBDIRS
    cfg = _runner_conf(tmp_path)
    kw = dict(conf=cfg, exps_folder_name=str(tmp_path), freeze_geometry=True, nepochs=1000, graph=graph,
              dataset_kwargs={'n_views': 8, 'img_res': (48, 48)}, log_freq=4)
    sd = syn.make_state_dict(cfg.get_config('model'), seed=4, bumpy=0.02)

    def make(**extra):
        torch.manual_seed(0)
        r = IDRTrainRunner(**dict(kw, **extra))
        if not extra.get('is_continue'):
            r.model.load_state_dict(sd)
            r.model.freeze_geometry()
        r.model.ray_tracer.minsdf_steps_override = torch.rand(100, generator=torch.Generator().manual_seed(3))
        return r

    full = make(expname='full', max_niters=15, new_timestamp='t0')
    full.run()
    assert full.step.cur_iter == 16
    # the tensorboard event file where the reference's SummaryWriter puts it (idr_train.py:114-115), scalars at the logging points
    from nefii_amd.utils import tb_writer
    run_dir = os.path.join(str(tmp_path), 'full', 't0')
    ev_files = [f for f in os.listdir(run_dir) if f.startswith('events.out.tfevents.')]
    assert len(ev_files) == 1
    full.writer.close()
    ev = tb_writer.read_events(os.path.join(run_dir, ev_files[0]))
    logged = {(e['tag'], e['step']) for e in ev if 'value' in e}
    assert {('loss', 0), ('sg_psnr', 4), ('mask_loss', 8), ('idr_lr', 12), ('alpha', 12)} <= logged, sorted(logged)[:12]
    assert all(s_ % 4 == 0 for _, s_ in logged)
    part = make(expname='part', max_niters=7, new_timestamp='t0')
    part.run()                                            # epoch 0 = iterations 0..7; the epoch-1 checkpoint follows
    ck = os.path.join(str(tmp_path), 'part', 't0', 'checkpoints')
    for sub in SUBDIRS.values():
        assert sorted(os.listdir(os.path.join(ck, sub))) == ['0.pth', '1.pth', 'latest.pth'], sub
    d = torch.load(os.path.join(ck, 'ModelParameters', 'latest.pth'))
    # the reference's payload keys (idr_train.py:334-337: what its loader reads) plus this build's record of the run's tracer arithmetic
    assert set(d) == {'epoch', 'model_state_dict', 'trace_tier'} and d['epoch'] == 1 and d['trace_tier'] is False
    assert set(d['model_state_dict']) == set(sd)
    o = torch.load(os.path.join(ck, 'IDROptimizerParameters', 'latest.pth'))
    assert set(o) == {'epoch', 'optimizer_state_dict'} and isinstance(o['optimizer_state_dict']['param_groups'][0]['lr'], float)
    cont = make(expname='part', max_niters=15, is_continue=True, timestamp='latest', new_timestamp='t1')
    assert cont.start_epoch == 1 and cont.step.cur_iter == 8
    assert cont.step.loss.alpha == full.step.loss.alpha          # the alpha milestone at 5 was re-applied
    cont.run()
    assert cont.step.cur_iter == 16
    a, b = full.model.state_dict(), cont.model.state_dict()
    # eager: the continued run repeats the uninterrupted one operation for operation.  graph: its first three iterations
    # run eagerly where the uninterrupted run replayed graphs - summation-order differences that Adam (|update| = lr
    # whatever the gradient's size) turns into a few lr-sized steps on near-zero-gradient entries.
    tol = 1e-2 if graph else 2e-4
    for k in a:
        if a[k].dtype.is_floating_point:
            assert rel_l2(b[k], a[k]) < tol, (k, rel_l2(b[k], a[k]))
    assert abs(float(cont.step.idr_optimizer.param_groups[0]["lr"]) - 5e-4 * 0.25) < 1e-9      # fp32 tensor in graph mode
    if not graph:
        # a checkpoint written by an EAGER run (python-float lr, capturable=False, CPU step counters - what a reference
        # checkpoint looks like) continued in GRAPH mode: the captured Adam needs capturable state (TrainStep.retensor_lr)
        g = make(expname='part', max_niters=15, is_continue=True, timestamp='t0', new_timestamp='t2', graph=True)
        assert g.step.graph and g.step.cur_iter == 8
        g.run()
        assert g.step.cur_iter == 16 and len(g.step._graphs) >= 1
        c = g.model.state_dict()
        for k in a:
            if a[k].dtype.is_floating_point:
                assert torch.isfinite(c[k]).all() and rel_l2(c[k], a[k]) < 1e-2, (k, rel_l2(c[k], a[k]))


def test_exp_runner_command_line(tmp_path):
    """The reference's command line (exp_runner.py) on a HOCON conf file: parse, build, three iterations, checkpoints."""
    import os
    from nefii_amd.training import exp_runner
    conf_text = '''
train {
    expname = cli
    dataset_class = nefii_amd.datasets.synthetic_dataset.SyntheticSceneDataset
    model_class = model.implicit_differentiable_renderer.IDRNetwork    # the reference's name; --model_class overrides
    loss_class = nefii_amd.model.loss.IDRLoss
    idr_learning_rate = 5.0e-4
    sg_learning_rate = 5.0e-4
    num_pixels = 256
    ckpt_freq = 2
    idr_sched_milestones = [2]
    idr_sched_factor = 0.5
}
loss { %s }
model { %s }
'''
    def hocon(d, ind=1):
        out = []
        for k, v in d.items():
            if isinstance(v, dict):
                out.append('%s { %s }' % (k, hocon(v, ind + 1)))
            elif isinstance(v, (list, tuple)):
                out.append('%s = [%s]' % (k, ', '.join(str(x) for x in v)))
            elif isinstance(v, bool):
                out.append('%s = %s' % (k, 'True' if v else 'False'))
            else:
                out.append('%s = %s' % (k, v))
        return '\n'.join(out)
    mc = syn.model_conf('physg', hidden=64)
    path = os.path.join(str(tmp_path), 'run.conf')
    with open(path, 'w') as f:
        f.write(conf_text % (hocon(syn.loss_conf('physg')), hocon(mc)))
    exp_runner.main(['--conf', path, '--expname', 'cli', '--exps_folder', str(tmp_path), '--freeze_geometry',
                     '--max_niter', '3', '--nepoch', '5', '--plot_freq', '100', '--gpu', 'ignore'])
    runs = os.listdir(os.path.join(str(tmp_path), 'cli'))
    assert len(runs) == 1
    ck = os.path.join(str(tmp_path), 'cli', runs[0], 'checkpoints', 'ModelParameters')
    assert 'latest.pth' in os.listdir(ck)
    assert os.path.exists(os.path.join(str(tmp_path), 'cli', runs[0], 'runconf.conf'))


def _bench_records(stdout, full_path):
    """bench.py's output: the LAST stdout line is the compact record the driver parses (< 4 KB, flat, carrying the headline's
    own numbers), the full record - returned - is the file named by --full-out (written by a --full run)."""
    import json
    lines = [l for l in stdout.splitlines() if l.strip()]
    assert lines[-1].startswith('{') and len(lines[-1]) < 4096, len(lines[-1])
    compact = json.loads(lines[-1])
    full = json.load(open(full_path))
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'scaling', 'dtype', 'invalid'):
        assert k in compact, k
        if isinstance(full[k], float):
            assert compact[k] == pytest.approx(full[k], rel=1e-4), k
        else:
            assert compact[k] == full[k], k
    assert compact['config']['workload'] == full['config']['workload'].split(':')[0]
    if 'roofline' in full:
        # frac is what the kernels executed - never more than what the reference's recurrences would have executed
        assert compact['roofline']['frac'] == pytest.approx(full['roofline']['frac_executed'], rel=1e-3)
        assert compact['roofline']['frac'] <= compact['roofline']['frac_credited'] * 1.001
        assert compact['config']['trace_tier'] == full['config']['trace_tier']
    return full


def test_bench_two_processes_share_one_gpu():
    """bench.py's multi-process path end to end, started the way the driver starts the one-GPU bench - `python bench.py --gpus
    2`, NO launcher: the script spawns its own two ranks (torch.distributed.run as a child process, before it touches a GPU).
    Headline = config 3 (MC shading, secondary-consistency step, its own all-reduces) in weak scaling; nested: config 2 and
    1 (graph step with eager Adam), config 4 as BASELINE defines it on several GPUs (--scaling strong: the global 8192-pixel
    batch split over the ranks) and a band of config 5's frame.  Two ranks on this box's one GPU over gloo - RCCL needs two
    devices."""
    import json
    import os
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NEFII_BENCH_BACKEND='gloo')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    full_path = os.path.join(tempfile.mkdtemp(), 'bench_full.json')
    cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '4', '--repeats', '1', '--full',
           '--no-cpu-baseline', '--frame-rows', '4', '--full-out', full_path]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _bench_records(r.stdout, full_path)
    assert d['n_gpus'] == 2 and d['config']['parallelism'] == 'dp2' and d['value'] > 0 and d['scaling'] == 'weak'
    assert d['config']['workload'].startswith('cfg3') and d['config']['primary_rays_per_step_per_gpu'] == 4096 * 64
    assert d['config']['rank_param_spread'] < 1e-9       # both ranks hold the same parameters after 8+ synchronised steps
    assert d['roofline']['secondary_hit_fraction'] > 0.2 and 0 < d['roofline']['frac_8d'] < d['roofline']['frac_kernel']
    assert d['roofline']['sustained_peak']['value'] > 500.0
    for k in ('cfg2', 'cfg1'):
        assert d[k]['value'] > 0 and d[k]['config']['rank_param_spread'] < 1e-9 and d[k]['scaling'] == 'weak', d[k]['config']
    assert d['cfg4']['scaling'] == 'strong' and d['cfg4']['config']['primary_rays_per_step_per_gpu'] == 4096 * 64
    assert d['cfg4']['config']['rank_param_spread'] < 1e-9
    assert d['cfg5']['n_gpus'] == 2 and d['cfg5']['config']['finite'] and d['cfg5']['config']['primary_rays_per_frame'] == 4 * 800 * 256
    assert not d['invalid']


def test_bench_eight_processes_share_one_gpu():
    """The launch the driver makes on an 8-GPU node - `python bench.py --gpus 8`, no launcher - at the world size it will use,
    on this box's one GPU over gloo with every workload shrunk (NEFII_BENCH_PIXELS=200: 50 patches, so the contiguous split
    leaves the last rank a remainder - 6 patches per rank, 8 on rank 7, scene_dataset.py:268-279): spawn_ranks, the flat
    gradient buffer all-reduced while each rank keeps three traces (whose evaluators claim whole SIMDs) in flight, config 4's
    strong split at W = 8, and config 5's round-robin plan for ONE row of the frame - 800 pixels in 7 chunks of 128 at level
    18 - 3, i.e. a rank that renders nothing (render.py:284-295)."""
    import json
    import os
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NEFII_BENCH_BACKEND='gloo', NEFII_BENCH_PIXELS='200')
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE'):
        env.pop(k, None)
    full_path = os.path.join(tempfile.mkdtemp(), 'bench_full.json')
    cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '8', '--steps', '2', '--warmup', '4', '--repeats', '1', '--full',
           '--no-cpu-baseline', '--frame-rows', '1', '--full-out', full_path]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _bench_records(r.stdout, full_path)
    assert d['n_gpus'] == 8 and d['config']['parallelism'] == 'dp8' and d['value'] > 0 and d['scaling'] == 'weak'
    assert d['config']['num_pixels_override'] == 200 and d['config']['primary_rays_per_step_per_gpu'] == 200 * 64
    assert d['config']['trace_prefetch'] == 3            # three traces in flight beside every step's all-reduce
    assert d['config']['rank_param_spread'] < 1e-9 and d['config']['nonfinite_steps'] == 0
    for k in ('cfg2', 'cfg1'):
        assert d[k]['value'] > 0 and d[k]['config']['rank_param_spread'] < 1e-9, d[k]['config']
    # strong scaling: 50 patches over 8 ranks = 6 each, rank 0 holds 24 pixels (the remainder of 2 goes to rank 7)
    assert d['cfg4']['scaling'] == 'strong' and d['cfg4']['config']['primary_rays_per_step_per_gpu'] == 24 * 64
    assert d['cfg4']['value'] * d['cfg4']['ms_per_step'] * 1e-3 == pytest.approx(200 * 64, rel=1e-6)      # every pixel traced once
    assert d['cfg4']['config']['rank_param_spread'] < 1e-9
    assert d['cfg5']['n_gpus'] == 8 and d['cfg5']['config']['finite'] and d['cfg5']['config']['primary_rays_per_frame'] == 800 * 256
    assert not d['invalid']


def _run_bench(args, nproc, port, timeout=600):
    import json
    import os
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NEFII_BENCH_BACKEND='gloo')
    full_path = os.path.join(tempfile.mkdtemp(), 'bench_full.json')
    args = list(args) + ['--full', '--full-out', full_path]
    if nproc > 1:
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(nproc), '--master-addr',
               '127.0.0.1', '--master-port', str(port), os.path.join(root, 'bench.py'), '--gpus', str(nproc)] + args
    else:
        cmd = [sys.executable, os.path.join(root, 'bench.py')] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    return _bench_records(r.stdout, full_path)


def test_bench_strong_scaling_modes():
    """bench.py --scaling strong (BASELINE config 4's own definition: the GLOBAL 8192-pixel batch cut into contiguous per-rank
    slices, scene_dataset.py:268-279) and --workload cfg5 (one full-frame eval render as the step, chunks dealt round-robin
    and gathered on rank 0, render.py:284-336) on two ranks sharing this box's GPU over gloo, against the one-rank run: the
    same global work, the same hit statistics."""
    one = _run_bench(['--workload', 'cfg4', '--scaling', 'strong', '--steps', '2', '--warmup', '1', '--repeats', '1',
                      '--no-cpu-baseline', '--no-side-measurement'], 1, 0)
    two = _run_bench(['--workload', 'cfg4', '--scaling', 'strong', '--steps', '2', '--warmup', '1', '--repeats', '1',
                      '--no-cpu-baseline', '--no-side-measurement'], 2, 29531)
    assert one['scaling'] == two['scaling'] == 'strong' and two['n_gpus'] == 2
    assert one['config']['primary_rays_per_step_per_gpu'] == 8192 * 64
    assert two['config']['primary_rays_per_step_per_gpu'] == 4096 * 64          # half of the global batch per rank
    # value counts the GLOBAL rays of a step over the step's time on both sides
    assert abs(one['value'] * one['ms_per_step'] - two['value'] * two['ms_per_step']) < 1e-6 * one['value'] * one['ms_per_step']
    assert not one['invalid'] and not two['invalid'] and two['config']['rank_param_spread'] < 1e-9
    f1 = _run_bench(['--workload', 'cfg5', '--frame-rows', '8', '--steps', '1'], 1, 0)
    f2 = _run_bench(['--workload', 'cfg5', '--frame-rows', '8', '--steps', '1'], 2, 29533)
    for f in (f1, f2):
        assert f['scaling'] == 'strong' and f['config']['finite'] and f['config']['primary_rays_per_frame'] == 8 * 800 * 256
    assert f2['n_gpus'] == 2 and abs(f1['config']['hit_pixel_fraction'] - f2['config']['hit_pixel_fraction']) < 1e-6


def test_bench_plain_run_times_the_steps_and_dumps_the_outputs(tmp_path):
    """bench.py without --full: the headline's keys in the line and none of --full's blocks, no full record; --dump-outputs
    writes what the last timed step returned as float32 / float64 arrays within 64 MB, under the same names, shapes and loss
    on a second run with the same arguments (config 3 shrunk to 256 pixels)."""
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NEFII_BENCH_PIXELS='256')
    dumps = []
    for run in ('a', 'b'):
        full_path, dump = str(tmp_path / ('full_%s.json' % run)), str(tmp_path / run)
        cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '2', '--dump-outputs', dump,
               '--full-out', full_path]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.strip()][-1])
        for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
            assert k in line, k
        assert line['steps'] == 3 and line['warmup'] == 2 and line['value'] > 0 and line['ms_per_step'] > 0 and not line['invalid']
        assert line['config']['workload'] == 'cfg3' and line['config']['num_pixels_override'] == 256
        assert not any(k in line for k in ('roofline', 'cpu_baseline', 'parity', 'others')) and not os.path.exists(full_path)
        arrays = {f[:-4]: np.load(os.path.join(dump, f)) for f in os.listdir(dump)}
        assert all(f.endswith('.npy') for f in os.listdir(dump))
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64e6
        assert arrays['out.sg_rgb_values'].shape[0] == 256 and np.isfinite(arrays['loss.loss']).all()
        assert any(k.startswith('param.') for k in arrays)
        dumps.append(arrays)
    a, b = dumps
    assert sorted(a) == sorted(b) and a['out.sg_rgb_values'].shape == b['out.sg_rgb_values'].shape
    assert float(a['loss.loss']) == pytest.approx(float(b['loss.loss']), rel=1e-3)


@pytest.mark.parametrize('lookahead', [2, 5])
@pytest.mark.parametrize('graph', [False, True])
def test_prefetched_trace_gives_the_same_steps(graph, lookahead):
    """TrainStep(next_input=...): tracing the next batch beside this batch's tail changes the schedule, not the result -
    same losses and parameter trajectory as the plain sequence of steps, also when a prefetch is not consumed.  Small
    batches are traced in groups of three as ONE tracer call (5 batches of lookahead: whole groups; 2: partial ones),
    each batch with its own min-SDF draw."""
    from nefii_amd.training.step import TrainStep
    mc = syn.model_conf('physg', hidden=64)
    sd = syn.make_state_dict(mc, seed=4, bumpy=0.02)
    lc = syn.loss_conf('physg')
    lc['idr_rgb_weight'] = 1.0
    batches = []
    NB = 6 if lookahead == 2 else 10
    for it in range(NB):
        inp, gt = syn.make_inputs(256, (64, 64), 100.0 + 5 * it, (0.2, 0.1, 2.0 + 0.04 * it), -1, seed=30 + it)
        batches.append((to_dev(inp), {'rgb': gt.to(DEV)}))
    runs = []
    for prefetch in (False, True):
        m = build_model(mc, sd, True)
        m.ray_tracer.minsdf_steps_override = [torch.rand(100, generator=torch.Generator().manual_seed(3 + i)) for i in range(NB)]
        st = TrainStep(m, lc, graph=graph, graph_bucket=64, graph_after=2)
        losses = []
        for i, (inp, gt) in enumerate(batches):
            nxt = None
            if prefetch and i != 3:                          # one step announces nothing
                nxt = [b[0] for b in batches[i + 1:i + 1 + lookahead]] or None      # batches of lookahead
                if i == 1 and lookahead == 2:
                    nxt = nxt[0]        # a single dict is accepted too (with more batches already traced ahead it
                                        # would read as a change of plan: they are dropped and traced again)
            out, lo = st(inp, gt, nxt)
            losses.append({k: v.item() for k, v in lo.items()})
        runs.append((losses, {k: v.detach().clone() for k, v in m.state_dict().items()}))
    (l0, p0), (l1, p1) = runs
    for a, b in zip(l0, l1):
        for k in a:
            assert abs(a[k] - b[k]) <= 1e-4 * max(abs(a[k]), 1e-3), (k, a[k], b[k])
    for k in p0:
        if p0[k].dtype.is_floating_point:
            assert rel_l2(p1[k], p0[k]) < 1e-4, (k, rel_l2(p1[k], p0[k]))


@pytest.mark.gpu
@pytest.mark.parametrize('graph,lookahead', [(False, 0), (True, 3), (True, 5)])
def test_min_sdf_on_reporting_iterations_only(graph, lookahead):
    """TrainStep(min_sdf_every=E): under frozen geometry the tracer's min-SDF search (ray_tracing.py:309-337) only feeds the
    VALUE of mask_loss, which the reference reads at its logging points (idr_train.py:754,784).  Running it on the iterations
    with cur_iter % E == 0 only must change nothing else: mask_loss on the reporting iterations BIT-identical (it depends on
    the frozen geometry and the trace alone; the search's draw is made every iteration: same RNG stream), every other loss
    term of every iteration and the parameters / Adam states after 13 steps as close to the every-iteration schedule as a
    second run of that schedule is to the first (the light's gradient leaves sg_render's backward through float atomics: two
    identical runs differ in its last bits) - plain steps, traces enqueued ahead one at a time and in groups."""
    from nefii_amd.training.step import TrainStep
    mc = syn.model_conf('physg', hidden=64)
    sd = syn.make_state_dict(mc, seed=4, bumpy=0.02)
    lc = syn.loss_conf('physg')
    lc['idr_rgb_weight'] = 1.0
    NB, E = 13, 5
    batches = []
    for it in range(NB):
        inp, gt = syn.make_inputs(256, (64, 64), 100.0 + 5 * it, (0.2, 0.1, 2.0 + 0.04 * it), -1, seed=30 + it)
        batches.append((to_dev(inp), {'rgb': gt.to(DEV)}))
    runs = []
    for every in (1, 1, E):
        torch.manual_seed(77)                   # the search's uniforms come from the host generator
        m = build_model(mc, sd, True)
        st = TrainStep(m, lc, graph=graph, graph_bucket=64, graph_after=2, min_sdf_every=every)
        losses = []
        for i, (inp, gt) in enumerate(batches):
            nxt = ([b[0] for b in batches[i + 1:i + 1 + lookahead]] or None) if lookahead else None
            out, lo = st(inp, gt, nxt)
            losses.append({k: v.item() for k, v in lo.items()})
            # the schedule's two switches live on the SHARED ray tracer: set while a trace is enqueued, put back behind it
            # (a later TrainStep or a direct model(...) call must not inherit skip = True)
            assert m.ray_tracer.skip_min_sdf_search is False and m.ray_tracer.draw_when_skipped is False
        state = {k: v.detach().clone() for k, v in m.state_dict().items() if v.dtype.is_floating_point}
        for j, o in enumerate((st.idr_optimizer, st.sg_optimizer)):
            for n_, s_ in enumerate(o.state.values()):
                for k, v in s_.items():
                    if torch.is_tensor(v) and v.dtype.is_floating_point and v.numel() > 1:
                        state['opt%d.%d.%s' % (j, n_, k)] = v.detach().clone()
        runs.append((losses, state, torch.rand(1).item()))
    (l0, p0, r0), (l0b, p0b, r0b), (l1, p1, r1) = runs
    assert r0 == r0b == r1, 'the schedules leave the host RNG stream in different places'
    for k in p0:
        noise = rel_l2(p0b[k], p0[k])
        assert rel_l2(p1[k], p0[k]) <= max(4.0 * noise, 1e-4), (k, rel_l2(p1[k], p0[k]), noise)
    differ = 0
    for i, (a, b) in enumerate(zip(l0, l1)):
        for k in a:
            if k == 'mask_loss' and i % E == 0:
                assert a[k] == b[k], (i, k, a[k], b[k])
            elif k in ('loss', 'mask_loss') and i % E != 0:
                differ += a[k] != b[k]
            elif k != 'loss':
                assert abs(a[k] - b[k]) <= 1e-5 * max(abs(a[k]), 1e-3), (i, k, a[k], b[k])
            else:
                assert abs(a[k] - b[k]) <= 1e-5 * max(abs(a[k]), 1e-3), (i, k, a[k], b[k])
    assert differ > 0, 'the schedule never skipped a search: the test does not test'


@pytest.mark.gpu
def test_steps_on_traces_enqueued_ahead_do_not_synchronise_the_callers_stream(monkeypatch):
    """A graph step whose trace was enqueued ahead must not call torch.nonzero, Tensor.cpu or Tensor.item on the way (they
    would wait for the previous step's tail on the caller's stream and keep the host from running ahead: round 3's config 1
    spent half of its step there): hit lists, hit counts and the tracer's round counters arrive through pinned memory from
    the trace stream.  Checked for config 1's shape (traces grouped eight at a time) and config 2's (four at a time)."""
    from nefii_amd.training.step import TrainStep
    for name, pixels in (('cfg1', 512), ('cfg2', 4096)):
        w = syn.WORKLOADS[name]
        mc = syn.model_conf(w['model'])
        m = build_model(mc, syn.make_state_dict(mc, seed=0), True)
        inp, gt = syn.make_inputs(pixels, w['image_hw'], w['focal'], w['cam_pos'], -1, seed=1)
        inp, gt = to_dev(inp), {'rgb': gt.to(DEV)}
        st = TrainStep(m, syn.loss_conf(w['model']), graph=True)
        nxt = [inp] * st.preferred_lookahead(inp)
        for _ in range(24 if name == 'cfg2' else 40):     # eager steps, the capture, the tracer's round guess settle (per tracer call)
            st(inp, gt, nxt)
        torch.cuda.synchronize()
        calls = []
        real_nonzero, real_cpu, real_item = torch.nonzero, torch.Tensor.cpu, torch.Tensor.item
        monkeypatch.setattr(torch, 'nonzero', lambda t, *a, **k: (calls.append('nonzero') if t.is_cuda else None, real_nonzero(t, *a, **k))[1])
        monkeypatch.setattr(torch.Tensor, 'cpu', lambda t, *a, **k: (calls.append('cpu') if t.is_cuda else None, real_cpu(t, *a, **k))[1])
        monkeypatch.setattr(torch.Tensor, 'item', lambda t: (calls.append('item') if t.is_cuda else None, real_item(t))[1])
        for _ in range(9 if name == 'cfg2' else 17):     # (at least two tracer calls: of four batches for config 2, of eight for config 1)
            out, lo = st(inp, gt, nxt)
        monkeypatch.undo()
        torch.cuda.synchronize()
        assert calls == [], (name, calls)
        assert int(st.nonfinite_steps.item()) == 0 and torch.isfinite(lo['loss']).item()


@pytest.mark.gpu
@pytest.mark.parametrize('pixels', [1280, 4352])
def test_traces_enqueued_ahead_are_dropped_when_their_bound_fails(pixels):
    """A trace enqueued ahead under a coarse bound that its own audit then finds violated is dropped - with every trace
    enqueued after it - when its batch comes up: the batch is traced again without the coarse pass, the drop counts once in
    retraced_steps, and the 'disabled' event is recorded once, with the iteration in which it reached the host.  Both sizes
    are above RayTracing.coarse_min_rays (the audit runs); 1280 rays are traced four batches per call, 4352 one at a time."""
    import warnings
    from nefii_amd.training.step import TrainStep
    mc = syn.model_conf('physg')                # the coarse pass needs the 512-wide net
    m = build_model(mc, syn.make_state_dict(mc, seed=0), True)
    net, rt = m.implicit_network, m.ray_tracer
    pool = []
    for it in range(4):
        inp, gt = syn.make_inputs(pixels, seed=40 + it)
        pool.append((to_dev(inp), {'rgb': gt.to(DEV)}))
    seq = [(dict(pool[i % 4][0]), pool[i % 4][1]) for i in range(48)]       # one dict object per step: the queue goes by identity
    st = TrainStep(m, syn.loss_conf('physg'), graph=False)
    G, L = st.trace_group_for(seq[0][0]), st.preferred_lookahead(seq[0][0])
    assert G == (4 if pixels <= 4096 else 1)
    losses = []

    def step(i):
        out, lo = st(seq[i][0], seq[i][1], [b[0] for b in seq[i + 1:i + 1 + L]])
        losses.append(lo['loss'].item())

    i = 0
    # ... until the audit has reported, and the next step enqueues (it does so before it takes its own trace)
    while i == 0 or net.coarse_audit_max <= 0.0 or len(st._prefetch) + G > L + 1:
        step(i)
        i += 1
        assert i < 8
    assert st.retraced_steps == 0 and net.coarse_tau(rt.object_bounding_sphere) > 0.0
    net._tau = (net._tau[0], net._tau[1], 0.1 * net.coarse_audit_max)
    before = {id(e[0]) for e in st._prefetch}
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        step(i)
        fresh = [e[0] for e in st._prefetch if id(e[0]) not in before]
        assert fresh, 'nothing was enqueued under the understated bound: the test does not test'
        consumed_at = next(k for k, b in enumerate(seq) if b[0] is fresh[0])
        for i in range(i + 1, consumed_at + 1):
            assert st.retraced_steps == 0
            step(i)
    assert any('coarse pass' in str(x.message) for x in w)
    assert st.retraced_steps == 1
    disabled = [e for e in st.coarse_events if e[1] == 'disabled']
    assert len(disabled) == 1 and disabled[0][0] == consumed_at, st.coarse_events
    assert net.coarse_tau(rt.object_bounding_sphere) == 0.0
    for i in range(consumed_at + 1, consumed_at + 3):
        step(i)
    assert len(st._prefetch) > 0 and st.retraced_steps == 1
    assert len([e for e in st.coarse_events if e[1] == 'disabled']) == 1
    assert all(np.isfinite(v) for v in losses) and int(st.nonfinite_steps.item()) == 0


@pytest.mark.gpu
def test_runner_on_a_scene_directory_with_exr_ground_truth(tmp_path):
    """The runner fed from an instance directory as the reference lays it out (cam_dict_norm.json, image/*.exr,
    mask/*.png) through `datasets.scene_dataset.SceneDataset`, the class name the reference's confs carry."""
    import json
    import os
    import numpy as np
    from PIL import Image
    from nefii_amd.training.idr_train import IDRTrainRunner
    from nefii_amd.utils import exr
    inst = tmp_path / 'scene'
    (inst / 'image').mkdir(parents=True)
    (inst / 'mask').mkdir()
    H = W = 40
    g = np.random.Generator(np.random.Philox(1))
    cams = {}
    for i in range(4):
        phi = 2 * np.pi * i / 4
        c2w = syn.look_at_origin_pose((2.4 * np.sin(phi), 0.4, 2.4 * np.cos(phi)))
        K = np.eye(4)
        K[0, 0] = K[1, 1] = 1111.0 * W / 800.0
        K[0, 2], K[1, 2] = W / 2.0, H / 2.0
        name = 'rgb_%06d.exr' % i
        cams[name] = {'K': K.reshape(-1).tolist(), 'W2C': np.linalg.inv(c2w).reshape(-1).tolist(), 'img_size': [W, H]}
        exr.imwrite(str(inst / 'image' / name), g.uniform(0, 1.5, size=(H, W, 3)).astype(np.float32))
        yy, xx = np.mgrid[0:H, 0:W]
        Image.fromarray((((yy - H / 2) ** 2 + (xx - W / 2) ** 2 < 15 ** 2) * 255).astype(np.uint8)).save(
            inst / 'mask' / ('mask_%06d.png' % i))
    (inst / 'cam_dict_norm.json').write_text(json.dumps(cams))
    cfg = _runner_conf(tmp_path, n_pix=128)
    cfg['train']['dataset_class'] = 'datasets.scene_dataset.SceneDataset'
    torch.manual_seed(0)
    r = IDRTrainRunner(conf=cfg, exps_folder_name=str(tmp_path), freeze_geometry=True, nepochs=1000, graph=False,
                       expname='scene', max_niters=5, new_timestamp='t0', data_split_dir=str(inst), gamma=2.2, log_freq=2,
                       plot_freq=3, memory_capacity_level=10)
    assert type(r.train_dataset).__name__ == 'SceneDataset' and r.train_dataset.img_res == [H, W]
    assert torch.allclose(r.train_dataset.rgb_images[0].max(), torch.tensor(1.5 ** 2.2), rtol=1e-2)
    sd = syn.make_state_dict(cfg.get_config('model'), seed=4, bumpy=0.02)
    r.model.load_state_dict(sd)
    r.model.freeze_geometry()
    before = {k: v.clone() for k, v in r.model.state_dict().items()}
    r.run()
    assert r.step.cur_iter == 6
    after = r.model.state_dict()
    moved = [k for k in before if before[k].dtype.is_floating_point and not torch.equal(before[k].to(after[k].device), after[k])]
    assert any(k.startswith('envmap_material_network') for k in moved)
    assert not any(k.startswith('implicit_network') for k in moved)
    assert all(torch.isfinite(v).all() for v in after.values() if v.dtype.is_floating_point)
    assert os.path.exists(os.path.join(str(tmp_path), 'scene', 't0', 'checkpoints', 'ModelParameters', 'latest.pth'))
    # vis_train wrote views 0 and 1 at iterations 0 and 3 (eval-mode full frames beside the training batches)
    tp = os.path.join(str(tmp_path), 'scene', 't0', 'plots')
    assert sorted(f for f in os.listdir(tp) if f.startswith('render_')) == ['render_000.png', 'render_003.png']
    assert exr.imread(os.path.join(tp, 'rerender_rgb-003.exr')).shape == (H, W, 3)
    assert r.train_dataset.sampling_idx is not None and r.model.training
    # ... and the render script over the same directory as its test split, from view 2 on, then evaluate.py
    from nefii_amd.scripts.render import RenderRunner
    from nefii_amd.scripts import evaluate as ev
    rr = RenderRunner(conf=cfg, exps_folder_name=str(tmp_path), expname='scene', timestamp='latest', checkpoint='latest',
                      new_timestamp='t1', data_split_dir_test=str(inst), gamma=2.2, memory_capacity_level=10, start_index=2,
                      num_rays=4)
    assert rr.run() == [2, 3]
    plots = os.path.join(str(tmp_path), 'scene', 't1', 'plots')
    files = sorted(os.listdir(plots))
    assert 'envmap.exr' in files and 'render_002.png' in files and 'rerender_rgb-003.exr' in files and len(files) == 17
    gt2 = exr.imread(os.path.join(plots, 'gt-002.exr'))
    assert gt2.shape == (H, W, 3) and np.allclose(gt2.reshape(-1, 3), r.train_dataset.rgb_images[2].numpy())
    pred = exr.imread(os.path.join(plots, 'rerender_rgb-002.exr'))
    assert np.isfinite(pred).all() and pred.max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize('name,hidden,n', [('physg', 64, 700), ('conf', 512, 300), ('neus', None, 257)])
def test_sdf_weight_gradients_for_the_geometry_fit(name, hidden, n):
    """Step-1: d L1(sdf(x), target) / d(weight_v, weight_g, bias) of the SDF network through the fused kernels (skip
    layer included) against torch autograd on the fp64 oracle."""
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    mc = syn.model_conf(name, hidden=hidden)
    sd = syn.make_state_dict(mc, seed=6, bumpy=0.02 if hidden == 64 else 0.004)
    g = torch.Generator().manual_seed(8)
    for l in mc['implicit_network']['skip_in']:
        w = sd['implicit_network.lin%d.weight_v' % l]
        w[:, -36:] = torch.randn(w.shape[0], 36, generator=g) * 0.02
    m = IDRNetwork(conf.from_dict(mc))
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    x = torch.randn(n, 3, generator=g) * 0.5
    target = torch.randn(n, 1, generator=g) * 0.3
    net = m.implicit_network
    net.train()
    pred = net(x.to(DEV))
    assert pred.requires_grad and pred.shape == (n, 1 + mc['feature_vector_size'])
    loss = torch.nn.functional.l1_loss(pred[:, 0:1], target.to(DEV))
    loss.backward()
    ref_sd = {k: v.double().clone().requires_grad_(k.startswith('implicit_network')) for k, v in sd.items()}
    ref = nets.sdf_forward(ref_sd, mc['implicit_network'], x.double())
    assert rel_l2(pred, ref) < 1e-5
    ref_loss = torch.nn.functional.l1_loss(ref[:, 0:1], target.double())
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-5
    for k, p in net.named_parameters():
        want = ref_sd['implicit_network.' + k].grad
        assert p.grad is not None and rel_l2(p.grad, want) < 1e-3, (k, rel_l2(p.grad, want))
    with pytest.raises(NotImplementedError):      # gradients wrt positions stay out of scope
        net.gradient(x.to(DEV))


@pytest.mark.gpu
def test_geometry_fit_runner_regresses_a_box(tmp_path):
    """GeometryTrainRunner (geometry_train.py): L1 regression of the SDF net onto samples of a mesh; checkpoint layout of
    the reference; the fitted geometry loads into a Step-2 model through the pretrain_geometry_path route."""
    import os
    from nefii_amd.training.geometry_train import GeometryTrainRunner, SUBDIRS
    from test_geometry_cpu import box_mesh, box_sdf
    lo, hi = (-0.45, -0.3, -0.35), (0.4, 0.35, 0.3)
    v, f, _ = box_mesh(lo, hi)
    cfg = _runner_conf(tmp_path)
    cfg['train']['idr_learning_rate'] = 1e-3
    cfg['train']['idr_sched_milestones'] = [200]
    cfg['train']['ckpt_freq'] = 100
    torch.manual_seed(0)
    r = GeometryTrainRunner(conf=cfg, exps_folder_name=str(tmp_path), expname='s1', new_timestamp='t0', mesh=(v, f),
                            scale_to_unit=False, sample_num=512, batch_size=4096, max_niters=1000, nepochs=1, log_freq=50)
    # 1000 items of 512 samples, 8 per batch: 125 iterations per epoch, epochs 0 and 1 (geometry_train.py:347)
    assert r.train_dataloader.batch_size == 8 and len(r.train_dataloader) == 125
    hist = r.run()
    assert r.cur_iter == 250 and hist[0][1] > 5 * hist[-1][1], hist
    assert abs(r.idr_scheduler.get_last_lr()[0] - 5e-4) < 1e-12
    ck = os.path.join(str(tmp_path), 's1', 't0', 'checkpoints')
    for sub in SUBDIRS.values():
        # keyed by the batch index within the epoch (geometry_train.py:352-353): iterations 0, 100, 200 = batches 0, 100, 75
        assert sorted(os.listdir(os.path.join(ck, sub))) == ['0.pth', '1.pth', '100.pth', '75.pth', 'latest.pth'], sub
    d = torch.load(os.path.join(ck, 'ModelParameters', 'latest.pth'))
    assert set(d) == {'epoch', 'model_state_dict'}
    # the fitted field through the frozen (Step-2) evaluation path
    g = np.random.Generator(np.random.Philox(4))
    p = g.uniform(-0.8, 0.8, size=(3000, 3))
    m = build_model(cfg.get_config('model'), d['model_state_dict'], training=False)
    with torch.no_grad():
        pred = m.implicit_network(torch.from_numpy(p).float().to(DEV))[:, 0].cpu().numpy()
    err = np.abs(pred - box_sdf(p, lo, hi))
    assert err.mean() < 0.03, err.mean()
    cont = GeometryTrainRunner(conf=cfg, exps_folder_name=str(tmp_path), expname='s1', new_timestamp='t1', mesh=(v, f),
                               scale_to_unit=False, sample_num=512, batch_size=4096, max_niters=5, is_continue=True)
    a, b = cont.model.state_dict(), d['model_state_dict']
    assert all(torch.equal(a[k].cpu(), b[k].cpu()) for k in b)
    assert cont.idr_optimizer.state_dict()['state'][0]['step'] == 250


@pytest.mark.gpu
def test_render_writes_the_buffers_evaluate_reads(tmp_path):
    """render.py's per-frame files (gt / rerender_rgb / diffuse_rgb / specular_rgb / diffuse_albedo / roughness /
    specular_reflection EXRs, the PNG strip, envmap.exr) and scripts/evaluate.py over them."""
    import os
    from PIL import Image
    from nefii_amd.scripts import evaluate as ev
    from nefii_amd.training import render as R
    from nefii_amd.utils import exr
    mc = syn.model_conf('physg', hidden=64)
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    m = build_model(mc, sd, False)
    H, W = 24, 32
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    uv = torch.stack([xs, ys], -1).reshape(1, -1, 2).float() * 2.0 + 1.0
    inp, _ = syn.make_inputs(16, (64, 64), 100.0, (0.2, 0.1, 2.0), -1, seed=2)
    full = to_dev({'uv': uv, 'object_mask': torch.ones(1, H * W, dtype=torch.bool), 'pose': inp['pose'],
                   'intrinsics': inp['intrinsics']})
    out = R.render_frame(m, full, H * W, num_rays=1, memory_capacity_level=8)
    gt = out['sg_rgb_values'].reshape(1, H * W, 3) * 0.9
    plots = str(tmp_path / 'exp' / 'plots')
    buf = R.write_frame(m, out, gt, full['pose'], [H, W], plots, 7)
    hit = out['network_object_mask'].reshape(H, W).cpu()
    assert hit.any() and not hit.all()
    names = ['gt', 'rerender_rgb', 'diffuse_rgb', 'specular_rgb', 'diffuse_albedo', 'roughness', 'specular_reflection']
    assert sorted(os.listdir(plots)) == sorted(['%s-007.exr' % n for n in names] + ['render_007.png'])
    back = exr.imread(os.path.join(plots, 'rerender_rgb-007.exr'))
    assert np.array_equal(back, out['sg_rgb_values'].reshape(H, W, 3).cpu().numpy())
    rough = exr.imread(os.path.join(plots, 'roughness-007.exr'))
    assert np.array_equal(rough[..., 0], rough[..., 2]) and np.array_equal(
        rough[..., 0], out['sg_roughness_values'].reshape(H, W).cpu().numpy())
    assert Image.open(os.path.join(plots, 'render_007.png')).size == (8 * W, H)
    d = buf['depth'][..., 0]
    assert torch.allclose(d[~hit], 0.98 * d[hit].min().expand_as(d[~hit])) and (d[hit] > 0.5).all()
    # envmap: the background-radiance kernel over the lat-long grid = the closed form, both axis conventions
    lgt = m.envmap_material_network.get_light()
    for ct in ('mitsuba', 'blender'):
        env = R.compute_envmap(lgt, 16, 32, coordinate_type=ct).cpu().double()
        dirs = R.envmap_directions(16, 32, False, ct).double()
        l = lgt.cpu().double()
        ax = l[:, :3] / l[:, :3].norm(dim=-1, keepdim=True)
        ref = (l[:, -3:].abs() * torch.exp(l[:, 3:4].abs() * ((dirs[..., None, :] * ax).sum(-1, keepdim=True) - 1))).sum(-2)
        assert rel_l2(env, ref) < 1e-5
    assert abs(R.envmap_directions(8, 16, False, 'blender')[0, 0] - torch.tensor([0., 0., 1.])).max() < 1e-6
    import os as _os
    gold = dict(np.load(_os.path.join(_os.path.dirname(_os.path.abspath(__file__)), 'golden', 'envmap_ref.npz')))
    for ct in ('mitsuba', 'blender'):           # the kernel against the reference's compute_envmap (make_envmap_golden.py)
        for hemi in (False, True):
            env = R.compute_envmap(torch.from_numpy(gold['lgtSGs']).to(DEV), 12, 20, upper_hemi=hemi, coordinate_type=ct)
            assert rel_l2(env, torch.from_numpy(gold['%s_%d' % (ct, int(hemi))])) < 1e-5, (ct, hemi)
    R.write_envmap(m, plots)
    assert exr.imread(os.path.join(plots, 'envmap.exr')).shape == (256, 512, 3)
    # evaluate.py over a ground-truth directory built from the same buffers
    gtd = tmp_path / 'scene' / 'test'
    for sub in ('image', 'diffuse', 'roughness', 'sp_rgb', 'mask'):
        (gtd / sub).mkdir(parents=True)
    Image.fromarray((hit.numpy() * 255).astype(np.uint8)).save(gtd / 'mask' / '000007.png')
    exr.imwrite(str(gtd / 'image' / '000007.exr'), buf['gt'].numpy())
    exr.imwrite(str(gtd / 'diffuse' / '000007_diffuse.00.exr'), buf['diffuse_albedo'].numpy() * np.float32(2.0))
    exr.imwrite(str(gtd / 'roughness' / '000007.exr'), buf['roughness'].numpy())
    exr.imwrite(str(gtd / 'sp_rgb' / '000007_sprgb.00.exr'), buf['specular_rgb'].numpy())
    res = ev.main(plots, str(gtd))
    assert 20 < res['rgb']['psnr'] < 60 and res['roughness']['mse'] == 0 and res['sp_rgb']['psnr'] == float('inf')
    assert res['diffuse_align']['psnr'] > res['diffuse']['psnr'] + 3


@pytest.mark.gpu
@pytest.mark.parametrize('name,hidden,num_rays,iters,drop', [('physg', 64, -1, 120, 0.4), ('physg', 64, 4, 72, 0.5),
                                                             ('conf', 64, 4, 72, 0.8), ('neus', None, 4, 48, 1.0)])
def test_step2_training_recovers_a_rendered_target(name, hidden, num_rays, iters, drop):
    """The whole Step-2 loop learns, eagerly and with the captured step alike: ground truth = renders of a 'teacher'
    material / light on frozen geometry, the student starts from a different material / light; 120 TrainStep iterations
    over 12 pixel batches (different hit counts, one padded size: one graph replayed ~115 times; the next batches'
    traces prefetched) bring the rgb loss down several times.  In graph mode every gradient of every replay is also
    compared with an eager recomputation: this is the test that caught weight gradients zeroed by a hipMemsetAsync
    node going non-finite after a few replays (nefii_mlp_wgrad now zeroes with a kernel)."""
    from nefii_amd.model.loss import IDRLoss
    from nefii_amd.training.step import TrainStep
    # (the MC-shaded models' targets carry fresh sampling noise every time they are rendered: their loss has a high floor,
    # the full-size neus case only has to stay finite and not rise)
    # also with several jittered rays per pixel, and - eager only: its Monte-Carlo shading draws fresh samples every call,
    # so a recomputed gradient is not reproducible - for the conf.conf model (MC direct + near-field indirect shading,
    # secondary-consistency step every 10 iterations)
    mc = syn.model_conf(name, hidden=hidden)         # hidden=None: the conf's own sizes (neus: the 256-wide tracer kernel)
    lc = syn.loss_conf(name)
    mc_shading = mc.get('render_type', 'sg') != 'sg'
    teacher = build_model(mc, syn.make_state_dict(mc, seed=11, bumpy=0.0), training=False)
    sd = syn.make_state_dict(mc, seed=12, bumpy=0.0)
    for k, v in teacher.state_dict().items():           # same geometry (and radiance field), different material / light
        if not k.startswith('envmap_material_network'):
            sd[k] = v.cpu().clone()

    def batch(seed):
        inp, _ = syn.make_inputs(1024 if num_rays < 0 else 256, (96, 96), 130.0, (0.3, 0.2, 2.2), num_rays, seed=seed)
        inp = to_dev(inp)
        with torch.no_grad():
            target = teacher(inp)
        return inp, {'rgb': target['sg_rgb_values'].reshape(1, -1, 3).clone()}

    batches = [batch(100 + i) for i in range(12)]
    loss_fn = IDRLoss(**lc)
    final = {}
    for graph in ((False,) if mc_shading else (False, True)):
        student = build_model(mc, sd, training=True)
        shadow = build_model(mc, sd, training=True)
        step = TrainStep(student, lc, idr_lr=5e-4, sg_lr=5e-3, graph=graph, graph_after=3, num_rays=num_rays,
                         secondary_train_interval=10 if mc_shading else 0, secondary_batch_size=256)
        losses = []
        for it in range(iters):
            inp, gt = batches[it % 12]
            nxt = [batches[(it + 1) % 12][0], batches[(it + 2) % 12][0]]
            if graph:
                shadow.load_state_dict(student.state_dict())
            out, lo = step(inp, gt, nxt)
            losses.append(lo['sg_rgb_loss'].item())
            if graph and it >= 3:
                for p in shadow.parameters():
                    p.grad = None
                loss_fn(shadow(inp), gt)['loss'].backward()
                for (name, p), (_, q) in zip(student.named_parameters(), shadow.named_parameters()):
                    if q.grad is not None:
                        assert torch.isfinite(p.grad).all(), (it, name)
                        # (+ 1e-9 absolute: the global specular parameter's gradient passes through zero as it trains - seen at -4.0e-8,
                        # where the float atomics' summation order alone is 1.3e-10 = 3e-3 of it)
                        assert (p.grad - q.grad).norm().item() < 1e-3 * q.grad.norm().item() + 1e-9, (it, name, rel_l2(p.grad, q.grad))
        first, last = sum(losses[:12]) / 12, sum(losses[-12:]) / 12
        assert last < drop * first and all(l == l for l in losses), (graph, first, last)
        for opt in (step.idr_optimizer, step.sg_optimizer):
            for st in opt.state_dict()['state'].values():
                assert torch.isfinite(st['exp_avg_sq']).all() and torch.isfinite(st['exp_avg']).all()
        if graph:
            assert 1 <= len(step._graphs) <= 4          # padded hit counts: a handful of graphs, replayed ~100 times
        final[graph] = last
        for k, v in student.state_dict().items():
            assert not v.dtype.is_floating_point or torch.isfinite(v).all(), k
    if not mc_shading:
        assert abs(final[True] - final[False]) < 0.15 * final[False], final


@pytest.mark.gpu
def test_runner_partial_checkpoint_loads(tmp_path):
    """The runner's partial loads (idr_train.py:205-249,294-306): --pretrain_geometry_path / --pretrain_idr_rendering_path
    / --pretrain_diffuse_path take their sub-network from a full checkpoint, --geometry every key containing
    'implicit_network', --geometry_neus a NeuS checkpoint's `sdf_network_fine` straight into the SDF net, --light_sg_path
    an .npy of light lobes (7 columns: coloured light)."""
    from nefii_amd.training.idr_train import IDRTrainRunner
    cfg = _runner_conf(tmp_path)
    mc = cfg.get_config('model')
    donor = {k: syn.make_state_dict(mc, seed=s, bumpy=0.01) for k, s in (('geo', 21), ('idr', 22), ('dif', 23), ('neus', 24))}
    for k in ('geo', 'idr', 'dif'):
        torch.save({'epoch': 3, 'model_state_dict': donor[k]}, str(tmp_path / (k + '.pth')))
    torch.save({'sdf_network_fine': {k[len('implicit_network.'):]: v for k, v in donor['neus'].items()
                                     if k.startswith('implicit_network.')}}, str(tmp_path / 'neus.pth'))
    lgt = np.random.Generator(np.random.Philox(3)).normal(size=(32, 7)).astype(np.float32)
    np.save(str(tmp_path / 'light.npy'), lgt)
    kw = dict(conf=cfg, exps_folder_name=str(tmp_path), freeze_geometry=True, nepochs=1, graph=False,
              dataset_kwargs={'n_views': 2, 'img_res': (16, 16)})

    def same(model_sd, src, prefix):
        keys = [k for k in src if k.startswith(prefix)]
        assert keys
        return all(torch.equal(model_sd[k].cpu(), src[k]) for k in keys)

    torch.manual_seed(0)
    base = IDRTrainRunner(expname='a', new_timestamp='t', **kw).model.state_dict()
    r = IDRTrainRunner(expname='b', new_timestamp='t', pretrain_geometry_path=str(tmp_path / 'geo.pth'),
                       pretrain_idr_rendering_path=str(tmp_path / 'idr.pth'), pretrain_diffuse_path=str(tmp_path / 'dif.pth'),
                       light_sg_path=str(tmp_path / 'light.npy'), **kw)
    sd = r.model.state_dict()
    assert same(sd, donor['geo'], 'implicit_network.') and same(sd, donor['idr'], 'rendering_network.')
    assert same(sd, donor['dif'], 'envmap_material_network.diffuse_albedo_layers.')
    assert not same(sd, donor['geo'], 'rendering_network.') and not same(sd, donor['idr'], 'implicit_network.')
    mat = r.model.envmap_material_network
    assert np.array_equal(mat.lgtSGs.detach().cpu().numpy(), lgt) and mat.numLgtSGs == 32 and mat.white_light is False
    assert set(sd) == set(base)
    r2 = IDRTrainRunner(expname='c', new_timestamp='t', geometry=str(tmp_path / 'idr.pth'),
                        geometry_neus=str(tmp_path / 'neus.pth'), **kw)
    sd2 = r2.model.state_dict()
    assert same(sd2, donor['neus'], 'implicit_network.')            # applied after --geometry, as in the reference
    r3 = IDRTrainRunner(expname='d', new_timestamp='t', geometry=str(tmp_path / 'idr.pth'), **kw)
    assert same(r3.model.state_dict(), donor['idr'], 'implicit_network.')
    assert not same(r3.model.state_dict(), donor['idr'], 'rendering_network.')


def _ddp_worker(rank, world, port, tmp):
    import os
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    from nefii_amd.model.loss import IDRLoss
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)         # RCCL needs two devices; gloo stages through the host
    torch.cuda.set_device(0)
    mc = syn.model_conf('conf', hidden=64)
    torch.manual_seed(100 + rank)                                        # every rank builds ITS OWN initialisation ...
    m = IDRNetwork(conf.from_dict(mc)).to(DEV)
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    m.implicit_network.load_state_dict({k[len('implicit_network.'):]: v for k, v in sd.items()
                                        if k.startswith('implicit_network.')})
    ddp = DistributedDataParallel(m, device_ids=[0], find_unused_parameters=True)    # idr_train.py:308-309
    ddp.module.freeze_geometry()                                          # after the wrap, as in the reference (:621-626)
    ddp.train()
    start = {k: v.detach().clone().cpu() for k, v in ddp.module.state_dict().items()}
    # rank 1 looks away from the object: no hit, no gradient for the radiance / material networks on that rank
    inp, gt = syn.make_inputs(64, (64, 64), 100.0, (0.2, 0.1, 2.0), 2, seed=6 + rank)
    if rank == 1:
        pose = inp['pose'].clone()
        pose[0, :3, 3] = torch.tensor([0., 0., 5.0])
        pose[0, :3, 2] = torch.tensor([0., 0., 1.0])
        inp['pose'] = pose
    ddp.module.ray_tracer.minsdf_steps_override = [torch.rand(100, generator=torch.Generator().manual_seed(3))] * 2
    ddp.module.uniforms_override = None
    out = ddp(to_dev(inp))
    lo = IDRLoss(**syn.loss_conf('conf'))(out, {'rgb': gt.to(DEV)})
    lo['loss'].backward()
    grads = {n: (p.grad.detach().clone().cpu() if p.grad is not None else None) for n, p in ddp.module.named_parameters()}
    torch.save({'start': start, 'grads': grads, 'hits': int(out['network_object_mask'].sum())},
               os.path.join(tmp, 'ddp%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_distributed_data_parallel_wraps_the_model_unchanged(tmp_path):
    """INTEGRATION.md's claim, exercised: the reference's wrap - DistributedDataParallel(model,
    find_unused_parameters=True), frozen afterwards (idr_train.py:308-309,621-626) - works on this IDRNetwork as it is:
    construction broadcasts rank 0's parameters, forward / backward run through the custom autograd Functions of the HIP
    ops, the reducer averages their gradients, and a rank without a single hit (no gradient for the radiance / material
    networks there) neither hangs nor desynchronises.  Two processes share this box's GPU over gloo."""
    import os
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_ddp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    a, b = (torch.load(os.path.join(str(tmp_path), 'ddp%d.pt' % r)) for r in (0, 1))
    assert a['hits'] > 0 and b['hits'] == 0
    for k in a['start']:
        assert torch.equal(a['start'][k], b['start'][k]), k             # rank 1 started from rank 0's parameters
    n_grad = 0
    for k, g in a['grads'].items():
        h = b['grads'][k]
        assert (g is None) == (h is None), k
        if g is not None:
            assert torch.equal(g, h), k                                   # averaged: identical on both ranks
            assert torch.isfinite(g).all(), k
            n_grad += g.abs().sum().item() > 0
    assert n_grad > 10


@pytest.mark.gpu
@pytest.mark.parametrize('graph', [False, True])
def test_nonfinite_step_is_skipped_not_run_on_zero_gradients(graph):
    """TrainStep's NaN guard on the GPU (fused Adam, `found_inf`): a step whose loss is not finite leaves parameters, both
    moments and the step counters exactly as they were (reference: the runner stops before backward / step,
    idr_train.py:754-757), is counted, and the next step trains again - eager and with the tail replayed as a hipGraph."""
    from nefii_amd.training.step import TrainStep
    mc = syn.model_conf('physg', hidden=64)
    sd = syn.make_state_dict(mc, seed=4, bumpy=0.02)
    lc = syn.loss_conf('physg')
    lc['idr_rgb_weight'] = 1.0
    m = build_model(mc, sd, True)
    st = TrainStep(m, lc, graph=graph, graph_bucket=64, graph_after=2)
    inp, gt = syn.make_inputs(256, (64, 64), 100.0, (0.2, 0.1, 2.0), -1, seed=31)
    inp, good = to_dev(inp), {'rgb': gt.to(DEV)}
    bad = {'rgb': good['rgb'].clone()}
    bad['rgb'][0, ::7] = float('nan')

    def snapshot():
        opt_state = []
        for opt in (st.idr_optimizer, st.sg_optimizer):
            for p in opt.param_groups[0]['params']:
                s = opt.state.get(p, {})
                opt_state.append({k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in s.items()})
        return {k: v.detach().clone() for k, v in m.state_dict().items()}, opt_state

    for _ in range(4):                      # past graph_after: the captured tail is what replays below
        st(inp, good)
    p0, o0 = snapshot()
    out, lo = st(inp, bad)
    assert not torch.isfinite(lo['loss']).item()
    p1, o1 = snapshot()
    assert int(st.nonfinite_steps.item()) == 1
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
    for a, b in zip(o0, o1):
        for k in a:
            if torch.is_tensor(a[k]):
                assert torch.equal(a[k], b[k]), k
    st(inp, good)
    p2, _ = snapshot()
    assert any(not torch.equal(p1[k], p2[k]) for k in p1 if p1[k].dtype.is_floating_point)
    assert all(torch.isfinite(v).all() for v in p2.values() if v.dtype.is_floating_point)
    assert int(st.nonfinite_steps.item()) == 1
