"""The patch terms of IDRLoss on the GPU (nefii_idr_patch_loss through ops.PatchLossFn): every case of
tests/golden/patch_loss.npz within the bounds of test_patch_loss_cpu.py (expected values: the reference in fp64; a gradient's
relative L2 at most 8 x the reference's own fp32 error for that case, a scalar's absolute error at most 8 x the largest such
scalar error of the file), run-to-run bits, the fused IDRLoss against the torch formulation, and a captured training step."""
import numpy as np
import pytest
import torch

import patchloss_ref as ref
from nefii_amd import conf, ops, synthetic as syn
from nefii_amd.model.loss import IDRLoss

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = ref.golden()
BASE = dict(idr_rgb_weight=1.0, sg_rgb_weight=1.0, eikonal_weight=0.1, mask_weight=100.0, alpha=50.0, normalsmooth_weight=1.0,
            loss_type='L1', env_loss_type='L2', background_rgb_weight=0.5)        # make_patchloss_golden.py: BASE


def run_patch_fn(c, weights=None):
    """ops.PatchLossFn on a golden case -> (losses [4], d losses[0] / d (idr, sg, rough)) as numpy"""
    wi, ws, wr = (float(w) for w in (c['weights'] if weights is None else weights))
    t = lambda k: torch.from_numpy(c[k]).to(DEV)
    leaves = [t('idr').requires_grad_(True), t('sg').requires_grad_(True), t('rough').requires_grad_(True)]
    lo = ops.PatchLossFn.apply(*leaves, t('gt'), t('net'), t('obj'), t('normal'), ops.patch_loss_params(wi, ws, wr, int(c['r_patch'])))
    grads = torch.autograd.grad(lo[0], leaves)
    return lo.detach().cpu().numpy(), [g.cpu().numpy() for g in grads]


@pytest.mark.parametrize('i', range(len(G.names)), ids=G.names)
def test_kernel_matches_the_reference(i):
    c = G.cases[i]
    losses, grads = run_patch_fn(c)
    assert grads[0].shape == c['idr'].shape and grads[2].shape == c['rough'].shape
    ref.check_against_golden(c, losses, *grads, what=G.names[i])


def test_two_runs_give_the_same_bits():
    for name in ('two_holes', 'cap_smooth', 'rough_r1'):
        c = G.cases[G.names.index(name)]
        (l0, g0), (l1, g1) = run_patch_fn(c), run_patch_fn(c)
        assert l0.tobytes() == l1.tobytes()
        for a, b in zip(g0, g1):
            assert a.tobytes() == b.tobytes()


def test_one_ssim_weight_at_zero_still_reports_both_values():
    """the reference computes both SSIM values when either is weighted; the unweighted colour gets a zero gradient"""
    c = G.cases[G.names.index('p14_hole')]
    losses, grads = run_patch_fn(c, weights=(0.0, 0.25, 0.0))
    bound = ref.MARGIN * G.scalar_yard
    assert abs(losses[1] - c['terms64'][1]) <= bound and abs(losses[2] - c['terms64'][2]) <= bound and losses[3] == 0
    assert abs(losses[0] - 0.25 * c['terms64'][2]) <= bound
    assert not grads[0].any() and not grads[2].any() and grads[1].any()


def _outputs(c, dev=DEV):
    t = lambda k: torch.from_numpy(c[k]).to(dev)
    return ({'idr_rgb_values': t('idr').requires_grad_(True), 'sg_rgb_values': t('sg').requires_grad_(True),
             'sg_roughness_values': t('rough').requires_grad_(True), 'sdf_output': t('sdf'), 'normal_values': t('normal'),
             'grad_theta': None, 'network_object_mask': t('net'), 'object_mask': t('obj')}, {'rgb': t('gt').reshape(1, -1, 3)})


def test_fused_idrloss_matches_the_torch_formulation():
    """(6, 5) with every term weighted: the two paths of IDRLoss on the same GPU tensors.  Both are fp32 evaluations of the same
    terms: each value within 1e-5 relative (test_loss_cpu.py's tolerance between two formulations), the two SSIM values within
    twice the golden's scalar bound of one another (each side may use it up), the gradients of the whole loss within 1e-5
    relative L2 (the largest gradient bound of the golden cases is 2.1e-5 for the patch terms alone; the L1 terms' gradients,
    exact in both paths, make up most of the norm here)"""
    c = G.cases[G.names.index('two_holes')]
    wi, ws, wr = (float(w) for w in c['weights'])
    res = []
    for fused in (True, False):
        loss = IDRLoss(r_patch=6, idr_ssim_weight=wi, sg_ssim_weight=ws, roughnesssmooth_weight=wr, **BASE)
        loss.fused = fused
        out, gt = _outputs(c)
        lo = loss(out, gt)
        grads = torch.autograd.grad(lo['loss'], [out['idr_rgb_values'], out['sg_rgb_values'], out['sg_roughness_values']])
        res.append((lo, grads))
    (a, ga), (b, gb) = res
    assert set(a.keys()) == set(b.keys()) == set(G.loss_keys)
    for k in a:
        print(k, a[k].item(), b[k].item())
        if k not in ('idr_ssim_loss', 'sg_ssim_loss'):
            assert abs(a[k].item() - b[k].item()) <= 1e-5 * abs(b[k].item()) + 1e-7, (k, a[k].item(), b[k].item())
    for k in ('idr_ssim_loss', 'sg_ssim_loss'):
        assert a[k].item() > 0 and abs(a[k].item() - b[k].item()) <= 2 * ref.MARGIN * G.scalar_yard
    for x, y in zip(ga, gb):
        e = ref.rel_l2(x.double().cpu().numpy(), y.double().cpu().numpy())
        print('gradient rel L2', e)
        assert e < 1e-5


def test_zero_weights_launch_nothing_new_and_change_nothing():
    """the three weights at 0: the fused result is IdrLossFn's alone, bit for bit"""
    from nefii_amd._lib import LossParams
    c = G.cases[G.names.index('two_holes')]
    out, gt = _outputs(c)
    lo = IDRLoss(r_patch=6, **BASE)(out, gt)
    g = torch.autograd.grad(lo['loss'], [out['idr_rgb_values'], out['sg_rgb_values']])
    assert torch.autograd.grad(lo['loss'], out['sg_roughness_values'], allow_unused=True)[0] is None     # PatchLossFn did not run
    out2, _ = _outputs(c)
    p = LossParams(BASE['idr_rgb_weight'], BASE['sg_rgb_weight'], BASE['mask_weight'], BASE['alpha'], BASE['normalsmooth_weight'],
                   BASE['background_rgb_weight'], 0, 1, 6, 0)
    l2 = ops.IdrLossFn.apply(out2['idr_rgb_values'], out2['sg_rgb_values'], gt['rgb'], out2['network_object_mask'],
                             out2['object_mask'], out2['sdf_output'], out2['normal_values'], p)
    g2 = torch.autograd.grad(l2[0], [out2['idr_rgb_values'], out2['sg_rgb_values']])
    assert torch.equal(lo['loss'], l2[0]) and lo['idr_ssim_loss'].item() == 0 and lo['sg_ssim_loss'].item() == 0
    for k, j in (('idr_rgb_loss', 1), ('sg_rgb_loss', 2), ('mask_loss', 3), ('normalsmooth_loss', 4), ('background_rgb_loss', 5)):
        assert torch.equal(lo[k], l2[j]), k
    assert torch.equal(g[0], g2[0]) and torch.equal(g[1], g2[1])


def test_graph_step_with_patch_terms_matches_eager_step():
    """TrainStep(graph=True) with the patch terms weighted: the captured tail holds PatchLossFn's two launches, and gives the
    eager step's losses and parameters (the pattern and tolerances of test_gpu_renderer.test_graph_step_matches_eager_step).
    Four 12 x 12 patches of neighbouring pixels around the image centre, where every ray hits."""
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    from nefii_amd.training.step import TrainStep
    mc = syn.model_conf('physg', hidden=64)
    sd = syn.make_state_dict(mc, seed=4, bumpy=0.02)
    lc = dict(syn.loss_conf('physg'), idr_rgb_weight=1.0, r_patch=6, idr_ssim_weight=0.5, sg_ssim_weight=0.5,
              roughnesssmooth_weight=1.0)
    yy, xx = np.mgrid[0:12, 0:12]
    uv = np.concatenate([np.stack([x0 + xx, y0 + yy], -1).reshape(-1, 2) for y0 in (20, 32) for x0 in (20, 32)])
    batches = []
    for it in range(3):
        inp, gt = syn.make_inputs(576, (64, 64), 140.0 + 3 * it, (0.2, 0.1, 2.0), -1, seed=30 + it)
        inp['uv'] = torch.from_numpy(uv).to(inp['uv'].dtype)[None]
        batches.append(({k: v.to(DEV) for k, v in inp.items()}, {'rgb': gt.to(DEV)}))
    runs = []
    for graph in (False, True):
        m = IDRNetwork(conf.from_dict(mc))
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV)
        m.freeze_geometry()
        m.train(True)
        m.ray_tracer.minsdf_steps_override = [torch.rand(100, generator=torch.Generator().manual_seed(3)) for _ in range(9)]
        st = TrainStep(m, lc, graph=graph, graph_bucket=64, graph_after=1)
        losses = []
        for inp, gt in batches:
            out, lo = st(inp, gt)
            losses.append({k: v.item() for k, v in lo.items()})
        runs.append((losses, {k: v.detach().clone() for k, v in m.state_dict().items()}, st))
    (l0, p0, _), (l1, p1, st1) = runs
    assert len(st1._graphs) >= 1
    assert all(l['idr_ssim_loss'] > 0 and l['sg_ssim_loss'] > 0 for l in l0), l0       # the erosion left pixels: the terms ran
    for a, b in zip(l0, l1):
        for k in a:
            assert abs(a[k] - b[k]) <= 1e-4 * max(abs(a[k]), 1e-3), (k, a[k], b[k])
    moved = 0
    for k in p0:
        if p0[k].dtype.is_floating_point:
            e = (p1[k].double() - p0[k].double()).norm() / p0[k].double().norm().clamp(min=1e-30)
            assert e < 1e-4, (k, e.item())
            moved += int(not torch.equal(p0[k].cpu(), sd[k]))
    assert moved > 0
