"""The patch terms of IDRLoss (SSIM of both colours, roughness-smoothness) without a GPU: the fp64 restatement
and the torch formulation against the reference's values in tests/golden/patch_loss.npz, the constructor's refusals, the
zero-weight result and the entry point's host-side checks.

Bounds (patchloss_ref.check_against_golden): the expected values are the reference's fp64 results; the yardstick is the
reference's own fp32 result against them, stored per case.  A gradient's relative L2 may be 8 x its case's yardstick, a
scalar's absolute error 8 x the largest scalar yardstick of the file."""
import ctypes

import numpy as np
import pytest
import torch

import patchloss_ref as ref
from nefii_amd import synthetic as syn
from nefii_amd.model.loss import IDRLoss

G = ref.golden()
CASES = list(range(len(G.names)))
BASE = dict(idr_rgb_weight=1.0, sg_rgb_weight=1.0, eikonal_weight=0.1, mask_weight=100.0, alpha=50.0, normalsmooth_weight=1.0,
            loss_type='L1', env_loss_type='L2', background_rgb_weight=0.5)        # make_patchloss_golden.py: BASE


def test_golden_has_the_cases_the_terms_need():
    assert G.names == ['full', 'two_holes', 'p14_hole', 'cap_smooth', 'centre_holes', 'hole_per_patch', 'rough_r1', 'rough_r2',
                       'empty']
    by = dict(zip(G.names, G.cases))
    for name in ('full', 'two_holes', 'p14_hole', 'cap_smooth', 'hole_per_patch'):
        assert by[name]['eroded'] > 0 and by[name]['terms64'][1] > 0 and by[name]['terms64'][2] > 0
    assert by['centre_holes']['eroded'] == 0 and by['centre_holes']['terms64'][1] == 0       # M = 0 ...
    assert by['centre_holes']['dict64'][G.loss_keys.index('idr_rgb_loss')] > 0              # ... while the rgb term is not
    assert by['hole_per_patch']['terms64'][3] == 0 and not by['hole_per_patch']['g_rough'].any()
    for name in ('rough_r1', 'rough_r2'):
        assert by[name]['terms64'][3] > 0 and by[name]['idr'].shape[0] % 64 != 0
    assert not by['empty']['terms64'].any()
    assert 0 < G.scalar_yard < 1e-6                     # fp32 rounding of numbers below 1


@pytest.mark.parametrize('i', CASES, ids=G.names)
def test_fp64_restatement_matches_the_reference(i):
    """both sides are fp64 evaluations of one formula: 1e-9 relative"""
    c = G.cases[i]
    terms, gi, gs, gr = ref.patch_terms(c['idr'], c['sg'], c['gt'], c['net'], c['obj'], c['rough'], c['normal'],
                                        int(c['r_patch']), c['weights'])
    np.testing.assert_allclose(terms, c['terms64'], rtol=1e-9, atol=1e-15)
    for got, want in ((gi, c['g_idr']), (gs, c['g_sg']), (gr, c['g_rough'].reshape(-1))):
        if want.any():
            assert ref.rel_l2(got, want) < 1e-9
        else:
            assert not got.any()


def _run_idrloss(c, dtype):
    """IDRLoss on a golden case -> (loss dict, roughnesssmooth term, outputs dict with the three leaves)"""
    wi, ws, wr = (float(w) for w in c['weights'])
    loss = IDRLoss(r_patch=int(c['r_patch']), idr_ssim_weight=wi, sg_ssim_weight=ws, roughnesssmooth_weight=wr, **BASE)
    t = lambda k: torch.from_numpy(c[k])
    out = {'idr_rgb_values': t('idr').to(dtype).requires_grad_(True), 'sg_rgb_values': t('sg').to(dtype).requires_grad_(True),
           'sg_roughness_values': t('rough').to(dtype).requires_grad_(True), 'sdf_output': t('sdf').to(dtype),
           'normal_values': t('normal').to(dtype), 'grad_theta': None, 'network_object_mask': t('net'),
           'object_mask': t('obj')}
    lo = loss(out, {'rgb': t('gt').to(dtype).reshape(1, -1, 3)})
    rs = loss.get_roughnesssmooth_loss(out['sg_roughness_values'], out['normal_values'], out['network_object_mask'],
                                       out['object_mask'])
    return loss, lo, rs, out


def check_idrloss(c, dtype, what=''):
    """The whole IDRLoss (torch formulation) with the patch terms weighted, against the golden: the three terms, their
    gradients (of the weighted sum of the three, as the golden stores them), then the whole dict."""
    loss, lo, rs, out = _run_idrloss(c, dtype)
    leaves = [out['idr_rgb_values'], out['sg_rgb_values'], out['sg_roughness_values']]
    wi, ws, wr = (float(w) for w in c['weights'])
    patch = wi * lo['idr_ssim_loss'] + ws * lo['sg_ssim_loss'] + wr * rs
    grads = [(torch.zeros_like(v) if g is None else g).detach().double().numpy()
             for v, g in zip(leaves, torch.autograd.grad(patch, leaves, allow_unused=True, retain_graph=True))]
    terms = np.array([patch.item(), lo['idr_ssim_loss'].item(), lo['sg_ssim_loss'].item(), rs.item()])
    ref.check_against_golden(c, terms, *grads, what=what)
    want = dict(zip(G.loss_keys, c['dict64']))
    for k in ('loss', 'idr_rgb_loss', 'sg_rgb_loss', 'mask_loss', 'normalsmooth_loss', 'background_rgb_loss', 'eikonal_loss',
              'view_diff_loss'):
        assert abs(lo[k].item() - want[k]) <= 1e-5 * abs(want[k]) + 1e-7, (k, lo[k].item(), want[k])   # test_loss_cpu's tolerance
    assert set(lo.keys()) == set(G.loss_keys)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('i', CASES, ids=G.names)
def test_torch_formulation_matches_the_reference(i, dtype):
    check_idrloss(G.cases[i], dtype, what='%s %s' % (G.names[i], dtype))


def test_radiance_colour_stays_attached_for_its_ssim_term():
    """idr_rgb is detached only when neither of its terms is weighted"""
    c = G.cases[G.names.index('full')]
    kw = dict(BASE, idr_rgb_weight=0.0)
    t = lambda k: torch.from_numpy(c[k])
    for wi, attached in ((0.5, True), (0.0, False)):
        out = {'idr_rgb_values': t('idr').requires_grad_(True), 'sg_rgb_values': t('sg').requires_grad_(True),
               'sg_roughness_values': t('rough'), 'sdf_output': t('sdf'), 'normal_values': t('normal'), 'grad_theta': None,
               'network_object_mask': t('net'), 'object_mask': t('obj')}
        lo = IDRLoss(r_patch=6, idr_ssim_weight=wi, sg_ssim_weight=0.25, **kw)(out, {'rgb': t('gt').reshape(1, -1, 3)})
        g = torch.autograd.grad(lo['loss'], out['idr_rgb_values'], allow_unused=True)[0]
        assert (g is not None and g.abs().max() > 0) == attached


def test_constructor_refusals():
    kw = dict(idr_rgb_weight=1.0, sg_rgb_weight=1.0, eikonal_weight=0.1, mask_weight=100.0, alpha=50.0)
    for r in range(1, 6):
        for w in (dict(idr_ssim_weight=0.1), dict(sg_ssim_weight=0.1)):
            with pytest.raises(ValueError, match='r_patch'):
                IDRLoss(r_patch=r, **w, **kw)
        IDRLoss(r_patch=r, roughnesssmooth_weight=1.0, **kw)         # the roughness term has no such limit
    IDRLoss(r_patch=-1, idr_ssim_weight=0.1, **kw)                   # < 1: the patch terms are off, as in the reference
    IDRLoss(r_patch=6, idr_ssim_weight=0.1, sg_ssim_weight=0.1, roughnesssmooth_weight=1.0, **kw)
    IDRLoss(r_patch=20, sg_ssim_weight=0.1, **kw)
    with pytest.raises(NotImplementedError) as e:
        IDRLoss(r_patch=6, view_diff_weight=0.1, idr_ssim_weight=0.1, roughnesssmooth_weight=1.0, **kw)
    msg = str(e.value)
    assert 'view_diff' in msg and 'ssim' not in msg.lower() and 'roughness' not in msg.lower()


def test_zero_weights_equal_the_oracle_loss():
    """with the three weights at 0 the output is what it was (test_loss_cpu.py: equal to oracle.renderer.idr_loss)"""
    from oracle.renderer import idr_loss
    c = G.cases[G.names.index('two_holes')]
    lc = dict(syn.loss_conf('conf'))
    lc['r_patch'] = int(c['r_patch'])
    t = lambda k: torch.from_numpy(c[k])
    out = {'idr_rgb_values': t('idr').requires_grad_(True), 'sg_rgb_values': t('sg').requires_grad_(True),
           'sg_roughness_values': t('rough').requires_grad_(True), 'sdf_output': t('sdf'), 'normal_values': t('normal'),
           'grad_theta': None, 'network_object_mask': t('net'), 'object_mask': t('obj')}
    gt = t('gt').reshape(1, -1, 3)
    a = IDRLoss(**lc)(out, {'rgb': gt})
    b = idr_loss(out, gt, lc)
    for k in ('loss', 'idr_rgb_loss', 'sg_rgb_loss', 'mask_loss', 'normalsmooth_loss', 'background_rgb_loss'):
        assert torch.allclose(a[k], b[k], rtol=1e-5, atol=1e-7), (k, a[k].item(), b[k].item())
    assert a['idr_ssim_loss'].item() == 0 and a['sg_ssim_loss'].item() == 0
    assert torch.autograd.grad(a['loss'], out['sg_roughness_values'], allow_unused=True)[0] is None


def test_entry_point_refuses_on_the_host():
    from nefii_amd import _lib, ops
    lib = _lib.lib()
    assert ctypes.sizeof(_lib.PatchLossParams) == 64          # 3 floats + r_patch + 11 window taps + reserved
    p = ops.patch_loss_params(0.5, 0.25, 2.0, 6)
    assert (np.array(list(p.window), np.float32) == G.window).all()           # the reference's taps, bit for bit
    assert (ops.ssim_loss_window().numpy() == G.window).all()
    one = ctypes.c_void_p(64)                                   # non-NULL: looked at, never read - every call below is refused

    def call(params, n, skip=None):
        args = [one] * 7 + [n] + [one] * 2 + [None, None, None, None]
        if skip is not None:
            args[skip] = None
        return lib.nefii_idr_patch_loss(ctypes.byref(params) if params is not None else None, *args)

    assert call(None, 144) == -1
    for k in (0, 1, 2, 3, 4, 5, 6, 8, 9):                      # each input, the workspace, the losses
        assert call(p, 144, skip=k) == -1, k
    assert call(p, 143) == -2 and call(p, 0) == -2 and call(p, 144 + 72) == -2
    assert lib.nefii_idr_patch_loss_workspace_bytes(ctypes.byref(p), 143) == -2
    assert lib.nefii_idr_patch_loss_workspace_bytes(ctypes.byref(p), 144 * 3) == 3 * 5 * 8
    assert lib.nefii_idr_patch_loss_workspace_bytes(None, 144) == -1
    for r in (-1, 0, 1, 5, 17):                                 # an SSIM weight with r_patch outside 6 .. 16
        for w in ((0.5, 0.0), (0.0, 0.5)):
            q = ops.patch_loss_params(w[0], w[1], 0.0, r)
            assert call(q, 4 * r * r * 2 if r > 0 else 16) == -2, (r, w)
    for r in (0, 17):                                           # the roughness term alone: 1 .. 16
        assert call(ops.patch_loss_params(0.0, 0.0, 1.0, r), 4 * 17 * 17) == -2
    assert lib.nefii_idr_patch_loss_workspace_bytes(ctypes.byref(ops.patch_loss_params(0.0, 0.0, 1.0, 1)), 28) == 7 * 5 * 8
