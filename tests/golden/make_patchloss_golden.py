#!/usr/bin/env python3
"""tests/golden/patch_loss.npz: the patch terms of the REFERENCE's IDRLoss (code/model/loss.py:54-120 ssim_loss_fn, :237-253
get_ssim_loss, :266-276 get_roughnesssmooth_loss) and its whole forward(), on seeded patches (build container only).

    python tests/golden/make_patchloss_golden.py

kornia is not installed here: the stub module ref_shim leaves in its place gets a morphology.erosion of its own - pad the
{0,1} mask with 1, take the minimum over the 11 x 11 window.  That is kornia's DOCUMENTED behaviour for a flat kernel of ones
on a binary mask, not its code: the pinned 0.4.1 pads with 1 (its 'max_val' border), later releases pad geodesically, which for
an erosion is the neutral element again.  Either way what lies outside a patch never erodes.

Every case runs the reference twice on the same fp32 inputs: in fp32 (what the reference trains with) and in fp64.  The fp64
results are the expected values; |fp32 - fp64| is the yardstick the tests scale their bounds by (stored per case).  Stored per
case `c<i>_`: the inputs, the reference's loss dict (fp32 and fp64), the three patch terms and their weighted sum, and the
fp64 gradients of that weighted sum with respect to idr_rgb_values, sg_rgb_values and sg_roughness_values."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

ref_shim.install()


def _erosion(mask, kernel):
    k = kernel.shape[-1]
    padded = F.pad(mask, (k // 2,) * 4, mode='constant', value=1.0)
    return -F.max_pool2d(-padded, k, stride=1)


sys.modules['kornia'].morphology = type(sys)('kornia.morphology')
sys.modules['kornia'].morphology.erosion = _erosion
from model.loss import IDRLoss, _fspecial_gauss_1d  # noqa: E402  (the reference's)

BASE = dict(idr_rgb_weight=1.0, sg_rgb_weight=1.0, eikonal_weight=0.1, mask_weight=100.0, alpha=50.0,
            normalsmooth_weight=1.0, loss_type='L1', env_loss_type='L2', background_rgb_weight=0.5)
SSIM_W = dict(idr_ssim_weight=0.5, sg_ssim_weight=0.25, roughnesssmooth_weight=2.0)
ROUGH_W = dict(idr_ssim_weight=0.0, sg_ssim_weight=0.0, roughnesssmooth_weight=2.0)
LOSS_KEYS = ('loss', 'idr_rgb_loss', 'sg_rgb_loss', 'eikonal_loss', 'mask_loss', 'normalsmooth_loss', 'idr_ssim_loss',
             'sg_ssim_loss', 'view_diff_loss', 'background_rgb_loss')

# (name, r_patch, patches, weights, does the case mean to exercise SSIM)
CASES = [('full', 6, 1, SSIM_W, True), ('two_holes', 6, 5, SSIM_W, True), ('p14_hole', 7, 3, SSIM_W, True),
         ('cap_smooth', 16, 2, SSIM_W, True), ('centre_holes', 6, 2, SSIM_W, False), ('hole_per_patch', 6, 3, SSIM_W, True),
         ('rough_r1', 1, 7, ROUGH_W, False), ('rough_r2', 2, 5, ROUGH_W, False), ('empty', 6, 2, SSIM_W, False)]


def make_inputs(name, r, N, g):
    P = 2 * r
    n = N * P * P
    yy, xx = np.mgrid[0:P, 0:P]
    smooth = np.stack([0.5 + 0.35 * np.sin(xx / (2.0 + p) + c) * np.cos(yy / (3.0 + c) - p) for p in range(N) for c in range(3)])
    smooth = smooth.reshape(N, 3, P, P).transpose(0, 2, 3, 1).reshape(n, 3)
    if name == 'full':                  # plain noise: no structure for the window to follow
        gt, idr, sg = g.random((n, 3)), g.random((n, 3)), g.random((n, 3))
    else:
        amp = 0.02 if name == 'cap_smooth' else 0.08
        gt = smooth + g.normal(0, amp, (n, 3))
        idr = 0.9 * smooth + 0.03 + g.normal(0, amp, (n, 3))
        sg = smooth ** 1.2 + g.normal(0, 1.5 * amp, (n, 3))
    rough = 0.3 + 0.2 * smooth[:, :1] + g.normal(0, 0.05, (n, 1))
    normal = g.normal(0, 0.15, (n, 3)) + np.array([0.2, -0.1, 1.0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    sdf = g.normal(0, 0.05, (n, 1))
    net, obj = np.ones((N, P, P), bool), np.ones((N, P, P), bool)
    if name == 'two_holes':
        net[1, 3, 8] = False
        obj[3, 7, 2] = False
    elif name == 'p14_hole':
        obj[2, 6, 9] = False
    elif name == 'centre_holes':
        net[:, 5, 5] = net[:, 6, 6] = False
        obj[:, 5, 6] = obj[:, 6, 5] = False
    elif name == 'hole_per_patch':
        net[0, 0, 1] = obj[1, 11, 4] = net[2, 9, 10] = False
    elif name == 'rough_r1':
        net[2, 0, 1] = obj[5, 1, 1] = False
    elif name == 'rough_r2':
        obj[0, 3, 0] = net[3, 1, 2] = False
    elif name == 'empty':
        net[:] = False
        obj[:] = g.random(obj.shape) < 0.5
    f32 = lambda a: np.clip(a, 0.0, 1.0).astype(np.float32)
    return {'idr': f32(idr), 'sg': f32(sg), 'gt': f32(gt), 'rough': f32(rough), 'normal': normal.astype(np.float32),
            'sdf': sdf.astype(np.float32), 'net': net.reshape(n), 'obj': obj.reshape(n)}


def run_reference(inp, r, weights, dtype):
    loss = IDRLoss(r_patch=r, **BASE, **weights)
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    leaves = {k: t[k].to(dtype).requires_grad_(True) for k in ('idr', 'sg', 'rough')}
    out = {'idr_rgb_values': leaves['idr'], 'sg_rgb_values': leaves['sg'], 'sg_roughness_values': leaves['rough'],
           'sdf_output': t['sdf'].to(dtype), 'normal_values': t['normal'].to(dtype), 'grad_theta': None,
           'network_object_mask': t['net'], 'object_mask': t['obj']}
    gt = t['gt'].to(dtype).reshape(1, -1, 3)
    res = {k: v.detach().double().numpy() for k, v in loss(out, {'rgb': gt}).items()}
    i_ssim, s_ssim = loss.get_ssim_loss(leaves['idr'], leaves['sg'], gt, t['net'], t['obj'])
    rs = loss.get_roughnesssmooth_loss(leaves['rough'], out['normal_values'], t['net'], t['obj'])
    patch = weights['idr_ssim_weight'] * i_ssim + weights['sg_ssim_weight'] * s_ssim + weights['roughnesssmooth_weight'] * rs
    grads = {}
    for k, v in leaves.items():
        gr = torch.autograd.grad(patch, v, retain_graph=True, allow_unused=True)[0] if patch.requires_grad else None
        grads[k] = (torch.zeros_like(v) if gr is None else gr).double().numpy()
    terms = np.array([float(patch), float(i_ssim), float(s_ssim), float(rs)])
    return res, terms, grads


def eroded_count(inp, r):
    P = 2 * r
    m = torch.from_numpy(inp['net'] & inp['obj']).float().reshape(-1, 1, P, P)
    return int((_erosion(m, torch.ones(11, 11)) > 0.5).sum()) if P >= 11 else 0


def rel_l2(a, b):
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / den) if den > 0 else float(np.abs(a).max())


def main():
    g = np.random.Generator(np.random.Philox(23))
    out = {'names': np.array([c[0] for c in CASES])}
    for i, (name, r, N, weights, wants_ssim) in enumerate(CASES):
        inp = make_inputs(name, r, N, g)
        M = eroded_count(inp, r)
        assert (M > 0) == wants_ssim, (name, M)
        res32, terms32, grads32 = run_reference(inp, r, weights, torch.float32)
        res64, terms64, grads64 = run_reference(inp, r, weights, torch.float64)
        pre = 'c%d_' % i
        for k, v in inp.items():
            out[pre + k] = v
        out[pre + 'r_patch'] = np.int64(r)
        out[pre + 'weights'] = np.array([weights[k] for k in ('idr_ssim_weight', 'sg_ssim_weight', 'roughnesssmooth_weight')])
        out[pre + 'eroded'] = np.int64(M)
        out[pre + 'dict32'] = np.array([res32[k] for k in LOSS_KEYS])
        out[pre + 'dict64'] = np.array([res64[k] for k in LOSS_KEYS])
        out[pre + 'terms32'], out[pre + 'terms64'] = terms32, terms64       # weighted sum, idr_ssim, sg_ssim, roughnesssmooth
        for k in ('idr', 'sg', 'rough'):
            out[pre + 'g_' + k] = grads64[k]
        out[pre + 'g_yard'] = np.array([rel_l2(grads32[k], grads64[k]) for k in ('idr', 'sg', 'rough')])
        print(name, 'M = %d / %d' % (M, inp['net'].size), 'terms64', terms64, 'scalar yardstick', np.abs(terms32 - terms64),
              'gradient yardstick', out[pre + 'g_yard'])
    out['loss_keys'] = np.array(LOSS_KEYS)
    out['window'] = _fspecial_gauss_1d(11, 1.5).reshape(-1).numpy()          # fp32, as ssim_loss_fn forms it
    np.savez_compressed(os.path.join(HERE, 'patch_loss.npz'), **out)
    print(os.path.getsize(os.path.join(HERE, 'patch_loss.npz')), 'bytes')


if __name__ == '__main__':
    main()
