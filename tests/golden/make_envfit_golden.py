#!/usr/bin/env python3
"""tests/golden/envfit_ref.npz: the reference's spherical-Gaussian envmap fit (envmaps/fit_envmap_with_sg.py) on the
sunrise map, for tests/test_envfit_cpu.py and tests/test_gpu_envfit.py (build container only: reads the reference).

    python tests/golden/make_envfit_golden.py

The objective is restated here (fp64 for the loss / gradient, fp32 for the Adam curve); its forward pass is
cross-checked against the reference's importable model/sg_render.compute_envmap, which normalises the lobe axes
without the fit script's epsilon.  Stored:
    target        sunrise.exr (first 3 channels), 512 x 1024 box-averaged to 64 x 128 (= cv2.INTER_AREA at factor 8)
    init          [128, 7] float32: randn (torch.Generator seed 0) with the sharpness column x 100, the fit's init
    loss64, grad64  fp64 loss and gradient at init (blender convention's fp32 grid, eps 1e-8)
    curve_steps, curve  the loss before update k+1 of float32 autograd + torch.optim.Adam(lr=1e-2) from init
    ref_sg, ref_loss    the reference's own sunrise/sg_128.npy and its fp64 loss on this target (for information)
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

REF_ENVMAPS = os.path.join(ref_shim.REF_ROOT, 'envmaps')
H, W, M, EPS = 64, 128, 128, 1e-8
CURVE_STEPS = [0, 10, 100, 1000, 3000]


def blender_dirs(h, w, dtype):
    phi, theta = torch.meshgrid([torch.linspace(0., math.pi, h, dtype=dtype),
                                 torch.linspace(math.pi, -math.pi, w, dtype=dtype)], indexing='ij')
    return torch.stack([torch.cos(theta) * torch.sin(phi), torch.sin(theta) * torch.sin(phi), torch.cos(phi)], -1)


def sg_envmap(lgt, dirs, eps=EPS):
    """sum_m |mu_m| exp(|lambda_m| (d . v_m / (|v_m| + eps) - 1)) over dirs [..., 3]"""
    a = lgt[:, :3] / (torch.norm(lgt[:, :3], dim=-1, keepdim=True) + eps)
    e = torch.exp(lgt[:, 3].abs() * (dirs @ a.T - 1.))            # [..., M]
    return e @ lgt[:, 4:].abs()


def main():
    from nefii_amd.utils import exr
    full = exr.imread(os.path.join(REF_ENVMAPS, 'sunrise.exr'))[..., :3].astype(np.float64)
    fh, fw = full.shape[:2]
    target = full.reshape(H, fh // H, W, fw // W, 3).mean(axis=(1, 3)).astype(np.float32)
    init = torch.randn(M, 7, generator=torch.Generator().manual_seed(0))
    init[:, 3:4] *= 100.

    ref_shim.install()
    from model.sg_render import compute_envmap  # noqa: E402  (reference)
    ref = compute_envmap(lgtSGs=init.double(), H=H, W=W, log=False, coordinate_type='blender').numpy()
    own = sg_envmap(init.double(), blender_dirs(H, W, torch.float32).double(), eps=0.).numpy()   # its grid is fp32
    rel = np.abs(own - ref).max() / np.abs(ref).max()
    assert rel < 1e-12, rel
    print('forward matches model/sg_render.compute_envmap: max rel %.2e' % rel)

    t64 = torch.from_numpy(target).double()
    d64 = blender_dirs(H, W, torch.float32).double()      # the fp32 grid the fit runs on, evaluated in fp64
    p = init.double().clone().requires_grad_(True)
    loss64 = torch.mean((sg_envmap(p, d64) - t64) ** 2)
    loss64.backward()
    grad64 = p.grad.numpy()

    t32, d32 = torch.from_numpy(target), blender_dirs(H, W, torch.float32)
    p = torch.nn.Parameter(init.clone())
    opt = torch.optim.Adam([p], lr=1e-2)
    curve = []
    for step in range(CURVE_STEPS[-1] + 1):
        opt.zero_grad()
        loss = torch.mean((sg_envmap(p, d32) - t32) ** 2)
        if step in CURVE_STEPS:
            curve.append(loss.item())
            print('step %d loss %.6g' % (step, curve[-1]), flush=True)
        if step == CURVE_STEPS[-1]:
            break
        loss.backward()
        opt.step()

    ref_sg = np.load(os.path.join(REF_ENVMAPS, 'sunrise', 'sg_128.npy')).astype(np.float32)
    with torch.no_grad():
        ref_loss = torch.mean((sg_envmap(torch.from_numpy(ref_sg).double(), d64) - t64) ** 2).item()
    print('reference sg_128.npy on this target: loss %.6g' % ref_loss)
    np.savez_compressed(os.path.join(HERE, 'envfit_ref.npz'), target=target, init=init.numpy(),
                        loss64=np.float64(loss64.item()), grad64=grad64, curve_steps=np.array(CURVE_STEPS),
                        curve=np.array(curve), ref_sg=ref_sg, ref_loss=np.float64(ref_loss), eps=np.float64(EPS))


if __name__ == '__main__':
    main()
