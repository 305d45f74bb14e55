#!/usr/bin/env python3
"""Microseconds per iteration of the SG envmap fit at 256 x 512 directions x 128 lobes (fit_envmap_with_sg.py's size):

    python tools/envfit_microbench.py [--iters 200] [--repeats 5] [--height 256 --width 512 --lobes 128]

  fused_adam      nefii_envfit_adam: `iters` iterations enqueued in one call (two launches each)
  loss_grad       nefii_envfit_loss_grad alone, one call per iteration
  torch_autograd  the reference formulation on the GPU: [H, W, M, 7] expansion, autograd, torch.optim.Adam

HIP events around each batch after a warm-up batch; the median of --repeats batches is reported, with min and max."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sg2envmap_torch(lgt, viewdirs, eps=1e-8):
    """SG2Envmap of fit_envmap_with_sg.py, restated: the expanded [H, W, M, 7] formulation"""
    dots_sh = list(viewdirs.shape[:-1])
    M = lgt.shape[0]
    vd = viewdirs.unsqueeze(-2)
    lgt = lgt.view([1] * len(dots_sh) + [M, 7]).expand(dots_sh + [M, 7])
    lobes = lgt[..., :3] / (torch.norm(lgt[..., :3], dim=-1, keepdim=True) + eps)
    lam, mu = torch.abs(lgt[..., 3:4]), torch.abs(lgt[..., -3:])
    return torch.sum(mu * torch.exp(lam * (torch.sum(vd * lobes, dim=-1, keepdim=True) - 1.)), dim=-2)


def time_batches(fn, iters, repeats):
    fn(iters)                                               # warm-up (allocations, code objects)
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(iters)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)         # us per iteration
    return {'median_us': statistics.median(out), 'min_us': min(out), 'max_us': max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=256)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--lobes', type=int, default=128)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--torch_iters', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    from nefii_amd import ops
    from nefii_amd.lighting import init_light_sgs
    from nefii_amd.training.render import envmap_directions
    dev = torch.device('cuda:0')
    H, W, M = a.height, a.width, a.lobes
    dirs = envmap_directions(H, W).to(dev)
    g = torch.Generator().manual_seed(0)
    target = (torch.rand(H, W, 3, generator=g) * 2).to(dev)
    d2, t2 = dirs.reshape(-1, 3).contiguous(), target.reshape(-1, 3).contiguous()
    n = d2.shape[0]
    lgt0 = init_light_sgs(M, 0).to(dev)
    res = {'H': H, 'W': W, 'lobes': M, 'directions': n}

    lgt, m, v = lgt0.clone(), torch.zeros_like(lgt0), torch.zeros_like(lgt0)
    ws = ops.envfit_workspace(n, M, dev)
    state = {'step': 0}

    def fused(k):
        ops.envfit_adam(lgt, m, v, d2, t2, state['step'], k, workspace=ws)
        state['step'] += k
    res['fused_adam'] = time_batches(fused, a.iters, a.repeats)

    def lossgrad(k):
        for _ in range(k):
            ops.envfit_loss_grad(lgt, d2, t2, workspace=ws)
    res['loss_grad'] = time_batches(lossgrad, a.iters, a.repeats)

    p = torch.nn.Parameter(lgt0.clone())
    opt = torch.optim.Adam([p], lr=1e-2)

    def reference(k):
        for _ in range(k):
            opt.zero_grad()
            env = sg2envmap_torch(p, dirs)
            loss = torch.mean((env - target) * (env - target))
            loss.backward()
            opt.step()
    res['torch_autograd'] = time_batches(reference, a.torch_iters, a.repeats)

    # one iteration's arithmetic: forward + recomputed backward, one exp per (direction, lobe) each
    pairs = n * M
    res['exp_per_iter'] = 2 * pairs
    res['speedup_vs_torch'] = res['torch_autograd']['median_us'] / res['fused_adam']['median_us']
    for k in ('fused_adam', 'loss_grad', 'torch_autograd'):
        print('%-15s %10.1f us/iter  (min %.1f, max %.1f)' % (k, res[k]['median_us'], res[k]['min_us'], res[k]['max_us']))
    print('fused Adam is %.0fx the torch composition' % res['speedup_vs_torch'])
    print(json.dumps(res))
    if not all(math.isfinite(res[k]['median_us']) for k in ('fused_adam', 'loss_grad', 'torch_autograd')):
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
