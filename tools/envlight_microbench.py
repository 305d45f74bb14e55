#!/usr/bin/env python3
"""Map-light timings on one GPU:

    python tools/envlight_microbench.py [--points 1048576] [--strip_rows 4] [--repeats 5] [--json out.json]

  build_ms        nefii_envlight_build at 256x512, 1024x2048, 2048x4096, and bytes moved / time
  mis_ms          nefii_envlight_mis_sample on --points surface points, map 256x512 and 1024x2048
  radiance_ms     nefii_envlight_radiance on as many directions
  sg_mis_ms       nefii_mis_sample + nefii_env_radiance_forward (the SG path's sampler and light) at 128 and 512 lobes
  strip_ms        a strip of config 5's frame (bowl scene, 8 x 512 conf net, 800 x 800 at focal 1111, 256 rays per pixel)
                  rendered under a 128-lobe SG light and under its 256 x 512 map (EnvmapLight.from_sg)

HIP events around each repeat after one warm-up; the median of the repeats, with min and max."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median': statistics.median(ms), 'min': min(ms), 'max': max(ms), 'n': repeats}


def lognormal(H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.exp(torch.randn(H, W, 3, generator=g) * 1.5).to(dev)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--points', type=int, default=1 << 20)
    p.add_argument('--strip_rows', type=int, default=4)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--json', type=str, default='')
    a = p.parse_args(argv)
    from nefii_amd import ops
    from nefii_amd.lighting import EnvmapLight
    dev = torch.device('cuda')
    out = {'build': {}, 'mis': {}, 'radiance': {}, 'sg_mis': {}}
    for H, W in ((256, 512), (1024, 2048), (2048, 4096)):
        env = lognormal(H, W, dev)
        t = timed(lambda: ops.envlight_table(env), a.repeats)
        moved = H * W * 12 + H * W * 4 + H * 4 + H * 8 * 2          # map read, C written, M written, row sums
        t['GBps'] = moved / (t['median'] * 1e-3) / 1e9
        out['build']['%dx%d' % (H, W)] = t
        print('build %4dx%-4d %8.3f ms  %7.1f GB/s' % (H, W, t['median'], t['GBps']), flush=True)
    n = a.points
    g = torch.Generator(device=dev).manual_seed(1)
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=-1)
    view = torch.nn.functional.normalize(nrm + 0.5 * torch.randn(n, 3, device=dev, generator=g), dim=-1)
    rough = 0.05 + 0.9 * torch.rand(n, 1, device=dev, generator=g)
    uni = torch.rand(n, 7, device=dev, generator=g)
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=-1)
    for H, W in ((256, 512), (1024, 2048)):
        light = EnvmapLight(lognormal(H, W, dev), 'mitsuba')
        t = timed(lambda: light.sample(rough, nrm, view, uni), a.repeats)
        out['mis']['%dx%d' % (H, W)] = t
        r = timed(lambda: light.radiance(dirs), a.repeats)
        r['GBps'] = n * (12 + 12) / (r['median'] * 1e-3) / 1e9            # dirs read + rgb written (texel reads cached)
        out['radiance']['%dx%d' % (H, W)] = r
        print('map %4dx%-4d mis_sample %7.3f ms  radiance %7.3f ms (%6.1f GB/s) per %d points' % (
            H, W, t['median'], r['median'], r['GBps'], n), flush=True)
    for M in (128, 512):
        gl = torch.Generator().manual_seed(2)
        lgt = torch.randn(M, 7, generator=gl)
        lgt[:, 3] = lgt[:, 3].abs() * 50
        lgt = lgt.to(dev)

        def sg():
            wi, own, tab = ops.mis_sample(lgt, rough, nrm, view, uni)
            ops.EnvRadianceFn.apply(lgt, wi.reshape(-1, 3), 1e-6)
        t = timed(sg, a.repeats)
        out['sg_mis'][str(M)] = t
        print('SG %3d lobes: mis_sample + env_radiance %8.3f ms per %d points' % (M, t['median'], n), flush=True)
    out['strip'] = strip(a, dev)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


def strip(a, dev):
    """config 5's frame, rows 400 - strip_rows/2 .. : 800 x strip_rows pixels x 256 rays, as render_frame chunks it"""
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.lighting import EnvmapLight
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    from nefii_amd.training import render as R
    w = syn.WORKLOADS['cfg5']
    mc = syn.model_conf('conf')
    model = IDRNetwork(conf.from_dict(mc))
    model.load_state_dict(syn.make_state_dict(mc, seed=0, scene=w['scene']), strict=True)
    model = model.to(dev)
    model.freeze_geometry()
    model.eval()
    H, W = w['image_hw']
    rows, rays = a.strip_rows, w['num_rays']
    y, x = np.meshgrid(np.arange(rows) + H // 2 - rows // 2, np.arange(W), indexing='ij')
    g = np.random.Generator(np.random.Philox(0))
    uv = np.stack([x, y], -1).reshape(-1, 1, 2) + g.uniform(-0.5, 0.5, size=(rows * W, rays, 2))
    K = np.eye(4)
    K[0, 0] = K[1, 1] = w['focal']
    K[0, 2], K[1, 2] = W / 2., H / 2.
    f = lambda t: torch.from_numpy(np.asarray(t, np.float32)).to(dev)
    inp = {'uv': f(uv)[None], 'intrinsics': f(K)[None], 'pose': f(syn.look_at_origin_pose(w['cam_pos']))[None],
           'object_mask': torch.ones(1, rows * W, dtype=torch.bool, device=dev)}
    res = {}
    lgt = model.envmap_material_network.get_lgtSGs().detach()
    for name, light in (('sg_%d_lobes' % lgt.shape[0], None), ('map_256x512', EnvmapLight.from_sg(lgt, 256, 512))):
        model.set_envmap_light(light)

        def run():
            with torch.no_grad():
                R.render_frame(model, inp, rows * W, num_rays=rays, memory_capacity_level=w['memory_capacity_level'])
        t = timed(run, max(1, a.repeats // 2))
        res[name] = t
        print('strip %d x %d px x %d rays, %s: %9.1f ms' % (W, rows, rays, name, t['median']), flush=True)
    model.set_envmap_light(None)
    return res


if __name__ == '__main__':
    main()
