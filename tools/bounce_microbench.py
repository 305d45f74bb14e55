#!/usr/bin/env python3
"""Timings of the recomputed bounce under a map light on one GPU, by tools/envlight_microbench.py's protocol
(HIP events around each repeat after one warm-up; the median of the repeats, with min and max):

    python tools/bounce_microbench.py [--points 1048576] [--strip_rows 4] [--repeats 5] [--json out.json]

  bounce_ms       nefii_envlight_bounce_sample on --points secondary hits, map 256x512 and 1024x2048
  strip_ms        the strip of config 5's frame that 6g reports (bowl scene, 8 x 512 conf net, 800 x strip_rows pixels x 256
                  rays) under the 256 x 512 map of the model's own light, in mode mlp and in mode bounce, alternating repeat
                  by repeat in this process - and, from one more (untimed) render in mode bounce, the secondary rays, the share of
                  them that hit, and the tertiary rays traced"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from envlight_microbench import lognormal, timed  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--points', type=int, default=1 << 20)
    p.add_argument('--strip_rows', type=int, default=4)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--json', type=str, default='')
    a = p.parse_args(argv)
    from nefii_amd.lighting import EnvmapLight
    dev = torch.device('cuda')
    out = {'bounce': {}}
    n = a.points
    g = torch.Generator(device=dev).manual_seed(1)
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=-1)
    view = torch.nn.functional.normalize(nrm + 0.5 * torch.randn(n, 3, device=dev, generator=g), dim=-1)
    rough = 0.05 + 0.9 * torch.rand(n, 1, device=dev, generator=g)
    albedo = torch.rand(n, 3, device=dev, generator=g)
    uni = torch.rand(n, 3, device=dev, generator=g)
    spec = torch.tensor([0.04, 0.04, 0.04], device=dev)
    for H, W in ((256, 512), (1024, 2048)):
        light = EnvmapLight(lognormal(H, W, dev), 'mitsuba')
        t = timed(lambda: light.bounce_sample(spec, rough, albedo, nrm, view, uni), a.repeats)
        t['GBps'] = n * 4 * (1 + 3 * 4 + 3 * 2) / (t['median'] * 1e-3) / 1e9      # inputs read + wo, weight written
        out['bounce']['%dx%d' % (H, W)] = t
        print('map %4dx%-4d bounce_sample %7.3f ms (%6.1f GB/s of arguments) per %d hits' % (H, W, t['median'], t['GBps'], n),
              flush=True)
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
    light = EnvmapLight.from_sg(model.envmap_material_network.get_lgtSGs().detach(), 256, 512)

    def run():
        with torch.no_grad():
            R.render_frame(model, inp, rows * W, num_rays=rays, memory_capacity_level=w['memory_capacity_level'])
    # the two modes alternate, repeat by repeat, after one warm-up each: a drift of the machine lands on both
    ms = {'mlp': [], 'bounce': []}
    for rep in range(a.repeats + 1):
        for mode in ('mlp', 'bounce'):
            model.set_envmap_light(light, mode)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            if rep > 0:
                ms[mode].append(e0.elapsed_time(e1))
    res = {}
    for mode in ('mlp', 'bounce'):
        res[mode] = {'median': statistics.median(ms[mode]), 'min': min(ms[mode]), 'max': max(ms[mode]), 'n': a.repeats}
        print('strip %d x %d px x %d rays, map 256x512, indirect=%s: %9.1f ms (min %.1f, max %.1f)' % (
            W, rows, rays, mode, res[mode]['median'], res[mode]['min'], res[mode]['max']), flush=True)
    # one more render in mode bounce, counting the rays through the light's two samplers
    counts = {'secondary': 0, 'tertiary': 0}
    sample, bounce = light.sample, light.bounce_sample

    def counted_sample(rough, normal, *rest):
        counts['secondary'] += 3 * normal.shape[0]
        return sample(rough, normal, *rest)

    def counted_bounce(specular, rough, albedo, normal, *rest):
        counts['tertiary'] += normal.shape[0]
        return bounce(specular, rough, albedo, normal, *rest)
    light.sample, light.bounce_sample = counted_sample, counted_bounce
    run()
    torch.cuda.synchronize()
    del light.sample, light.bounce_sample
    model.set_envmap_light(None)
    res.update(counts)
    res['secondary_hit_share'] = counts['tertiary'] / max(counts['secondary'], 1)
    print('secondary rays %d, of which hit %.4f; tertiary rays %d; bounce / mlp = %.3f' % (
        counts['secondary'], res['secondary_hit_share'], counts['tertiary'], res['bounce']['median'] / res['mlp']['median']),
          flush=True)
    return res


if __name__ == '__main__':
    main()
