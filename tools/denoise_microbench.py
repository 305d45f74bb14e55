#!/usr/bin/env python3
"""The a-trous denoiser's timings and what it buys on one GPU:

    python tools/denoise_microbench.py [--size 800] [--repeats 5] [--frames 16,32,256] [--variance] [--json out.json]

  level_ms    nefii_denoise_atrous per level (step 1 .. 16) on a --size x --size frame with two signals, and the five levels
              together, set against the byte model: 25 taps x 64 B per pixel and level read through the caches, and
              (2 guides + 2 signals read, 2 signals written) x 16 B per pixel of unique traffic per level; --variance: the
              same of nefii_denoise_atrous_variance and Denoiser.filter_variance, with its 3 x 3 prefilter's
              9 x 48 B per pixel among the taps
  frames      config 5's frame (bowl scene, conf.conf net, 800 x 800, focal 1111) at each ray count of --frames through
              training/render.render_frame, the time of denoise_outputs on it, and - against the frame of the highest ray
              count - the rel-L2 error of sg_rgb over the pixels valid in both, raw and denoised (--frames '' skips this)

HIP events around each repeat after one warm-up; the median of the repeats, with min and max.  Frames are timed once, by a
host clock around a device synchronise."""
import argparse
import json
import os
import statistics
import sys
import time

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


def sphere_on_plane(H, W, dev, seed=0):
    """guides and two noisy signals of an orthographic sphere on a tilted plane (the scene of tests/denoise_ref.py, in torch)"""
    torch.manual_seed(seed)
    v, u = torch.meshgrid((torch.arange(H) + 0.5) / H * 2. - 1., (torch.arange(W) + 0.5) / W * 2. - 1., indexing='ij')
    r2 = u * u + v * v
    on = r2 < 0.45 ** 2
    zs = (0.45 ** 2 - r2).clamp_min(0.).sqrt()
    z = torch.where(on, zs, -0.6 + 0.3 * u + 0.2 * v)
    plane = torch.nn.functional.normalize(torch.tensor([-0.3, -0.2, 1.]), dim=0)
    nrm = torch.where(on[..., None], torch.stack([u, v, zs], -1) / 0.45, plane.expand(H, W, 3))
    valid = torch.ones(H, W, dtype=torch.bool)
    valid[:H // 12] = False
    light = torch.nn.functional.normalize(torch.tensor([0.3, 0.5, 0.8]), dim=0)
    lambert = (nrm @ light).clamp_min(0.)[..., None] * torch.tensor([1.0, 0.8, 0.6]) + 0.1
    glossy = ((nrm @ torch.nn.functional.normalize(light + torch.tensor([0., 0., 1.]), dim=0)).clamp_min(0.) ** 20)[..., None] + 0.05
    signals = torch.stack([lambert, glossy.expand(H, W, 3)])
    noise = torch.distributions.Gamma(4., 4.).sample(signals.shape)                     # mean 1, relative deviation 0.5
    return nrm.reshape(-1, 3).to(dev), torch.stack([u, v, z], -1).reshape(-1, 3).to(dev), valid.reshape(-1).to(dev), \
        (signals * noise).to(dev)


def levels(a, dev):
    from nefii_amd import ops
    from nefii_amd.denoise import DEFAULTS, VARIANCE_DEFAULTS, Denoiser
    H = W = a.size
    nrm, pts, valid, signals = sphere_on_plane(H, W, dev)
    den = Denoiser(nrm, pts, valid, (H, W))
    tap_bytes, unique = 25 * 64 * H * W, 6 * 16 * H * W
    if a.variance:      # the same frame with a plausible variance of the mean in the fourth lane: (0.5 luminance)^2 / 32
        lum = (signals * signals.new_tensor([0.2126, 0.7152, 0.0722])).sum(-1, keepdim=True)
        signals = torch.cat([signals, (0.5 * lum) ** 2 / 32.], dim=-1)
        src = signals.reshape(2, H * W, 4).contiguous()
        tap_bytes += 9 * 48 * H * W                     # the 3 x 3 prefilter: one guide and two signal elements per pixel
        P = VARIANCE_DEFAULTS
        level = lambda l: ops.denoise_atrous_variance(den.guides0, den.guides1, src, dst, H, W, 1 << l, P['sigma_n'],
                                                      P['sigma_x'], P['sigma_l'])
        whole, name = (lambda: den.filter_variance(signals)), 'Denoiser.filter_variance'
    else:
        src = torch.zeros(2, H * W, 4, device=dev)
        src[:, :, :3] = signals.reshape(2, H * W, 3)
        P = DEFAULTS
        level = lambda l: ops.denoise_atrous(den.guides0, den.guides1, src, dst, H, W, 1 << l, P['sigma_n'], P['sigma_x'],
                                             P['sigma_c'] * 2. ** -l)
        whole, name = (lambda: den.filter(signals)), 'Denoiser.filter'
    dst = torch.empty_like(src)
    out = {'size': [H, W], 'signals': 2, 'variance': bool(a.variance)}
    for l in range(P['levels']):
        t = timed(lambda: level(l), a.repeats)
        t['tap_GBps'] = tap_bytes / (t['median'] * 1e-3) / 1e9
        t['unique_GBps'] = unique / (t['median'] * 1e-3) / 1e9
        out['step_%d' % (1 << l)] = t
        print('level %d (step %2d): %7.3f ms [%.3f .. %.3f]  taps %7.1f GB/s through the caches, unique traffic %6.1f GB/s '
              '(%.1f %% of the HBM peak)' % (l, 1 << l, t['median'], t['min'], t['max'], t['tap_GBps'], t['unique_GBps'],
                                             100. * t['unique_GBps'] * 1e9 / HBM_PEAK), flush=True)
    t = timed(whole, a.repeats)
    out['filter_5_levels'] = t
    print('%s, 5 levels with packing: %7.3f ms [%.3f .. %.3f]; byte model per level: %.1f MB of taps, %.1f MB '
          'unique' % (name, t['median'], t['min'], t['max'], tap_bytes / 1e6, unique / 1e6), flush=True)
    return out


def rel_l2(x, ref):
    return ((x.double() - ref.double()).norm() / ref.double().norm()).item()


def frames(a, dev):
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.denoise import denoise_outputs
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    from nefii_amd.training import render as R
    counts = sorted(int(x) for x in a.frames.split(',') if x)
    if not counts:
        return {}
    w = syn.WORKLOADS['cfg5']
    mc, sd = syn.workload_state_dict('cfg5', seed=0)
    model = IDRNetwork(conf.from_dict(mc))
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    model.freeze_geometry()
    model.ray_tracer.trace_tier = os.environ.get('NEFII_TRACE_TIER', '1') != '0'       # as bench.py renders the frame
    H, W = w['image_hw']
    res, kept = {}, {}
    for rays in counts:
        inp = {k: v.to(dev) for k, v in syn.frame_inputs(w['image_hw'], w['focal'], w['cam_pos'], rays, seed=100 + rays).items()}
        warm = {'uv': inp['uv'][:, :2048].contiguous(), 'object_mask': inp['object_mask'][:, :2048].contiguous(),
                'pose': inp['pose'], 'intrinsics': inp['intrinsics']}
        R.render_frame(model, warm, 2048, num_rays=rays, memory_capacity_level=w['memory_capacity_level'])
        torch.cuda.synchronize()
        torch.manual_seed(rays)
        t0 = time.perf_counter()
        frame = R.render_frame(model, inp, H * W, num_rays=rays, memory_capacity_level=w['memory_capacity_level'])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        den = denoise_outputs(frame, (H, W))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res[str(rays)] = {'render_s': t1 - t0, 'denoise_s': t2 - t1,
                          'valid_share': frame['network_object_mask'].float().mean().item()}
        kept[rays] = (frame, den)
        print('frame %d x %d x %3d rays: render %7.2f s, denoise_outputs %.4f s (first call)' % (H, W, rays, t1 - t0, t2 - t1),
              flush=True)
    top = counts[-1]
    ref = kept[top][0]
    for rays in counts[:-1]:
        frame, den = kept[rays]
        valid = frame['network_object_mask'] & ref['network_object_mask']
        r = res[str(rays)]
        for k in ('sg_rgb_values', 'sg_diffuse_rgb_values', 'sg_specular_rgb_values'):
            r[k] = {'raw': rel_l2(frame[k][valid], ref[k][valid]), 'denoised': rel_l2(den[k][valid], ref[k][valid])}
        e = r['sg_rgb_values']
        print('%3d rays against %d rays over %d pixels valid in both: sg_rgb rel-L2 raw %.4f, denoised %.4f (ratio %.3f); '
              'diffuse %.4f -> %.4f, specular %.4f -> %.4f' % (
                  rays, top, int(valid.sum()), e['raw'], e['denoised'], e['denoised'] / e['raw'],
                  r['sg_diffuse_rgb_values']['raw'], r['sg_diffuse_rgb_values']['denoised'],
                  r['sg_specular_rgb_values']['raw'], r['sg_specular_rgb_values']['denoised']), flush=True)
    return res


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--size', type=int, default=800)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--frames', type=str, default='16,32,256')
    p.add_argument('--variance', default=False, action='store_true',
                   help="time the variance-guided level and Denoiser.filter_variance (DESIGN.md 6q) in place of 6j's")
    p.add_argument('--json', type=str, default='')
    a = p.parse_args(argv)
    dev = torch.device('cuda')
    out = {'levels': levels(a, dev)}
    out['frames'] = frames(a, dev)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
