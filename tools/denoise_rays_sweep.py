#!/usr/bin/env python3
"""What the two denoisers buy per ray count on the fitted bowl, on one GPU:

    python tools/denoise_rays_sweep.py [--res 256] [--ref_rays 1024] [--rays 4,8,16,32,64] [--match_rays 256]
                                       [--level_size 800] [--json out.json]

One view of the bowl (conf.conf net, synthetic.make_state_dict(scene='bowl_trained'), config 5's camera) at --res x --res.  A
reference frame at --ref_rays rays per pixel; then per ray count of --rays the frame with model.pixel_moments on, 6j's filter
(denoise_outputs) and the variance-guided one (denoise_outputs(variance=True)) at their defaults, and against the reference,
over the pixels valid in both, for sg_rgb, diffuse and specular: rel-L2, and the PSNR of the tone-mapped images
(nefii_amd.metrics.psnr, pixels outside the common mask set to 0 in both).  A raw frame at --match_rays gives the error a
frame of that many rays has without any filter.  Render times by a host clock around a synchronise, one run each; the
filters' times (denoise_outputs as a whole, guides included) by HIP events, one warm-up, median of 3 with min and max.
--level_size N (0 skips it): one level of either kernel on an N x N synthetic frame with two signals, per step, timed the
same way.  One JSON line, then a table.  Reads nothing outside the repository."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEYS = (('sg_rgb_values', 'sg_rgb'), ('sg_diffuse_rgb_values', 'diffuse'), ('sg_specular_rgb_values', 'specular'))


def timed(fn, repeats=3):
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
    return {'median': statistics.median(ms), 'min': min(ms), 'max': max(ms)}


def rel_l2(x, ref):
    return ((x.double() - ref.double()).norm() / ref.double().norm()).item()


def errors(out, ref, valid, res):
    """{short key: {'rel_l2', 'psnr'}} of a frame against the reference over `valid`"""
    from nefii_amd import metrics
    tone = lambda t: torch.where(valid[:, None], t.float().clamp_min(0.).pow(1. / 2.2).clamp(0., 1.),
                                 torch.zeros_like(t, dtype=torch.float32)).reshape(res, res, 3).contiguous()
    return {short: {'rel_l2': rel_l2(out[k][valid], ref[k][valid]), 'psnr': metrics.psnr(tone(out[k]), tone(ref[k]))}
            for k, short in KEYS}


def sweep(a, dev):
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.denoise import DEFAULTS, VARIANCE_DEFAULTS, denoise_outputs
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    from nefii_amd.training import render as R
    w = syn.WORKLOADS['cfg5']
    mc = syn.model_conf('conf')
    model = IDRNetwork(conf.from_dict(mc))
    model.load_state_dict(syn.make_state_dict(mc, seed=0, scene='bowl_trained'), strict=True)
    model = model.to(dev).eval()
    model.freeze_geometry()
    model.ray_tracer.trace_tier = os.environ.get('NEFII_TRACE_TIER', '1') != '0'       # as bench.py renders the frame
    res = a.res
    focal = w['focal'] * res / w['image_hw'][0]

    def render(rays, moments):
        inp = {k: v.to(dev) for k, v in syn.frame_inputs((res, res), focal, w['cam_pos'], rays, seed=100 + rays).items()}
        model.pixel_moments = moments
        torch.manual_seed(rays)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frame = R.render_frame(model, inp, res * res, num_rays=rays, memory_capacity_level=w['memory_capacity_level'],
                               extra_keys=(('denoise_signals', 8),) if moments else ())
        torch.cuda.synchronize()
        model.pixel_moments = False
        return frame, time.perf_counter() - t0

    render(2, True)                                                                     # warm-up: every kernel once
    ref, t_ref = render(a.ref_rays, False)
    out = {'res': res, 'ref_rays': a.ref_rays, 'ref_render_s': t_ref, 'defaults_6j': DEFAULTS, 'defaults_variance': VARIANCE_DEFAULTS,
           'valid_share': ref['network_object_mask'].float().mean().item(), 'rays': {}}
    print('reference: %d x %d x %d rays in %.2f s, %.1f %% of the pixels valid' % (res, res, a.ref_rays, t_ref,
                                                                                  100. * out['valid_share']), flush=True)
    if a.match_rays:
        frame, t = render(a.match_rays, False)
        valid = frame['network_object_mask'] & ref['network_object_mask']
        out['match'] = {'rays': a.match_rays, 'render_s': t, 'raw': errors(frame, ref, valid, res)}
    for rays in sorted(int(x) for x in a.rays.split(',') if x):
        frame, t = render(rays, True)
        valid = frame['network_object_mask'] & ref['network_object_mask']
        plain = {k: v for k, v in frame.items() if k != 'denoise_signals'}
        r = {'render_s': t, 'pixels': int(valid.sum()),
             'raw': errors(frame, ref, valid, res),
             '6j': errors(denoise_outputs(plain, (res, res)), ref, valid, res),
             'variance': errors(denoise_outputs(frame, (res, res), variance=True), ref, valid, res),
             '6j_ms': timed(lambda: denoise_outputs(plain, (res, res))),
             'variance_ms': timed(lambda: denoise_outputs(frame, (res, res), variance=True))}
        out['rays'][str(rays)] = r
        print('%4d rays: render %.2f s, sg_rgb rel-L2 raw %.4f, 6j %.4f, variance-guided %.4f' % (
            rays, t, r['raw']['sg_rgb']['rel_l2'], r['6j']['sg_rgb']['rel_l2'], r['variance']['sg_rgb']['rel_l2']), flush=True)
    return out


def levels(a, dev):
    """one level of either kernel on the synthetic frame of tools/denoise_microbench.py, by step"""
    from denoise_microbench import sphere_on_plane
    from nefii_amd import ops
    from nefii_amd.denoise import DEFAULTS, VARIANCE_DEFAULTS, Denoiser
    H = W = a.level_size
    nrm, pts, valid, signals = sphere_on_plane(H, W, dev)
    den = Denoiser(nrm, pts, valid, (H, W))
    src = torch.zeros(2, H * W, 4, device=dev)
    src[:, :, :3] = signals.reshape(2, H * W, 3)
    src4 = src.clone()
    src4[:, :, 3] = (0.25 * (0.2126 * src[:, :, 0] + 0.7152 * src[:, :, 1] + 0.0722 * src[:, :, 2])) ** 2     # relative deviation 0.25
    dst = torch.empty_like(src)
    out = {'size': [H, W], 'signals': 2, 'steps': {}}
    for l in range(DEFAULTS['levels']):
        step = 1 << l
        out['steps'][str(step)] = {
            '6j_ms': timed(lambda: ops.denoise_atrous(den.guides0, den.guides1, src, dst, H, W, step, DEFAULTS['sigma_n'],
                                                      DEFAULTS['sigma_x'], DEFAULTS['sigma_c'] * 2. ** -l)),
            'variance_ms': timed(lambda: ops.denoise_atrous_variance(den.guides0, den.guides1, src4, dst, H, W, step,
                                                                     VARIANCE_DEFAULTS['sigma_n'], VARIANCE_DEFAULTS['sigma_x'],
                                                                     VARIANCE_DEFAULTS['sigma_l']))}
    out['filter_6j_ms'] = timed(lambda: den.filter(src[:, :, :3]))
    out['filter_variance_ms'] = timed(lambda: den.filter_variance(src4))
    R = 32
    rays = [torch.rand(H * W * R, 3, device=dev) + 0.1 for _ in range(3)]
    hit = torch.ones(H * W * R, dtype=torch.bool, device=dev)
    out['moments_%d_rays_ms' % R] = timed(lambda: ops.pixel_moments(rays[0], rays[1], rays[2], hit, R))
    return out


def table(out):
    ms = lambda t: '%.3f [%.3f .. %.3f]' % (t['median'], t['min'], t['max'])
    print('\n| rays | render s | buffer | rel-L2 raw / 6j / variance | PSNR raw / 6j / variance | 6j ms | variance ms |')
    print('|---|---|---|---|---|---|---|')
    for rays, r in out['sweep']['rays'].items():
        for _, short in KEYS:
            print('| %s | %.2f | %s | %.4f / %.4f / %.4f | %.2f / %.2f / %.2f | %s | %s |' % (
                rays, r['render_s'], short, r['raw'][short]['rel_l2'], r['6j'][short]['rel_l2'], r['variance'][short]['rel_l2'],
                r['raw'][short]['psnr'], r['6j'][short]['psnr'], r['variance'][short]['psnr'], ms(r['6j_ms']), ms(r['variance_ms'])))
    m = out['sweep'].get('match')
    if m:
        print('raw frame of %d rays (%.2f s): ' % (m['rays'], m['render_s'])
              + ', '.join('%s rel-L2 %.4f PSNR %.2f' % (short, m['raw'][short]['rel_l2'], m['raw'][short]['psnr']) for _, short in KEYS))
    if 'levels' in out:
        lv = out['levels']
        print('\none level on %d x %d, two signals:\n| step | 6j ms | variance ms |\n|---|---|---|' % tuple(lv['size']))
        for step, t in lv['steps'].items():
            print('| %s | %s | %s |' % (step, ms(t['6j_ms']), ms(t['variance_ms'])))
        print('five levels with packing: 6j %s ms, variance-guided %s ms; pixel_moments at 32 rays %s ms'
              % (ms(lv['filter_6j_ms']), ms(lv['filter_variance_ms']), ms(lv['moments_32_rays_ms'])))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--res', type=int, default=256)
    p.add_argument('--ref_rays', type=int, default=1024)
    p.add_argument('--rays', type=str, default='4,8,16,32,64')
    p.add_argument('--match_rays', type=int, default=256, help='a raw frame of this many rays for comparison (0: none)')
    p.add_argument('--level_size', type=int, default=800, help='side of the frame the per-level timings use (0: none)')
    p.add_argument('--json', type=str, default='')
    a = p.parse_args(argv)
    dev = torch.device('cuda')
    out = {'sweep': sweep(a, dev)}
    if a.level_size:
        out['levels'] = levels(a, dev)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)
    table(out)


if __name__ == '__main__':
    main()
