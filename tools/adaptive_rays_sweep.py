#!/usr/bin/env python3
"""What adaptive sampling buys per ray budget on the fitted bowl, on one GPU:

    python tools/adaptive_rays_sweep.py [--res 256] [--ref_rays 1024] [--rays 8,16,32,64] [--json out.json]

One view of the bowl (conf.conf net, synthetic.make_state_dict(scene='bowl_trained'), config 5's camera) at --res x --res.  A
reference frame at --ref_rays rays per pixel; then per budget of --rays the uniform frame (render_frame) and the adaptive frame
(adaptive.render_frame_adaptive at the command line's defaults: pilot max(2, rays // 4), at most 4 x rays per pixel, epsilon 0.01,
dilated), each with its relative MSE mean(((x - ref) / (ref + 0.01))^2) of sg_rgb against the reference over the whole frame,
its time by HIP events around the whole frame loop (one run each, after a warm-up frame of both kinds), and for the adaptive
frame the rounds, lambda, the rays traced and the share of pixels at the floor (the pilot alone) and at the cap.  One JSON
line, then a table.  Reads nothing outside the repository."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rel_mse(x, ref, eps=0.01):
    return (((x.double() - ref.double()) / (ref.double() + eps)) ** 2).mean().item()


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b) / 1000.


def sweep(a, dev):
    from nefii_amd import adaptive, conf, synthetic as syn
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
    level = w['memory_capacity_level']
    centres = {k: v.to(dev) for k, v in syn.frame_inputs((res, res), focal, w['cam_pos'], -1).items()}

    def uniform(rays, seed):
        inp = {k: v.to(dev) for k, v in syn.frame_inputs((res, res), focal, w['cam_pos'], rays, seed=seed).items()}
        torch.manual_seed(seed)
        return event_timed(lambda: R.render_frame(model, inp, res * res, num_rays=rays, memory_capacity_level=level))

    def adaptive_frame(rays, seed):
        torch.manual_seed(seed)
        return event_timed(lambda: adaptive.render_frame_adaptive(model, centres, res * res, (res, res), budget=rays,
                                                                  memory_capacity_level=level))

    uniform(2, 1), adaptive_frame(8, 1)                                                 # warm-up: every kernel once
    ref, t_ref = uniform(a.ref_rays, 100 + a.ref_rays)
    ref_rgb = ref['sg_rgb_values']
    out = {'res': res, 'ref_rays': a.ref_rays, 'ref_render_s': t_ref, 'defaults': adaptive.DEFAULTS,
           'hit_share': ref['network_object_mask'].float().mean().item(), 'rays': {}}
    print('reference: %d x %d x %d rays in %.2f s, %.1f %% of the pixels on the object' % (res, res, a.ref_rays, t_ref,
                                                                                         100. * out['hit_share']), flush=True)
    for rays in sorted(int(x) for x in a.rays.split(',') if x):
        uni, t_u = uniform(rays, 100 + rays)
        ada, t_a = adaptive_frame(rays, 200 + rays)
        meta = ada['meta']
        k = ada['adaptive_rays'] // meta['pilot_rays']
        r = {'uniform_rel_mse': rel_mse(uni['sg_rgb_values'], ref_rgb), 'adaptive_rel_mse': rel_mse(ada['sg_rgb_values'], ref_rgb),
             'uniform_s': t_u, 'adaptive_s': t_a, 'pilot_rays': meta['pilot_rays'], 'max_rays': meta['max_rays'],
             'rounds': meta['rounds'], 'lam': meta['lam'], 'rays_traced': meta['rays_traced'], 'uniform_rays_traced': rays * res * res,
             'floor_share': (k == 1).float().mean().item(), 'cap_share': (k == meta['max_rays'] // meta['pilot_rays']).float().mean().item(),
             'active_pixels': meta['active_pixels']}
        r['ratio'] = r['adaptive_rel_mse'] / r['uniform_rel_mse']
        out['rays'][str(rays)] = r
        print('%4d rays: relative MSE uniform %.5f adaptive %.5f (ratio %.3f); %.2f s against %.2f s; %d rounds, floor %.3f, cap %.3f'
              % (rays, r['uniform_rel_mse'], r['adaptive_rel_mse'], r['ratio'], t_u, t_a, r['rounds'], r['floor_share'],
                 r['cap_share']), flush=True)
    return out


def table(out):
    print('\n| budget | pilot / cap | rel. MSE uniform | rel. MSE adaptive | ratio | uniform s | adaptive s | rounds | floor | cap |')
    print('|---|---|---|---|---|---|---|---|---|---|')
    for rays, r in out['rays'].items():
        print('| %s | %d / %d | %.5f | %.5f | %.3f | %.2f | %.2f | %d | %.3f | %.3f |' % (
            rays, r['pilot_rays'], r['max_rays'], r['uniform_rel_mse'], r['adaptive_rel_mse'], r['ratio'], r['uniform_s'],
            r['adaptive_s'], r['rounds'], r['floor_share'], r['cap_share']))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--res', type=int, default=256)
    p.add_argument('--ref_rays', type=int, default=1024)
    p.add_argument('--rays', type=str, default='8,16,32,64')
    p.add_argument('--json', type=str, default='')
    a = p.parse_args(argv)
    out = sweep(a, torch.device('cuda'))
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)
    table(out)


if __name__ == '__main__':
    main()
