#!/usr/bin/env python3
"""Timings of the light turntable on one GPU, by tools/envlight_microbench.py's protocol (HIP events around
each repeat after one warm-up; the median of the repeats, with min and max):

    python tools/turntable_microbench.py [--points 1048576] [--angles 24] [--strip_rows 4] [--repeats 5]
                                         [--steps sampler,strip_mlp,strip_bounce] [--json out.json]

  sampler        nefii_envlight_mis_sample_rot on --points surface points x --angles rotations in ONE launch, against
                 --angles calls of nefii_envlight_mis_sample, on 256 x 512 and 1024 x 2048 maps
  strip_mlp      the strip of config 5's frame that 6g reports (bowl scene, 8 x 512 conf net, 800 x strip_rows pixels x 256
                 rays, the 256 x 512 map of the model's own light) as a turntable of --angles angles (render_turntable),
                 against --angles standalone render_frame calls - the code path of a render before the turntable existed,
                 whose cost does not depend on the angle - alternating repeat by repeat; and the secondary rays each traces
  strip_bounce   the same in indirect mode 'bounce'

Every step runs in a child process of its own under its own time limit (--step_timeout seconds), one after the other; a
step that fails or runs out of time ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from envlight_microbench import lognormal, timed  # noqa: E402

STEPS = ('sampler', 'strip_mlp', 'strip_bounce')


def sampler(a, dev):
    from nefii_amd.lighting import EnvmapLight, turntable_rotations
    n, A = a.points, a.angles
    g = torch.Generator(device=dev).manual_seed(1)
    nrm = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=-1)
    view = torch.nn.functional.normalize(nrm + 0.5 * torch.randn(n, 3, device=dev, generator=g), dim=-1)
    rough = 0.05 + 0.9 * torch.rand(n, 1, device=dev, generator=g)
    uni = torch.rand(n, 7, device=dev, generator=g)
    R = turntable_rotations(np.arange(A) * (360. / A), 'mitsuba').to(dev)
    out = {}
    for H, W in ((256, 512), (1024, 2048)):
        light = EnvmapLight(lognormal(H, W, dev), 'mitsuba')
        batched = timed(lambda: light.sample_rotations(R, rough, nrm, view, uni), a.repeats)

        def calls():
            for _ in range(A):
                light.sample(rough, nrm, view, uni)
        single = timed(calls, a.repeats)
        # bytes the batched launch writes: wi, pdf_table, light [A,3,n,3] and own_pdf [A,3,n]
        batched['GBps_written'] = A * 3 * n * 4 * 10 / (batched['median'] * 1e-3) / 1e9
        out['%dx%d' % (H, W)] = {'batched': batched, 'calls': single}
        print('map %4dx%-4d %d points x %d rotations: one launch %8.3f ms (%6.1f GB/s written), %d unrotated calls %8.3f ms'
              % (H, W, n, A, batched['median'], batched['GBps_written'], A, single['median']), flush=True)
    return out


def strip(a, dev, mode):
    """config 5's frame, rows 400 - strip_rows/2 .. : 800 x strip_rows pixels x 256 rays, as render_frame chunks it"""
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.lighting import EnvmapLight, turntable_rotations
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
    rows, rays, A = a.strip_rows, w['num_rays'], a.angles
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
    model.set_envmap_light(light, mode)
    rot = turntable_rotations(np.arange(A) * (360. / A), 'mitsuba')
    kw = dict(num_rays=rays, memory_capacity_level=w['memory_capacity_level'])

    def turntable():
        R.render_turntable(model, inp, rows * W, rot, **kw)

    def standalone():
        with torch.no_grad():
            for _ in range(A):
                R.render_frame(model, inp, rows * W, **kw)
    # the two alternate, repeat by repeat, after one warm-up each: a drift of the machine lands on both
    ms = {'turntable': [], 'standalone': []}
    for rep in range(a.repeats + 1):
        for name, fn in (('turntable', turntable), ('standalone', standalone)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep > 0:
                ms[name].append(e0.elapsed_time(e1))
            print('  %s repeat %d: %.1f ms' % (name, rep, e0.elapsed_time(e1)), flush=True)
    res = {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'n': a.repeats} for k, v in ms.items()}
    # one more (untimed) pass of each, counting the rays of every tracer call after the primary one of a chunk
    rt = model.ray_tracer
    inner = rt.forward
    counts = []

    def forward(*args, **kwargs):
        d = kwargs['ray_directions']
        counts.append((d.shape[0] * d.shape[1], d.shape[1] > 1))
        return inner(*args, **kwargs)
    rt.forward = forward
    try:
        for name, fn in (('turntable', turntable), ('standalone', standalone)):
            del counts[:]
            fn()
            torch.cuda.synchronize()
            res[name]['primary_rays'] = sum(c for c, primary in counts if primary)
            res[name]['other_rays'] = sum(c for c, primary in counts if not primary)
            res[name]['tracer_calls'] = len(counts)
    finally:
        del rt.forward
    model.set_envmap_light(None)
    res['time_ratio'] = res['turntable']['median'] / res['standalone']['median']
    res['ray_ratio'] = res['turntable']['other_rays'] / max(res['standalone']['other_rays'], 1)
    print('strip %d x %d px x %d rays, map 256x512, indirect=%s, %d angles: turntable %9.1f ms, %d standalone frames %9.1f ms: '
          'time ratio %.3f; secondary (+ tertiary) rays %d against %d: ratio %.3f (26/72 = %.3f); tracer calls %d against %d'
          % (W, rows, rays, mode, A, res['turntable']['median'], A, res['standalone']['median'], res['time_ratio'],
             res['turntable']['other_rays'], res['standalone']['other_rays'], res['ray_ratio'], 26 / 72,
             res['turntable']['tracer_calls'], res['standalone']['tracer_calls']), flush=True)
    return res


def run_step(a):
    dev = torch.device('cuda')
    if a.step == 'sampler':
        return sampler(a, dev)
    return strip(a, dev, a.step[len('strip_'):])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--points', type=int, default=1 << 20)
    p.add_argument('--angles', type=int, default=24)
    p.add_argument('--strip_rows', type=int, default=4)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--steps', type=str, default=','.join(STEPS))
    p.add_argument('--step_timeout', type=int, default=540)
    p.add_argument('--json', type=str, default='')
    p.add_argument('--step', type=str, default='', help=argparse.SUPPRESS)          # the child's step
    a = p.parse_args(argv)
    if a.step:
        res = run_step(a)
        if a.json:
            with open(a.json, 'w') as f:
                json.dump(res, f, indent=1)
        return 0
    steps = [s for s in a.steps.split(',') if s]
    if any(s not in STEPS for s in steps):
        raise SystemExit('--steps takes %s' % ', '.join(STEPS))
    out = {}
    for s in steps:
        part = (a.json + '.' + s) if a.json else ''
        cmd = [sys.executable, os.path.abspath(__file__), '--step', s, '--points', str(a.points), '--angles', str(a.angles),
               '--strip_rows', str(a.strip_rows), '--repeats', str(a.repeats)] + (['--json', part] if part else [])
        try:
            rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
        except subprocess.TimeoutExpired:
            print('step %s ran out of its %d s: stopping' % (s, a.step_timeout), flush=True)
            return 124
        if rc != 0:
            print('step %s ended with status %d: stopping' % (s, rc), flush=True)
            return rc
        if part:
            with open(part) as f:
                out[s] = json.load(f)
            os.remove(part)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
