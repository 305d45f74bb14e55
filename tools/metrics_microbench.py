#!/usr/bin/env python3
"""The image-metric kernels' timings on one GPU against the host path:

    python tools/metrics_microbench.py [--size 800] [--repeats 5] [--split_views 4] [--json out.json]

  device      ops.image_metrics on --size x --size x 3 pairs, levels 1 and 5, B = 1 and 4: HIP events around each repeat
              after one warm-up, the median of the repeats with min and max, set against the model: the fp32 inputs read
              once (2 x 4 B per pixel and channel), and 2 passes x 11 taps x 5 moments multiply-adds per position and level
  host        scripts/evaluate.py's calculate_ssim + calculate_ms_ssim on the same arrays, by a host clock, torch limited to
              --threads threads: the median of the repeats
  split       `evaluate.main` without and with --gpu on a synthetic split of --split_views views of --size x --size, once
              each, by a host clock (file reading, tonemapping, alignment and masks are the host's in both; 0 skips this)"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_VECTOR_PEAK = 78.6e12          # MI355X, vector fp64 FLOP/s
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


def host_timed(fn, repeats):
    fn()
    s = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        s.append((time.perf_counter() - t0) * 1e3)
    return {'median': statistics.median(s), 'min': min(s), 'max': max(s), 'n': repeats}


def pair(size, seed):
    g = np.random.Generator(np.random.Philox(seed))
    yy, xx = np.mgrid[0:size, 0:size]
    a = (0.5 + 0.4 * np.sin(xx / 9.0 + np.arange(3)[:, None, None]) * np.cos(yy / 5.0)).transpose(1, 2, 0)
    a = np.ascontiguousarray(a, np.float32)
    return a, np.clip(a + g.normal(0, 0.05, a.shape), 0, 1).astype(np.float32)


def model(size, levels, B):
    flops, byts, s = 0, 2 * 4 * size * size * 3 * B, size
    for _ in range(levels):
        flops += 2 * 2 * 11 * 5 * (s - 10) * (s - 10) * 3 * B
        s = (s + 1) // 2
    return flops, byts


def device(a, dev):
    from nefii_amd import ops
    out = {}
    x, y = pair(a.size, 0)
    for B in (1, 4):
        xs = torch.from_numpy(np.stack([x] * B)).to(dev)
        ys = torch.from_numpy(np.stack([y] * B)).to(dev)
        for levels in (1, 5):
            t = timed(lambda: ops.image_metrics(xs, ys, levels), a.repeats)
            flops, byts = model(a.size, levels, B)
            t['GFLOPs'] = flops / (t['median'] * 1e-3) / 1e9
            t['input_GBps'] = byts / (t['median'] * 1e-3) / 1e9
            out['B%d_levels%d' % (B, levels)] = t
            print('device B = %d, levels = %d: %7.3f ms [%.3f .. %.3f]  %.1f MFLOP of filtering -> %7.1f GFLOP/s (%.2f %% of the '
                  'fp64 vector peak), %.2f MB of input -> %6.1f GB/s (%.2f %% of the HBM peak)'
                  % (B, levels, t['median'], t['min'], t['max'], flops / 1e6, t['GFLOPs'], 100. * t['GFLOPs'] * 1e9 / FP64_VECTOR_PEAK,
                     byts / 1e6, t['input_GBps'], 100. * t['input_GBps'] * 1e9 / HBM_PEAK), flush=True)
    return out


def host(a):
    from nefii_amd.scripts import evaluate as ev
    torch.set_num_threads(a.threads)
    x, y = pair(a.size, 0)
    out = {'threads': a.threads,
           'ssim': host_timed(lambda: ev.calculate_ssim(x, y), a.repeats),
           'ms_ssim': host_timed(lambda: ev.calculate_ms_ssim(x, y), a.repeats)}
    print('host, %d threads: calculate_ssim %.1f ms, calculate_ms_ssim %.1f ms (medians of %d)'
          % (a.threads, out['ssim']['median'], out['ms_ssim']['median'], a.repeats), flush=True)
    return out


def split(a):
    from PIL import Image
    from nefii_amd.scripts import evaluate as ev
    from nefii_amd.utils import exr
    if a.split_views <= 0:
        return {}
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        gt, plots = os.path.join(tmp, 'scene', 'test'), os.path.join(tmp, 'exp', 'plots')
        for d in ('image', 'diffuse', 'roughness', 'sp_rgb', 'mask'):
            os.makedirs(os.path.join(gt, d))
        os.makedirs(plots)
        yy, xx = np.mgrid[0:a.size, 0:a.size]
        mask = (((yy - a.size / 2) ** 2 + (xx - a.size / 2) ** 2) < (0.4 * a.size) ** 2).astype(np.uint8) * 255
        for i in range(a.split_views):
            Image.fromarray(mask).save(os.path.join(gt, 'mask', '%06d.png' % i))
            for k, (gt_name, pre_name) in enumerate((('image/%06d.exr', 'rerender_rgb-%03d.exr'),
                                                     ('diffuse/%06d_diffuse.00.exr', 'diffuse_albedo-%03d.exr'),
                                                     ('roughness/%06d.exr', 'roughness-%03d.exr'),
                                                     ('sp_rgb/%06d_sprgb.00.exr', 'specular_rgb-%03d.exr'))):
                x, y = pair(a.size, 10 * i + k)
                exr.imwrite(os.path.join(gt, gt_name % i), x)
                exr.imwrite(os.path.join(plots, pre_name % i), y)
        for name, gpu in (('host', False), ('gpu', True), ('gpu_again', True)):
            t0 = time.perf_counter()
            ev.main(plots, gt, gpu=gpu)
            out[name + '_s'] = time.perf_counter() - t0
    print('evaluate.main on %d views of %d x %d: host %.2f s, --gpu %.2f s (first call), --gpu %.2f s (second call)'
          % (a.split_views, a.size, a.size, out['host_s'], out['gpu_s'], out['gpu_again_s']), flush=True)
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--size', type=int, default=800)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--threads', type=int, default=16)
    p.add_argument('--split_views', type=int, default=4)
    p.add_argument('--json', type=str, default='')
    a = p.parse_args(argv)
    dev = torch.device('cuda')
    out = {'size': a.size, 'device': device(a, dev), 'host': host(a), 'split': split(a)}
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
