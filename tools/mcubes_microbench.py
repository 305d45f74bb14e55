#!/usr/bin/env python3
"""Mesh export timings on one GPU, on the 8 x 512 conf.conf SDF net fitted to the bowl scene ('bowl_trained'):

    python tools/mcubes_microbench.py [--resolutions 256 512 1024] [--repeats 5] [--json out.json]

  grid_ms      mesh.sdf_grid: the SDF at r^3 grid points through the tracer's split-precision evaluator
  mcubes_ms    mesh.marching_cubes on that volume: count, the one host read of the two counts, emit
  V, F         vertices and triangles
  mc_GBps      (volume read once + vertices and faces written) / mcubes_ms, and its share of the 8 TB/s HBM peak
  extract_s    mesh.extract_mesh end to end (grid, marching cubes, normals, materials), wall clock after a synchronise

HIP events around each repeat after one warm-up; the median of the repeats is reported with min and max (the grid at
1024^3 and extract_mesh are timed fewer times: --big_repeats)."""
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


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--resolutions', type=int, nargs='+', default=[256, 512, 1024])
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--big_repeats', type=int, default=2)
    p.add_argument('--json', type=str, default='')
    opt = p.parse_args(argv)
    from nefii_amd import conf, mesh, synthetic as syn
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    dev = torch.device('cuda:0')
    mc = syn.model_conf('conf')
    model = IDRNetwork(conf.from_dict(mc))
    model.load_state_dict(syn.make_state_dict(mc, seed=0, scene='bowl_trained'), strict=True)
    model = model.to(dev)
    model.freeze_geometry()
    model.eval()
    net, bound = model.implicit_network, model.object_bounding_sphere
    rows = []
    for r in opt.resolutions:
        reps = opt.repeats if r <= 512 else opt.big_repeats
        box = {}

        def grid():
            box['vol'] = mesh.sdf_grid(net, r, bound)
        tg = timed(grid, reps)
        vol = box.pop('vol')
        sp = 2.0 * bound / (r - 1)

        def mcubes():
            box['out'] = mesh.marching_cubes(vol, 0.0, spacing=(sp, sp, sp), origin=(-bound,) * 3)
        tm = timed(mcubes, opt.repeats)
        v, f = box.pop('out')
        V, F = v.shape[0], f.shape[0]
        del v, f, vol
        torch.cuda.empty_cache()
        nbytes = r ** 3 * 4 + V * 12 + F * 12
        gbps = nbytes / (tm['median'] * 1e-3) / 1e9
        walls = []
        for _ in range(max(1, opt.big_repeats) + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = mesh.extract_mesh(model, resolution=r)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
            del m
        row = {'resolution': r, 'grid_ms': tg, 'mcubes_ms': tm, 'V': V, 'F': F, 'mc_min_bytes': nbytes,
               'mc_GBps': gbps, 'mc_hbm_share': gbps * 1e9 / HBM_PEAK,
               'grid_pflops': r ** 3 * 3.67e6 / (tg['median'] * 1e-3) / 1e15,
               'extract_s': {'median': statistics.median(walls[1:]), 'first': walls[0], 'n': len(walls) - 1}}
        rows.append(row)
        print('%5d^3  grid %9.2f ms (%.2f PFLOP/s est.)  mc %7.3f ms  V %9d  F %9d  mc %6.0f GB/s (%.1f%% of HBM peak)  '
              'extract_mesh %.3f s' % (r, tg['median'], row['grid_pflops'], tm['median'], V, F, gbps,
                                      100 * row['mc_hbm_share'], row['extract_s']['median']), flush=True)
        torch.cuda.empty_cache()
    out = {'device': torch.cuda.get_device_name(0), 'net': 'conf.conf 8 x 512, bowl_trained', 'rows': rows}
    print(json.dumps(out))
    if opt.json:
        with open(opt.json, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
