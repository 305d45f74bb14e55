#!/usr/bin/env python3
"""Mesh export timings on one GPU, on the 8 x 512 conf.conf SDF net fitted to the bowl scene ('bowl_trained'):

    python tools/mcubes_microbench.py [--resolutions 256 512 1024] [--repeats 5] [--json out.json]

  grid_ms      mesh.sdf_grid: the SDF at r^3 grid points through the tracer's split-precision evaluator
  mcubes_ms    mesh.marching_cubes on that volume: count, the one host read of the two counts, emit
  V, F         vertices and triangles
  mc_GBps      (volume read once + vertices and faces written) / mcubes_ms, and its share of the 8 TB/s HBM peak
  extract_s    mesh.extract_mesh end to end (grid, marching cubes, normals, materials), wall clock after a synchronise

HIP events around each repeat after one warm-up; the median of the repeats is reported with min and max (the grid at
1024^3 and extract_mesh are timed fewer times: --big_repeats).

    python tools/mcubes_microbench.py --sparse [--resolutions 256 512 1024 2048] [--brick 8] [--no_dense]

times extract_mesh(sparse=True) (DESIGN.md 6f "Sparse export") against extract_mesh() per resolution, interleaved, after one
warm-up of each: --repeats sparse runs, and as many dense ones (--big_repeats above 512^3; none where the dense path cannot
hold the grid, or with --no_dense).  Per path: grid_s and mcubes_s (extract_mesh's HIP events: for the sparse path
classification + evaluation + audit, and the brick kernels + sort), extract_s (wall clock after a synchronise) and the peak
of torch's allocator; for the sparse path the active and evaluated shares.  The SDF interval grid is built before the
timed runs (warm); build_s is ops.build_bound_grid alone, which a first export of a network pays once on top."""
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


def _export_runs(mesh, model, r, n, **kw):
    runs = []
    for _ in range(n):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        m = mesh.extract_mesh(model, resolution=r, **kw)
        torch.cuda.synchronize()
        runs.append(dict(extract_s=time.perf_counter() - t0, grid_s=m.meta['grid_s'], mcubes_s=m.meta['mcubes_s'],
                         peak_bytes=torch.cuda.max_memory_allocated(), V=m.verts.shape[0], F=m.faces.shape[0],
                         sparse=m.meta.get('sparse')))
        del m
        torch.cuda.empty_cache()
    return runs


def _summary(runs):
    out = {k: statistics.median(x[k] for x in runs) for k in ('extract_s', 'grid_s', 'mcubes_s')}
    out.update(n=len(runs), peak_bytes=max(x['peak_bytes'] for x in runs), V=runs[0]['V'], F=runs[0]['F'],
               extract_min=min(x['extract_s'] for x in runs), extract_max=max(x['extract_s'] for x in runs))
    return out


def _stage_peak(fn):
    """peak of torch's allocator over fn() above what was allocated before it"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def _grid_stage_peaks(mesh, ops, net, cells, bound, r, brick, dense):
    """peak memory of the grid stage alone (evaluation + marching cubes, no audit, no per-vertex passes), from the public
    pieces extract_mesh is made of - extract_mesh's own peak is set by the normals and materials of all V vertices at once"""
    pm = net.packed(f16x3=True)
    sp = 2.0 * bound / (r - 1)
    frame = ((r,) * 3, [-bound] * 3, [[sp, 0.0, 0.0], [0.0, sp, 0.0], [0.0, 0.0, sp]])

    def sparse_stage():
        active = ops.classify_bricks(cells, bound, frame, 0.0, brick)
        return ops.marching_cubes_sparse(lambda idx: ops.sdf_eval(pm, mesh.grid_points_at(idx, r, bound)), (r,) * 3, active,
                                         0.0, (-bound,) * 3, (sp,) * 3, brick)

    def dense_stage():
        return mesh.marching_cubes(mesh.sdf_grid(net, r, bound), 0.0, spacing=(sp,) * 3, origin=(-bound,) * 3)

    with torch.no_grad():
        return _stage_peak(sparse_stage), (_stage_peak(dense_stage) if dense else None)


def sparse_bench(opt, model, mesh):
    from nefii_amd import ops
    net, bound = model.implicit_network, model.object_bounding_sphere
    pm = net.packed(f16x3=True)
    tau = net.coarse_tau(bound)
    build = timed(lambda: ops.build_bound_grid(pm, bound, tau), opt.repeats)
    assert net.bound_grid(radius=bound) is not None
    print('interval grid G = %d: build %.2f ms (median of %d)' % (ops.BOUND_GRID_SIZE, build['median'], build['n']), flush=True)
    rows = []
    for r in opt.resolutions:
        fits = r ** 3 <= ops.MCUBES_MAX_POINTS and not opt.no_dense
        n_dense = (opt.repeats if r <= 512 else opt.big_repeats) if fits else 0
        _export_runs(mesh, model, r, 1, sparse=True, brick=opt.brick)
        if fits:
            _export_runs(mesh, model, r, 1)
        sparse, dense = [], []
        for i in range(opt.repeats):                     # interleaved
            sparse += _export_runs(mesh, model, r, 1, sparse=True, brick=opt.brick)
            if i < n_dense:
                dense += _export_runs(mesh, model, r, 1)
        meta = sparse[0]['sparse']
        assert meta['fallback'] is None and meta['audit_violations'] == 0, meta
        row = {'resolution': r, 'brick': opt.brick, 'sparse': _summary(sparse), 'dense': _summary(dense) if dense else None,
               'active_share': meta['active_bricks'] / meta['bricks'],
               'evaluated_share': meta['evaluated_points'] / meta['dense_points'], 'meta': meta,
               'build_ms': build['median']}
        row['sparse']['grid_stage_peak_bytes'], dense_peak = _grid_stage_peaks(
            mesh, ops, net, net.bound_grid(radius=bound), bound, r, opt.brick, bool(dense))
        if dense:
            row['dense']['grid_stage_peak_bytes'] = dense_peak
        if dense:
            assert (row['sparse']['V'], row['sparse']['F']) == (row['dense']['V'], row['dense']['F'])
            row['speedup'] = row['dense']['extract_s'] / row['sparse']['extract_s']
        rows.append(row)
        s, d = row['sparse'], row['dense']
        print('%5d^3  sparse: extract %.3f s (grid %.3f, mc %.3f; peak %.2f GB, grid stage %.2f GB)  active %.2f %%  evaluated %.2f %%  V %d F %d'
              % (r, s['extract_s'], s['grid_s'], s['mcubes_s'], s['peak_bytes'] / 1e9, s['grid_stage_peak_bytes'] / 1e9,
                 100 * row['active_share'],
                 100 * row['evaluated_share'], s['V'], s['F'])
              + ('  |  dense: extract %.3f s (grid %.3f, mc %.3f; peak %.2f GB, grid stage %.2f GB; n %d)  speed-up %.2f x'
                 % (d['extract_s'], d['grid_s'], d['mcubes_s'], d['peak_bytes'] / 1e9, d['grid_stage_peak_bytes'] / 1e9, d['n'],
                    row['speedup']) if d else ''),
              flush=True)
    return {'interval_grid': ops.BOUND_GRID_SIZE, 'build_ms': build, 'rows': rows}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--sparse', default=False, action='store_true', help='time extract_mesh(sparse=True) against extract_mesh()')
    p.add_argument('--brick', type=int, default=8)
    p.add_argument('--no_dense', default=False, action='store_true', help='--sparse: skip the dense runs')
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
    if opt.sparse:
        out = {'device': torch.cuda.get_device_name(0), 'net': 'conf.conf 8 x 512, bowl_trained', **sparse_bench(opt, model, mesh)}
        print(json.dumps(out))
        if opt.json:
            with open(opt.json, 'w') as fh:
                json.dump(out, fh, indent=1)
        return
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
