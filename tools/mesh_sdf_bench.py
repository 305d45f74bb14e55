#!/usr/bin/env python3
"""What the mesh BVH buys Step 1 on one GPU: brute force against the tree on torus meshes of growing size.

    python tools/mesh_sdf_bench.py [--faces 2304,36864,262144,1048576] [--samples 16384] [--window 1.0] [--rounds 3]
                                   [--brute_cap 524288] [--skip_iteration] [--json out.json]

Per mesh (a closed torus of nu x nu/2 quads, R 0.6, r 0.25):
  build      mesh_bvh.build_bvh on the device, the one-off cost per mesh
  sample     one SDFSampler.sample() of --samples points under method 'brute', 'bvh' and 'bvh' with Morton-sorted queries
             (MeshSDF.sort_queries), all three drawing the same points
  query      the distance query alone (MeshSDF.__call__ on those points): what differs between the methods
  iteration  one Step-1 iteration as training/geometry_train.py runs it with run_s1.sh's shapes - a batch of 16 dataset items
             of 1024 samples each, then GeometryTrainRunner.train_iteration on them (conf.conf's SDF network) - under
             'brute' and 'bvh'
Timing: device events around synchronised work, every shape warmed first, each window repeats the call until --window
seconds have passed, the methods alternate over --rounds rounds in this one process; a figure is the median of the rounds'
per-call times with their min and max.  Above --brute_cap faces brute force is timed on 1/16 of the points (its cost is
points x faces, in chunks of MeshSDF.pair_budget pairs) and multiplied by 16: such figures carry "scaled": true.
The iteration is never scaled.  Results are compared while they are there: the largest |d_bvh - d_brute| of each mesh is
printed.  Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torus_mesh(nu, nv, R=0.6, r=0.25):
    """closed torus about the z axis: nu x nv quads, two triangles each -> (vertices [nu nv, 3], faces [2 nu nv, 3])"""
    u, v = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing='ij')
    verts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    i1, j1 = (i + 1) % nu, (j + 1) % nv
    v00, v10, v11, v01 = i * nv + j, i1 * nv + j, i1 * nv + j1, i * nv + j1
    faces = np.stack([np.stack([v00, v10, v11], -1), np.stack([v00, v11, v01], -1)], 2).reshape(-1, 3)
    return verts, faces.astype(np.int64)


def window(fn, seconds):
    """per-call milliseconds of fn over a window of at least `seconds` (after one warm-up call that also sizes the window)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    n = max(1, int(np.ceil(seconds * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n, n


def alternate(fns, seconds, rounds):
    """{name: fn} -> {name: {median, min, max, calls per window}} of per-call ms, the methods taking turns round by round"""
    ms = {k: [] for k in fns}
    calls = {}
    for _ in range(rounds):
        for k, fn in fns.items():
            t, calls[k] = window(fn, seconds)
            ms[k].append(t)
    return {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'calls_per_window': calls[k], 'rounds': rounds}
            for k, v in ms.items()}


def show(name, r):
    return '%s %9.3f ms [%.3f .. %.3f]%s' % (name, r['median'], r['min'], r['max'], ' (scaled x16)' if r.get('scaled') else '')


def scaled(r, factor):
    return dict({k: (v * factor if k in ('median', 'min', 'max') else v) for k, v in r.items()}, scaled=True)


def runner_conf():
    from nefii_amd import conf, synthetic as syn
    return conf.from_dict({
        'train': {'model_class': 'nefii_amd.model.implicit_differentiable_renderer.IDRNetwork',
                  'loss_class': 'nefii_amd.model.loss.IDRLoss', 'idr_learning_rate': 5e-4, 'idr_sched_milestones': [],
                  'idr_sched_factor': 0.5, 'ckpt_freq': 1 << 30},
        'loss': syn.loss_conf('conf'), 'model': syn.model_conf('conf')})


def bench_mesh(a, nu, dev, tmp):
    from nefii_amd.datasets.sdf_dataset import SDFSampler
    from nefii_amd.mesh_bvh import build_bvh
    from nefii_amd.training.geometry_train import GeometryTrainRunner
    verts, faces = torus_mesh(nu, nu // 2)
    F = len(faces)
    out = {'faces': F, 'samples': a.samples}
    cut = F > a.brute_cap
    n_brute = a.samples // 16 if cut else a.samples
    s = {'bvh': SDFSampler(None, a.samples, device=dev, mesh=(verts, faces), method='bvh'),
         'brute': SDFSampler(None, n_brute, device=dev, mesh=(verts, faces), method='brute')}
    s['bvh_sorted'] = SDFSampler(None, a.samples, device=dev, mesh=(verts, faces), method='bvh')
    s['bvh_sorted'].mesh_sdf.sort_queries = True
    s['bvh'].mesh_sdf.sort_queries = False
    m = s['bvh'].mesh_sdf
    out['build'] = alternate({'build': lambda: build_bvh(m.ra, m.rb, m.rc)}, min(a.window, 0.5), a.rounds)['build']
    out['levels'] = m.bvh.levels
    print('%8d faces, %d tree levels: %s' % (F, m.bvh.levels, show('build', out['build'])), flush=True)

    g = torch.Generator()
    pts = (s['bvh'].sample(g.manual_seed(0))[0] - torch.as_tensor(s['bvh'].center, device=dev)) / s['bvh'].scale
    d = {k: v.mesh_sdf(pts[:n_brute] if k == 'brute' else pts) for k, v in s.items()}
    out['max_abs_diff'] = (d['bvh'][:n_brute] - d['brute']).abs().max().item()
    out['sorted_bitwise_equal'] = bool(torch.equal(d['bvh'].view(torch.int64), d['bvh_sorted'].view(torch.int64)))
    print('          max |d_bvh - d_brute| = %.3g over %d points; sorted queries give the same bits: %s' % (
        out['max_abs_diff'], n_brute, out['sorted_bitwise_equal']), flush=True)

    for what, fns in (('sample', {k: (lambda v=v: v.sample(g)) for k, v in s.items()}),
                      ('query', {k: (lambda k=k, v=v: v.mesh_sdf(pts[:n_brute] if k == 'brute' else pts)) for k, v in s.items()})):
        r = alternate(fns, a.window, a.rounds)
        if cut:
            r['brute'] = scaled(r['brute'], 16)
        out[what] = r
        print('          %-9s %s | %s | %s | brute / bvh = %.1f, sorted / unsorted = %.2f' % (
            what, show('brute', r['brute']), show('bvh', r['bvh']), show('bvh sorted', r['bvh_sorted']),
            r['brute']['median'] / r['bvh']['median'], r['bvh_sorted']['median'] / r['bvh']['median']), flush=True)
    out['bvh_query_us_per_point'] = out['query']['bvh']['median'] * 1e3 / a.samples

    if not a.skip_iteration:
        cfg = runner_conf()
        fns = {}
        for k in ('brute', 'bvh'):
            torch.manual_seed(0)
            r = GeometryTrainRunner(conf=cfg, exps_folder_name=tmp, expname='bench', new_timestamp='%d_%s' % (F, k),
                                    mesh=(verts, faces), sample_num=1024, batch_size=16384, max_niters=1 << 30,
                                    sdf_method=k)

            def iteration(r=r):
                points, sdf = next(iter(r.train_dataloader))
                r.train_iteration(points, sdf)
            fns[k] = iteration
        r = alternate(fns, a.window, a.rounds)                  # never scaled: brute force runs its whole batch here
        out['iteration'] = r
        print('          iteration %s | %s | brute / bvh = %.1f' % (show('brute', r['brute']), show('bvh', r['bvh']),
                                                                  r['brute']['median'] / r['bvh']['median']), flush=True)
    return out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--faces', type=str, default='2304,36864,262144,1048576')
    p.add_argument('--samples', type=int, default=16384)
    p.add_argument('--window', type=float, default=1.0)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--brute_cap', type=int, default=524288)
    p.add_argument('--skip_iteration', default=False, action='store_true')
    p.add_argument('--json', type=str, default='')
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        print('mesh_sdf_bench: no GPU - nothing here can be timed without one', file=sys.stderr)
        return 1
    dev = torch.device('cuda')
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        for F in (int(x) for x in a.faces.split(',') if x):
            nu = int(round(F ** 0.5))
            if nu * (nu // 2) * 2 != F:
                print('mesh_sdf_bench: --faces takes squares of even numbers (nu x nu/2 quads), got %d' % F, file=sys.stderr)
                return 2
            res.append(bench_mesh(a, nu, dev, tmp))
    if len(res) > 1:
        lo, hi = res[0], res[-1]
        print('bvh query per point: %s us at %s faces: x %.2f for x %.0f faces' % (
            ', '.join('%.4f' % r['bvh_query_us_per_point'] for r in res), ', '.join(str(r['faces']) for r in res),
            hi['bvh_query_us_per_point'] / lo['bvh_query_us_per_point'], hi['faces'] / lo['faces']))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(0), 'meshes': res}, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
