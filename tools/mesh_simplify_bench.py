#!/usr/bin/env python3
"""What simplifying the exported mesh costs on one GPU, and what it does to the surface.

    python tools/mesh_simplify_bench.py [--scene bowl_trained] [--resolution 512] [--simplify 2,4] [--repeats 5]
                                        [--json out.json]

For each cell size K of --simplify: mesh.extract_mesh(resolution, simplify=K) end to end once (marching-cubes time as meta
reports it, faces and vertices before and after, mean |network sdf| and mean distance to the analytic scene with and
without the projection), then mesh.simplify_mesh alone on the marching-cubes mesh: device events around its three stages
(clustering and the corner sort, the kernel with its 8-byte read-back, face bookkeeping), one warm-up call, the median of
--repeats calls with their min and max.  Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def spread(values):
    return {'median': statistics.median(values), 'min': min(values), 'max': max(values)}


def show(r):
    return '%8.3f ms [%.3f .. %.3f]' % (r['median'], r['min'], r['max'])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--scene', type=str, default='bowl_trained')
    p.add_argument('--resolution', type=int, default=512)
    p.add_argument('--simplify', type=str, default='2,4')
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--json', type=str, default='')
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        print('mesh_simplify_bench: no GPU - nothing here can be timed without one', file=sys.stderr)
        return 1
    import scenes
    from mesh_components_bench import load_model
    from nefii_amd import mesh
    dev = torch.device('cuda')
    model = load_model(a.scene, dev)
    net = model.implicit_network
    truth = scenes.SCENES[a.scene.split('_')[0]]

    def errors(m):
        with torch.no_grad():
            own = net.value_feature_gradient(m.verts)[0].abs().mean().item()
        return own, truth(m.verts.double().cpu()).abs().mean().item()

    plain = mesh.extract_mesh(model, resolution=a.resolution)
    res = {'device': torch.cuda.get_device_name(0), 'scene': a.scene, 'resolution': a.resolution,
           'verts': plain.verts.shape[0], 'faces': plain.faces.shape[0], 'mcubes_ms': plain.meta['mcubes_s'] * 1e3,
           'grid_ms': plain.meta['grid_s'] * 1e3, 'errors': errors(plain), 'simplify': []}
    print('%s at %d: %d vertices, %d faces; grid %.1f ms, marching cubes %.3f ms; mean |network sdf| %.3e, to the scene %.3e'
          % (a.scene, a.resolution, res['verts'], res['faces'], res['grid_ms'], res['mcubes_ms'], *res['errors']))
    bare = mesh.Mesh(plain.verts, plain.faces)
    for k in (float(x) for x in a.simplify.split(',') if x):
        raw = mesh.extract_mesh(model, resolution=a.resolution, simplify=k, project=False)
        proj = mesh.extract_mesh(model, resolution=a.resolution, simplify=k)
        cell = k * plain.meta['spacing']
        mesh.simplify_mesh(bare, cell)                                   # warm-up
        runs = [mesh.simplify_mesh(bare, cell).meta['simplify'] for _ in range(a.repeats)]
        row = {'k': k, 'cell': cell, 'clusters': runs[0]['clusters'], 'verts': runs[0]['verts'], 'faces': runs[0]['faces'],
               'cancelled_sets': runs[0]['cancelled_sets'], 'mcubes_ms_same_call': proj.meta['mcubes_s'] * 1e3,
               'errors_simplified': errors(raw), 'errors_projected': errors(proj)}
        for key in ('simplify_s', 'cluster_s', 'kernel_s', 'faces_s'):
            row[key.replace('_s', '_ms')] = spread([r[key] * 1e3 for r in runs])
        res['simplify'].append(row)
        print('simplify %g (cell %.5f): %d clusters -> %d vertices, %d faces (%.1f %% of the faces), %d sets cancelled; '
              'marching cubes of the same call %.3f ms' % (k, cell, row['clusters'], row['verts'], row['faces'],
                                                          100.0 * row['faces'] / res['faces'], row['cancelled_sets'],
                                                          row['mcubes_ms_same_call']))
        print('    simplify_mesh %s = clustering and sort %s + kernel %s + faces %s' % tuple(
            show(row[key]) for key in ('simplify_ms', 'cluster_ms', 'kernel_ms', 'faces_ms')))
        print('    mean |network sdf| %.3e -> projected %.3e; mean distance to the scene %.3e -> projected %.3e' % (
            row['errors_simplified'][0], row['errors_projected'][0], row['errors_simplified'][1], row['errors_projected'][1]))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
