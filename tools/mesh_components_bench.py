#!/usr/bin/env python3
"""What component labelling costs and what the aligned grid buys the mesh export on one GPU.

    python tools/mesh_components_bench.py [--scene bowl_trained] [--label_resolutions 256,512] [--resolution 192]
                                          [--low_resolution 100] [--margin 0.2] [--repeats 5] [--json out.json]

  labelling  ops.mesh_components on the marching-cubes mesh of the fitted scene at each of --label_resolutions: vertices,
             faces, components, rounds, time (the whole call: init, the rounds, the 8-byte read-back after each)
  export     mesh.extract_mesh end to end (grid evaluation, marching cubes, labelling, normals and materials):
               uniform        the uniform grid at --resolution - the path of the commit before this one, unchanged
               high_res       --high_res at the same --resolution (points along the component's shortest axis), keep='largest'
               uniform_equal  the uniform grid at the resolution whose spacing is high_res's: what the same surface detail
                              costs without the aligned grid
Timing: device events around each call, one warm-up call per shape, the median of --repeats calls with their min and max.
Fails without a GPU."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats):
    """(last result, {median, min, max} in ms) of fn over `repeats` calls after one warm-up call"""
    fn()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return out, {'median': statistics.median(ms), 'min': min(ms), 'max': max(ms), 'repeats': repeats}


def show(r):
    return '%9.3f ms [%.3f .. %.3f]' % (r['median'], r['min'], r['max'])


def load_model(scene, dev):
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    mc = syn.model_conf('conf')
    model = IDRNetwork(conf.from_dict(mc))
    model.load_state_dict(syn.make_state_dict(mc, seed=0, scene=scene), strict=True)
    model = model.to(dev)
    model.freeze_geometry()
    model.eval()
    return model


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--scene', type=str, default='bowl_trained')
    p.add_argument('--label_resolutions', type=str, default='256,512')
    p.add_argument('--resolution', type=int, default=192)
    p.add_argument('--low_resolution', type=int, default=100)
    p.add_argument('--margin', type=float, default=0.2)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--json', type=str, default='')
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        print('mesh_components_bench: no GPU - nothing here can be timed without one', file=sys.stderr)
        return 1
    from nefii_amd import mesh, ops
    dev = torch.device('cuda')
    model = load_model(a.scene, dev)
    bound = float(model.object_bounding_sphere)
    res = {'device': torch.cuda.get_device_name(0), 'scene': a.scene, 'labelling': [], 'export': {}}

    for r in (int(x) for x in a.label_resolutions.split(',') if x):
        vol = mesh.sdf_grid(model.implicit_network, r, bound, precision=mesh._tracer_precision(model))
        sp = 2.0 * bound / (r - 1)
        verts, faces = mesh.marching_cubes(vol, 0.0, spacing=(sp, sp, sp), origin=(-bound,) * 3)
        del vol
        f32 = faces.int().contiguous()
        (label, rounds), t = timed(lambda: ops.mesh_components(f32, verts.shape[0]), a.repeats)
        row = {'resolution': r, 'vertices': verts.shape[0], 'faces': faces.shape[0], 'rounds': rounds,
               'components': int(torch.unique(label).numel()), 'ms': t}
        _, row['table_ms'] = timed(lambda: mesh.component_table(verts, faces, label), a.repeats)
        res['labelling'].append(row)
        print('labelling r = %4d: %8d vertices %8d faces %4d components %2d rounds %s; component_table %s' % (
            r, row['vertices'], row['faces'], row['components'], rounds, show(t), show(row['table_ms'])), flush=True)

    def export(name, **kw):
        m, t = timed(lambda: mesh.extract_mesh(model, **kw), a.repeats)
        row = {'ms': t, 'vertices': m.verts.shape[0], 'faces': m.faces.shape[0], 'grid_shape': list(m.meta['grid_shape']),
               'grid_points': int(math.prod(m.meta['grid_shape'])), 'spacing': m.meta['spacing'],
               'grid_s': m.meta['grid_s'], 'mcubes_s': m.meta['mcubes_s'], 'cc_rounds': m.meta['cc_rounds'],
               'cc_s': m.meta['cc_s']}
        res['export'][name] = row
        print('export %-13s %s: grid %s = %.2f M points, spacing %.5f, %d vertices %d faces (grid %.3f s, marching cubes '
              '%.3f s, labelling %.4f s in %d rounds)' % (name, show(t), 'x'.join(str(v) for v in row['grid_shape']),
                                                          row['grid_points'] / 1e6, row['spacing'], row['vertices'],
                                                          row['faces'], row['grid_s'], row['mcubes_s'], row['cc_s'],
                                                          row['cc_rounds']), flush=True)
        return row

    export('uniform', resolution=a.resolution)
    hi = export('high_res', resolution=a.resolution, high_res=True, low_resolution=a.low_resolution, margin=a.margin,
                keep='largest')
    equal = int(math.ceil(2.0 * bound / hi['spacing'])) + 1
    if equal ** 3 > ops.MCUBES_MAX_POINTS:
        print('export uniform_equal: a uniform grid of that spacing needs %d^3 points - more than marching_cubes takes' % equal)
    else:
        eq = export('uniform_equal', resolution=equal)
        print('equal spacing: uniform %d^3 takes %.2f x the time and %.2f x the grid points of high_res' % (
            equal, eq['ms']['median'] / hi['ms']['median'], eq['grid_points'] / hi['grid_points']))
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
