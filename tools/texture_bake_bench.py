#!/usr/bin/env python3
"""What baking the materials of an exported mesh into textures costs on one GPU, and what the textures keep.

    python tools/texture_bake_bench.py [--scene bowl_trained] [--resolution 512] [--simplify 4] [--sizes 2048,4096]
                                       [--repeats 3] [--samples 20000] [--ao_rays 64] [--irradiance sky.exr [--irradiance_rays 64]]
                                       [--json out.json]

mesh.extract_mesh(resolution, keep='largest', simplify=K) once, then for each size of --sizes: texture.bake_textures with one
warm-up call and the median of --repeats calls with their min and max (bake_s and its split into the raster kernel and the
networks, by device events as meta reports them), the 8-bit encoding between two events, and texture.verify_textures: mean and
max error of texture lookups and of interpolated per-vertex attributes against the networks.  --ao_rays K adds one
texture.bake_occlusion of K rays per texel (6r; one call, no repeats: it is the long step): its time by device events, rays per
second and the mean occlusion over the covered texels.  --irradiance sky.exr adds one texture.bake_irradiance under that map (6u;
--irradiance_rays per texel, half of them drawn from the map): its time, the rays traced and skipped, the time per traced ray
and the covered means.  Fails without a GPU."""
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
    return '%9.3f ms [%.3f .. %.3f]' % (r['median'], r['min'], r['max'])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--scene', type=str, default='bowl_trained')
    p.add_argument('--resolution', type=int, default=512)
    p.add_argument('--simplify', type=float, default=4.0)
    p.add_argument('--sizes', type=str, default='2048,4096')
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--samples', type=int, default=20000)
    p.add_argument('--ao_rays', type=int, default=0, help='also bake ambient occlusion with this many rays per texel (0: off)')
    p.add_argument('--irradiance', type=str, default='', help='also bake the diffuse lightmap under this lat-long HDR map (.exr)')
    p.add_argument('--irradiance_rays', type=int, default=64)
    p.add_argument('--json', type=str, default='')
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        print('texture_bake_bench: no GPU - nothing here can be timed without one', file=sys.stderr)
        return 1
    from mesh_components_bench import load_model
    from nefii_amd import mesh, texture
    dev = torch.device('cuda')
    model = load_model(a.scene, dev)
    m = mesh.extract_mesh(model, resolution=a.resolution, keep='largest', simplify=a.simplify)
    light = None
    if a.irradiance:
        from nefii_amd.lighting import EnvmapLight
        light = EnvmapLight.from_exr(a.irradiance, device=dev)
    res = {'device': torch.cuda.get_device_name(0), 'scene': a.scene, 'resolution': a.resolution, 'simplify': a.simplify,
           'verts': m.verts.shape[0], 'faces': m.faces.shape[0], 'sizes': []}
    print('%s at %d, simplify %g: %d vertices, %d faces' % (a.scene, a.resolution, a.simplify, res['verts'], res['faces']))
    for size in (int(x) for x in a.sizes.split(',') if x):
        if m.faces.shape[0] > texture.atlas_capacity(size):
            print('texture %d holds at most %d faces: skipped' % (size, texture.atlas_capacity(size)))
            continue
        texture.bake_textures(model, m, size)                                    # warm-up
        runs = [texture.bake_textures(model, m, size) for _ in range(a.repeats)]
        baked = runs[-1]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        texture.encode_textures(baked)
        ev[0].record()
        texture.encode_textures(baked)
        ev[1].record()
        torch.cuda.synchronize()
        row = {'size': size, 'cell': baked.meta['cell'], 'leg': baked.meta['leg'], 'owned_texels': baked.meta['owned_texels'],
               'covered_texels': baked.meta['covered_texels'], 'encode_ms': ev[0].elapsed_time(ev[1]),
               'verify': texture.verify_textures(model, m, baked, a.samples)}
        for key in ('bake_s', 'raster_s', 'network_s'):
            row[key.replace('_s', '_ms')] = spread([r.meta[key] * 1e3 for r in runs])
        res['sizes'].append(row)
        print('texture %d: cells of %d texels (leg %d), %d owned texels (%.1f %% of the image), %d covered' % (
            size, row['cell'], row['leg'], row['owned_texels'], 100.0 * row['owned_texels'] / size ** 2, row['covered_texels']))
        print('    bake %s = raster %s + networks %s; 8-bit encoding %.3f ms' % (
            show(row['bake_ms']), show(row['raster_ms']), show(row['network_ms']), row['encode_ms']))
        v = row['verify']
        print('    against the networks at %d surface points, mean (max) |difference|: albedo %.3e (%.3e) from the texture, %.3e '
              '(%.3e) from the vertices; roughness %.3e (%.3e), %.3e (%.3e)' % (
                  v['samples'], v['texture_albedo_mean'], v['texture_albedo_max'], v['vertex_albedo_mean'], v['vertex_albedo_max'],
                  v['texture_roughness_mean'], v['texture_roughness_max'], v['vertex_roughness_mean'], v['vertex_roughness_max']))
        if a.ao_rays:
            occ = texture.bake_occlusion(model, m, baked, rays=a.ao_rays)
            row['ao'] = dict(occ.meta, rays_per_s=occ.meta['traced_rays'] / occ.meta['ao_s'])
            print('    ambient occlusion, %d rays per texel: %d rays in %.3f s, %.3g rays/s (%.1f x the material bake); mean over '
                  'the covered texels %.4f, %d texels off the surface' % (
                      a.ao_rays, occ.meta['traced_rays'], occ.meta['ao_s'], row['ao']['rays_per_s'],
                      occ.meta['ao_s'] * 1e3 / row['bake_ms']['median'], occ.meta['mean_ao_covered'],
                      occ.meta['off_surface_texels']))
            del occ
        if light is not None:
            irr = texture.bake_irradiance(model, m, baked, light, rays=a.irradiance_rays)
            im = irr.meta
            row['irradiance'] = dict(im, map=list(light.shape), rays_per_s=im['traced_rays'] / im['irradiance_s'],
                                     ns_per_traced_ray=1e9 * im['irradiance_s'] / max(im['traced_rays'], 1))
            print('    irradiance under %s (%d x %d), %d + %d rays per texel: %d traced, %d skipped in %.3f s, %.3g rays/s = %.1f ns '
                  'per traced ray (%.1f x the material bake); covered means: irradiance %.6g, noise %.6g' % (
                      os.path.basename(a.irradiance), light.shape[0], light.shape[1], im['rays_cos'], im['rays_map'],
                      im['traced_rays'], im['skipped_rays'], im['irradiance_s'], row['irradiance']['rays_per_s'],
                      row['irradiance']['ns_per_traced_ray'], im['irradiance_s'] * 1e3 / row['bake_ms']['median'],
                      im['mean_irradiance_covered'], im['mean_noise_covered']))
            del irr
        del runs, baked
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
