"""Export the trained SDF (and the materials on it) as a PLY mesh: the reference's plots.get_surface_trace /
get_surface_high_res_mesh (utils/plots.py:127-241), on the GPU.

    python -m nefii_amd.scripts.extract_mesh --conf confs_sg/conf.conf --expname robot --exps_folder_name exps \\
        [--old_expdir ...] [--timestamp latest] [--checkpoint latest] --resolution 512 [--level 0] [--bound 1.0] \\
        [--no_materials] [--out surface.ply] [--compare_mesh input.obj [--compare_samples 20000] [--no_scale_to_unit]] \\
        [--keep all|largest|<fraction>] [--high_res [--low_resolution 100] [--grid_margin 0.2]] \\
        [--simplify 3 [--no_project]] [--sparse [--brick 8]] \\
        [--texture 2048 [--texture_pad 2] [--no_texture_project] [--texture_exr] [--verify_texture 20000] \\
            [--texture_ao 64 [--ao_distance D] [--ao_bias B] [--ao_seed S] [--texture_bent_normal] [--texture_orm] \\
             [--verify_ao 2000]] \\
            [--texture_irradiance sky.exr [--irradiance_rays 64] [--irradiance_map_share 0.5] [--irradiance_height H \\
             --irradiance_width W] [--irradiance_scale 1] [--irradiance_rotate Y,X,Z] [--coordinate_type mitsuba|blender] \\
             [--irradiance_bias B] [--irradiance_seed S] [--irradiance_exposure 1] [--verify_irradiance 2000]]]
    python -m nefii_amd.scripts.extract_mesh --conf confs_sg/sdf.conf --geometry <Step-1 ModelParameters/N.pth> --out s.ply
    python -m nefii_amd.scripts.extract_mesh --conf confs_sg/conf_neus.conf --geometry_neus <ckpt.pth> --out s.ply

A Step-2 checkpoint (<exps>/<expname>/<timestamp>/checkpoints/ModelParameters/<checkpoint>.pth, loaded as
scripts/render.py loads it) gives normals and per-vertex materials, written by default to
<exps>/<expname>/<timestamp>/plots/surface_<epoch>.ply.  --geometry / --geometry_neus load only the SDF network (as
idr_train.py does) and write normals only.

--keep largest drops every connected component but the one of the largest area (the floaters an SDF network leaves away
from the object); --keep 0.1 keeps the components of at least a tenth of that area.  --high_res meshes the uniform grid at
--low_resolution first, fits a PCA-aligned box with --grid_margin around the largest component and re-meshes there:
--resolution then counts the points along the box's SHORTEST axis, the other two axes get the same spacing.

--simplify K merges the vertices of every cube of K grid spacings (K > 1) into one, placed by the quadric error of the faces
around them, and snaps the result back onto the SDF's level set (--no_project leaves it where the quadrics put it); normals
and materials are evaluated at the new vertices.  K = 3 leaves roughly a tenth of the faces.  The result is not guaranteed
to be manifold.  --keep applies before it, --compare_mesh measures the simplified mesh.

--sparse evaluates and meshes only the bricks (--brick cells per edge) of the grid that the network's SDF interval grid
cannot rule out: the same mesh for less work, and --resolution may then exceed the dense path's 1290, up to 4096.  The
intervals are audited during the export; a violation is reported and the export repeated without them.

--texture T bakes the materials into T x T maps over an atlas that gives every face its own chart and writes,
next to the PLY (which stays as it is), <stem>.obj with texture coordinates, <stem>.mtl and <stem>_albedo.png (tone-mapped
as the PLY's vertex colours), <stem>_roughness.png, <stem>_normal.png (object space).  Every texel is evaluated by the networks
at its own surface point, so the maps keep the materials' resolution when --simplify thins the mesh.  The face count must fit:
T holds 2 (T // (3 pad + 1))^2 faces.  --verify_texture N prints, as one JSON line, the mean and max error of texture lookups
and of interpolated per-vertex attributes against the networks at N random surface points.

--texture_ao K also bakes ambient occlusion: every texel sends K cosine-weighted rays (1 .. 1024) from its
surface point against the SDF itself, and <stem>_ao.png holds the share that escapes (linear, 1 = open); the MTL names it as
map_Ka.  --ao_distance D counts only hits within D, --ao_bias B starts the rays B above the surface, --ao_seed S picks another
rotation of the ray sequence.  --texture_bent_normal writes <stem>_bent_normal.png (the mean unoccluded direction, object space,
0.5 n + 0.5), --texture_orm writes <stem>_orm.png in the glTF packing (R occlusion, G roughness, B 0), --texture_exr also
<stem>_ao.exr.  --verify_ao N prints, as one JSON line, the map's error against a direct estimate at N random surface points and
the noise floor of K rays.

--texture_irradiance sky.exr also bakes a diffuse lightmap under that lat-long HDR map: the direct irradiance of
every texel, its visibility traced against the SDF itself, no interreflection.  Every texel sends --irradiance_rays rays (1 ..
1024), the share --irradiance_map_share of them drawn from the map's own distribution and the rest cosine-weighted, combined by
the balance heuristic.  The map is loaded as scripts/render.py --light_envmap loads it (--irradiance_height / _width resample it,
--irradiance_scale is its exposure, --coordinate_type its up axis: mitsuba y, blender z); --irradiance_rotate Y,X,Z turns it by
Euler angles in degrees as fit_envmap --rotate does.  <stem>_irradiance.exr holds the linear irradiance, <stem>_lit.png the
diffuse radiance --irradiance_exposure x albedo x E / pi, tone-mapped as the albedo map.  --verify_irradiance N prints, as one
JSON line, the map's error against a direct estimate at N random surface points beside the bake's own noise estimate.
"""
import argparse
import json
import os
import sys
import time

import torch

from .. import conf as hocon
from ..utils import general as utils

DEFAULT_MODEL = 'nefii_amd.model.implicit_differentiable_renderer.IDRNetwork'


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0], formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--conf', type=str, required=True)
    p.add_argument('--expname', type=str, default='')
    p.add_argument('--exps_folder_name', '--exps_folder', dest='exps_folder', type=str, default='exps')
    p.add_argument('--old_expdir', type=str, default='')
    p.add_argument('--timestamp', default='latest', type=str)
    p.add_argument('--checkpoint', default='latest', type=str)
    p.add_argument('--geometry', type=str, default='', help='a Step-1 checkpoint (ModelParameters/N.pth): SDF only')
    p.add_argument('--geometry_neus', type=str, default='', help='a NeuS checkpoint (sdf_network_fine): SDF only')
    p.add_argument('--model_class', type=str, default='')
    p.add_argument('--resolution', type=int, default=512, help='grid points per axis (plots.get_grid_uniform)')
    p.add_argument('--level', type=float, default=0.0)
    p.add_argument('--bound', type=float, default=None, help='grid half-width (default: the object bounding sphere)')
    p.add_argument('--no_materials', default=False, action='store_true')
    p.add_argument('--keep', type=str, default='all',
                   help="connected components to keep: all, largest (by area), or a fraction x in (0, 1]: those of at least "
                        'x times the largest area')
    p.add_argument('--high_res', default=False, action='store_true',
                   help="re-mesh on a grid aligned with the largest component of a low-resolution mesh "
                        '(plots.get_surface_high_res_mesh); --resolution counts the points along its shortest axis')
    p.add_argument('--low_resolution', type=int, default=100, help='--high_res: points per axis of the first, uniform grid')
    p.add_argument('--grid_margin', type=float, default=0.2, help="--high_res: margin around the component's box")
    p.add_argument('--simplify', type=float, default=0.0,
                   help='simplify by vertex clustering with quadric error metrics: the cell size in grid spacings (> 1); '
                        '0: off')
    p.add_argument('--no_project', default=False, action='store_true',
                   help='--simplify: do not move the simplified vertices back onto the level set of the SDF')
    p.add_argument('--sparse', default=False, action='store_true',
                   help='evaluate only the bricks the SDF interval grid cannot rule out; lifts the limit on --resolution to 4096')
    p.add_argument('--brick', type=int, default=8, help='--sparse: cells per brick edge, 2 .. 8')
    p.add_argument('--out', type=str, default='', help='output PLY (needed with --geometry / --geometry_neus)')
    p.add_argument('--compare_mesh', type=str, default='',
                   help='an .obj to measure the extracted surface against, normalised as Step 1 normalises it; prints '
                        'one JSON line of accuracy, completeness, Chamfer and Hausdorff distances.  Exact point-to-mesh '
                        'distances on the GPU (datasets/sdf_dataset.MeshSDF) through a bounding-volume hierarchy over '
                        "each mesh's faces: one tree build per mesh, then a tree walk per sample - no longer samples x "
                        "faces (that path, in chunks of MeshSDF.pair_budget point-face pairs, remains as method='brute')")
    p.add_argument('--compare_samples', type=int, default=20000, help='points sampled on each mesh for --compare_mesh')
    p.add_argument('--no_scale_to_unit', default=False, action='store_true',
                   help='--compare_mesh: take the .obj as it is (Step 1 with --not_scale_to_unit)')
    p.add_argument('--texture', type=int, default=None,
                   help='bake albedo, roughness and object-space normal maps of this many texels per side (7 .. 8192) over a '
                        'per-face-chart atlas and write <stem>.obj, <stem>.mtl and three PNGs next to the PLY')
    p.add_argument('--texture_pad', type=int, default=None, help='--texture: texels between the charts (>= 2; default 2)')
    p.add_argument('--no_texture_project', default=False, action='store_true',
                   help="--texture: evaluate the texels on the mesh's faces, not on the level set of the SDF")
    p.add_argument('--texture_exr', default=False, action='store_true',
                   help='--texture: also write the linear float maps <stem>_albedo.exr and <stem>_roughness.exr')
    p.add_argument('--verify_texture', type=int, default=None,
                   help='--texture: compare the textures, and the per-vertex attributes, with the networks at this many '
                        'random surface points; prints one JSON line')
    p.add_argument('--texture_ao', type=int, default=None,
                   help='--texture: also bake ambient occlusion with this many rays per texel (1 .. 1024), traced against the '
                        'SDF; writes <stem>_ao.png and names it in the MTL (map_Ka)')
    p.add_argument('--ao_distance', type=float, default=None,
                   help='--texture_ao: only hits within this distance occlude (default: unbounded)')
    p.add_argument('--ao_bias', type=float, default=None,
                   help='--texture_ao: start the rays this far above the surface along the normal (default 0)')
    p.add_argument('--ao_seed', type=int, default=None, help='--texture_ao: the seed of the ray sequence (default 0)')
    p.add_argument('--texture_bent_normal', default=False, action='store_true',
                   help='--texture_ao: also write <stem>_bent_normal.png, the mean unoccluded direction in object space')
    p.add_argument('--texture_orm', default=False, action='store_true',
                   help='--texture_ao: also write <stem>_orm.png, the glTF packing R = occlusion, G = roughness, B = 0')
    p.add_argument('--verify_ao', type=int, default=None,
                   help='--texture_ao: compare the occlusion map with a direct estimate at this many random surface points; '
                        'prints one JSON line')
    p.add_argument('--texture_irradiance', type=str, default='',
                   help='--texture: also bake the direct irradiance under this lat-long HDR map (.exr), MIS-sampled and traced '
                        'against the SDF; writes <stem>_irradiance.exr and <stem>_lit.png')
    p.add_argument('--irradiance_rays', type=int, default=None, help='--texture_irradiance: rays per texel, 1 .. 1024 (default 64)')
    p.add_argument('--irradiance_map_share', type=float, default=None,
                   help="--texture_irradiance: the share of the rays drawn from the map's distribution, in [0, 1] (default 0.5); "
                        'the rest are cosine-weighted')
    p.add_argument('--irradiance_height', type=int, default=None, help='--texture_irradiance: resample the map to this height')
    p.add_argument('--irradiance_width', type=int, default=None, help='--texture_irradiance: resample the map to this width')
    p.add_argument('--irradiance_scale', type=float, default=None, help='--texture_irradiance: exposure scale of the map (default 1)')
    p.add_argument('--irradiance_rotate', type=str, default=None,
                   help='--texture_irradiance: Y,X,Z Euler angles in degrees that turn the light, as fit_envmap --rotate')
    p.add_argument('--coordinate_type', type=str, default=None,
                   help="--texture_irradiance: the map's up axis, mitsuba (y, the default) or blender (z)")
    p.add_argument('--irradiance_bias', type=float, default=None,
                   help='--texture_irradiance: start the rays this far above the surface along the normal (default 0)')
    p.add_argument('--irradiance_seed', type=int, default=None, help='--texture_irradiance: the seed of the ray sequences (default 0)')
    p.add_argument('--irradiance_exposure', type=float, default=None,
                   help='--texture_irradiance: the exposure of <stem>_lit.png (default 1)')
    p.add_argument('--verify_irradiance', type=int, default=None,
                   help='--texture_irradiance: compare the lightmap with a direct estimate at this many random surface points; '
                        'prints one JSON line')
    return p


IRRADIANCE_FLAGS = ('irradiance_rays', 'irradiance_map_share', 'irradiance_height', 'irradiance_width', 'irradiance_scale',
                    'irradiance_rotate', 'coordinate_type', 'irradiance_bias', 'irradiance_seed', 'irradiance_exposure',
                    'verify_irradiance')


def _irradiance_flags(opt):
    """the message of the first flag of the irradiance bake that cannot stand (None: all can), before the GPU is touched; parses
    --irradiance_rotate into opt.irradiance_rotation (three angles or None)"""
    opt.irradiance_rotation = None
    if not opt.texture_irradiance:
        given = ['--' + k for k in IRRADIANCE_FLAGS if getattr(opt, k) is not None]
        if given:
            return '%s need%s --texture_irradiance (and --texture)' % (', '.join(given), 's' if len(given) == 1 else '')
        return None
    if opt.texture is None:
        return '--texture_irradiance needs --texture'
    if opt.no_texture_project:
        return ('--texture_irradiance cannot be combined with --no_texture_project: texels left on the faces may lie inside the '
                'surface')
    if opt.irradiance_rays is not None and not 1 <= opt.irradiance_rays <= 1024:
        return '--irradiance_rays must lie in 1 .. 1024'
    if opt.irradiance_map_share is not None and not 0.0 <= opt.irradiance_map_share <= 1.0:
        return '--irradiance_map_share must lie in [0, 1]'
    for k in ('irradiance_height', 'irradiance_width', 'verify_irradiance'):
        if getattr(opt, k) is not None and getattr(opt, k) < 1:
            return '--%s must be positive' % k
    if opt.irradiance_scale is not None and not 0.0 < opt.irradiance_scale < float('inf'):
        return '--irradiance_scale must be positive'
    if opt.irradiance_exposure is not None and not 0.0 <= opt.irradiance_exposure < float('inf'):
        return '--irradiance_exposure must not be negative'
    if opt.irradiance_bias is not None and not opt.irradiance_bias >= 0.0:
        return '--irradiance_bias must not be negative'
    if opt.irradiance_seed is not None and not 0 <= opt.irradiance_seed < 1 << 32:
        return '--irradiance_seed must lie in 0 .. 2^32 - 1'
    if opt.coordinate_type is not None and opt.coordinate_type not in ('mitsuba', 'blender'):
        return '--coordinate_type is mitsuba or blender, not %r' % opt.coordinate_type
    if opt.irradiance_rotate is not None:
        try:
            angles = [float(v) for v in opt.irradiance_rotate.split(',')]
        except ValueError:
            angles = []
        if len(angles) != 3 or not all(abs(a) < float('inf') for a in angles):
            return '--irradiance_rotate takes three comma-separated angles, Y,X,Z'
        opt.irradiance_rotation = angles
    if not os.path.exists(opt.texture_irradiance):
        return '--texture_irradiance: no map at ' + opt.texture_irradiance
    return None


def _resolve_checkpoint(opt):
    """(checkpoint path, expdir, timestamp) as scripts/render.py finds them"""
    expdir = os.path.join(opt.exps_folder, opt.expname)
    old = opt.old_expdir or expdir
    timestamp = opt.timestamp
    if timestamp == 'latest':                                                   # render.py:75-90
        stamps = sorted(s for s in os.listdir(old) if '.' not in s) if os.path.exists(old) else []
        if not stamps:
            raise FileNotFoundError('no experiment under ' + old)
        timestamp = stamps[-1]
    ckpt = os.path.join(old, timestamp, 'checkpoints', 'ModelParameters', str(opt.checkpoint) + '.pth')
    return ckpt, expdir, timestamp


def load_model(opt, c, device):
    """-> (model, path of the checkpoint read, epoch or None, whether the materials were trained)"""
    model_cls = opt.model_class or c.get_string('train.model_class', default=DEFAULT_MODEL)
    model = utils.get_class(model_cls)(conf=c.get_config('model')).to(device)
    if opt.geometry or opt.geometry_neus:
        path = opt.geometry or opt.geometry_neus
        if not os.path.exists(path):
            raise FileNotFoundError('no checkpoint at ' + path)
        saved = torch.load(path, map_location=device)
        if opt.geometry:                                                        # idr_train.py:294-301
            full = model.state_dict()
            full.update({k: v for k, v in saved['model_state_dict'].items() if 'implicit_network' in k})
            model.load_state_dict(full)
        else:                                                                   # idr_train.py:303-306
            model.implicit_network.load_state_dict(saved['sdf_network_fine'])
        epoch = saved.get('epoch')
        trained_materials = False
    else:
        path, _, _ = _resolve_checkpoint(opt)
        if not os.path.exists(path):
            raise FileNotFoundError('no checkpoint at ' + path)
        saved = torch.load(path, map_location=device)
        model.load_state_dict(saved['model_state_dict'])
        epoch = saved.get('epoch')
        trained_materials = True
    model.freeze_geometry()
    model.eval()
    return model, path, epoch, trained_materials


def compare(mesh, obj_path, samples, scale_to_unit, device, seed=0, method='auto'):
    """accuracy (extracted -> input), completeness (input -> extracted), Chamfer (their mean), Hausdorff (their max);
    method: how MeshSDF answers the distance queries ('auto': the BVH kernel on a GPU)"""
    from ..datasets.sdf_dataset import MeshSDF, SDFSampler, load_obj, resolve_method
    ref = SDFSampler(obj_path, number_of_points=1, scale_to_unit=scale_to_unit, device=device, mesh=load_obj(obj_path),
                     method=method)
    ours = MeshSDF(mesh.verts.double(), mesh.faces, device=device, method=resolve_method(method, device))
    g = torch.Generator().manual_seed(seed)
    acc = ref.mesh_sdf(ours.sample_surface(samples, g), signed=False)          # only |d| is wanted: no parity pass
    comp = ours(ref.mesh_sdf.sample_surface(samples, g), signed=False)
    r = {'accuracy_mean': acc.mean().item(), 'accuracy_max': acc.max().item(),
         'completeness_mean': comp.mean().item(), 'completeness_max': comp.max().item()}
    r['chamfer'] = 0.5 * (r['accuracy_mean'] + r['completeness_mean'])
    r['hausdorff'] = max(r['accuracy_max'], r['completeness_max'])
    r['samples'] = samples
    return r


def vertex_props(mesh):
    if mesh.diffuse_albedo is None:
        return None
    a = mesh.diffuse_albedo.clamp_min(0.).pow(1. / 2.2).clamp(0., 1.)                 # the render panel's tone map
    rgb = (a * 255. + 0.5).floor().clamp(0, 255).to(torch.uint8).cpu().numpy()
    alb = mesh.diffuse_albedo.cpu().numpy()
    spec = mesh.specular_reflection.cpu().numpy()
    return {'red': rgb[:, 0], 'green': rgb[:, 1], 'blue': rgb[:, 2],
            'albedo_r': alb[:, 0], 'albedo_g': alb[:, 1], 'albedo_b': alb[:, 2],
            'roughness': mesh.roughness.cpu().numpy()[:, 0],
            'specular_r': spec[:, 0], 'specular_g': spec[:, 1], 'specular_b': spec[:, 2]}


def write_textures(model, mesh, stem, size, pad, project, exr, ao_name=None):
    """bake the materials over the mesh's faces and write <stem>.obj, <stem>.mtl, <stem>_albedo.png, <stem>_roughness.png,
    <stem>_normal.png (and, with exr, the linear float maps <stem>_albedo.exr, <stem>_roughness.exr) -> BakedTextures.
    ao_name: the occlusion map write_occlusion will write, for the MTL to name"""
    from PIL import Image
    from ..texture import bake_textures, corner_uv, encode_textures
    from ..utils.obj import write_mtl, write_obj
    t0 = time.perf_counter()
    baked = bake_textures(model, mesh, size, pad=pad, project=project)
    images = {k: v.cpu().numpy() for k, v in encode_textures(baked).items()}
    base = os.path.basename(stem)
    names = {k: '%s_%s.png' % (base, k) for k in ('albedo', 'roughness', 'normal')}
    for k, name in names.items():
        Image.fromarray(images[k]).save(os.path.join(os.path.dirname(stem), name))
    write_obj(stem + '.obj', mesh.verts, mesh.faces, mesh.normals, corner_uv(baked.atlas), base + '.mtl')
    write_mtl(stem + '.mtl', baked.specular_reflection, names['albedo'], names['roughness'], names['normal'],
              **({} if ao_name is None else {'ao': ao_name}))
    if exr:
        from ..utils import exr as exr_io
        exr_io.imwrite(stem + '_albedo.exr', baked.diffuse_albedo.cpu().numpy())
        exr_io.imwrite(stem + '_roughness.exr', baked.roughness.cpu().numpy())
    m = baked.meta
    print('extract_mesh: texture %d: cells of %d texels (leg %d, pad %d), %d owned texels, %d covered; bake %.3f s (raster '
          '%.4f s, networks %.3f s), %.3f s with the files -> %s.obj' % (
              m['size'], m['cell'], m['leg'], m['pad'], m['owned_texels'], m['covered_texels'], m['bake_s'], m['raster_s'],
              m['network_s'], time.perf_counter() - t0, stem))
    return baked


def write_occlusion(model, mesh, baked, stem, rays, distance, bias, seed, bent_normal, orm, exr):
    """bake ambient occlusion over the texels of `baked` and write <stem>_ao.png (and, as asked, <stem>_bent_normal.png,
    <stem>_orm.png, <stem>_ao.exr) -> BakedOcclusion"""
    from PIL import Image
    from ..texture import bake_occlusion, encode_occlusion
    t0 = time.perf_counter()
    occ = bake_occlusion(model, mesh, baked, rays=rays, distance=distance, bias=bias, seed=seed)
    images = encode_occlusion(baked, occ)
    wanted = ['ao'] + (['bent_normal'] if bent_normal else []) + (['orm'] if orm else [])
    for k in wanted:
        Image.fromarray(images[k].cpu().numpy()).save('%s_%s.png' % (stem, k))
    if exr:
        from ..utils import exr as exr_io
        exr_io.imwrite(stem + '_ao.exr', occ.ao.cpu().numpy())
    m = occ.meta
    print('extract_mesh: ambient occlusion: %d rays per texel, %d traced in %.3f s (%.3g rays/s), distance %s, bias %g, seed %d; '
          'mean over the covered texels %.4f, %d texels off the surface; %.3f s with the files -> %s_ao.png' % (
              m['rays'], m['traced_rays'], m['ao_s'], m['traced_rays'] / max(m['ao_s'], 1e-9),
              'unbounded' if m['distance'] is None else '%g' % m['distance'], m['bias'], m['seed'], m['mean_ao_covered'],
              m['off_surface_texels'], time.perf_counter() - t0, stem))
    return occ


def write_irradiance(model, mesh, baked, stem, opt):
    """bake the diffuse lightmap under the map of --texture_irradiance over the texels of `baked` and write
    <stem>_irradiance.exr and <stem>_lit.png -> (BakedIrradiance, the light, the rotation or None)"""
    from PIL import Image
    from ..lighting import EnvmapLight
    from ..texture import bake_irradiance, encode_irradiance
    from ..utils import exr as exr_io
    t0 = time.perf_counter()
    light = EnvmapLight.from_exr(opt.texture_irradiance, opt.coordinate_type or 'mitsuba', height=opt.irradiance_height,
                                 width=opt.irradiance_width, scale=1.0 if opt.irradiance_scale is None else opt.irradiance_scale,
                                 device=baked.owner.device)
    rotation = None
    if opt.irradiance_rotation is not None:
        from scipy.spatial.transform import Rotation
        rotation = torch.from_numpy(Rotation.from_euler('yxz', opt.irradiance_rotation, degrees=True).as_matrix()).float()
    irr = bake_irradiance(model, mesh, baked, light, rays=64 if opt.irradiance_rays is None else opt.irradiance_rays,
                          map_share=0.5 if opt.irradiance_map_share is None else opt.irradiance_map_share,
                          bias=opt.irradiance_bias or 0.0, seed=opt.irradiance_seed or 0, rotation=rotation)
    images = encode_irradiance(baked, irr, 1.0 if opt.irradiance_exposure is None else opt.irradiance_exposure)
    exr_io.imwrite(stem + '_irradiance.exr', images['irradiance'].cpu().numpy())
    Image.fromarray(images['lit'].cpu().numpy()).save(stem + '_lit.png')
    m = irr.meta
    print('extract_mesh: irradiance under %s (%d x %d): %d + %d rays per texel (cosine + map), %d traced and %d skipped in %.3f s '
          '(%.3g rays/s), bias %g, seed %d; mean irradiance over the covered texels %.6g, mean noise %.6g, %d texels off the '
          'surface; %.3f s with the files -> %s_irradiance.exr' % (
              os.path.basename(opt.texture_irradiance), light.shape[0], light.shape[1], m['rays_cos'], m['rays_map'],
              m['traced_rays'], m['skipped_rays'], m['irradiance_s'], m['traced_rays'] / max(m['irradiance_s'], 1e-9), m['bias'],
              m['seed'], m['mean_irradiance_covered'], m['mean_noise_covered'], m['off_surface_texels'],
              time.perf_counter() - t0, stem))
    return irr, light, rotation


def print_components(title, table, meta):
    """the component table select_components leaves in Mesh.meta, largest area first"""
    if not table:
        return
    print('extract_mesh: %s: %d component%s (labelled in %d rounds, %.4f s in all)%s' % (
        title, table['count'], '' if table['count'] == 1 else 's', meta['cc_rounds'], meta['cc_s'],
        '' if table['count'] <= len(table['ids']) else ', the %d largest:' % len(table['ids'])))
    print('    %10s %10s %10s %14s' % ('id', 'vertices', 'faces', 'area'))
    for row in zip(table['ids'], table['n_verts'], table['n_faces'], table['area']):
        print('    %10d %10d %10d %14.6g' % row)


def main(argv=None):
    opt = build_parser().parse_args(argv)
    if (opt.geometry or opt.geometry_neus) and not opt.out:
        print('extract_mesh: --geometry / --geometry_neus need --out', file=sys.stderr)
        return 2
    if not (opt.geometry or opt.geometry_neus) and not opt.expname and not opt.old_expdir:
        print('extract_mesh: give --expname (or --old_expdir), or --geometry / --geometry_neus', file=sys.stderr)
        return 2
    if opt.resolution < 2:
        print('extract_mesh: --resolution must be >= 2', file=sys.stderr)
        return 2
    from ..mesh import _parse_keep, _parse_simplify
    try:
        keep = _parse_keep(opt.keep)
        simplify = _parse_simplify(opt.simplify)
    except ValueError as e:
        print('extract_mesh: --%s' % e, file=sys.stderr)
        return 2
    if opt.high_res and (opt.low_resolution < 2 or not opt.grid_margin >= 0.0):
        print('extract_mesh: --low_resolution must be >= 2 and --grid_margin must not be negative', file=sys.stderr)
        return 2
    if opt.sparse and not 2 <= opt.brick <= 8:
        print('extract_mesh: --brick must lie in 2 .. 8', file=sys.stderr)
        return 2
    bad = _irradiance_flags(opt)
    if bad:
        print('extract_mesh: %s' % bad, file=sys.stderr)
        return 2
    if opt.texture_ao is None:
        given = [name for name, on in (('--ao_distance', opt.ao_distance is not None), ('--ao_bias', opt.ao_bias is not None),
                                       ('--ao_seed', opt.ao_seed is not None), ('--texture_bent_normal', opt.texture_bent_normal),
                                       ('--texture_orm', opt.texture_orm), ('--verify_ao', opt.verify_ao is not None)) if on]
        if given:
            print('extract_mesh: %s need%s --texture_ao (and --texture)' % (', '.join(given), 's' if len(given) == 1 else ''),
                  file=sys.stderr)
            return 2
    if opt.texture is None:
        given = [name for name, on in (('--texture_pad', opt.texture_pad is not None), ('--no_texture_project',
                                       opt.no_texture_project), ('--texture_exr', opt.texture_exr),
                                       ('--verify_texture', opt.verify_texture is not None),
                                       ('--texture_ao', opt.texture_ao is not None)) if on]
        if given:
            print('extract_mesh: %s need%s --texture' % (', '.join(given), 's' if len(given) == 1 else ''), file=sys.stderr)
            return 2
    else:
        if not 7 <= opt.texture <= 8192:
            print('extract_mesh: --texture must lie in 7 .. 8192', file=sys.stderr)
            return 2
        if opt.texture_pad is not None and opt.texture_pad < 2:
            print('extract_mesh: --texture_pad must be >= 2', file=sys.stderr)
            return 2
        if opt.verify_texture is not None and opt.verify_texture < 1:
            print('extract_mesh: --verify_texture must be positive', file=sys.stderr)
            return 2
        if opt.texture_ao is not None:
            bad = None
            if not 1 <= opt.texture_ao <= 1024:
                bad = '--texture_ao must lie in 1 .. 1024 rays'
            elif opt.no_texture_project:
                bad = ('--texture_ao cannot be combined with --no_texture_project: texels left on the faces may lie inside the '
                       'surface')
            elif opt.ao_distance is not None and not opt.ao_distance > 0.0:
                bad = '--ao_distance must be positive'
            elif opt.ao_bias is not None and not opt.ao_bias >= 0.0:
                bad = '--ao_bias must not be negative'
            elif opt.ao_seed is not None and not 0 <= opt.ao_seed < 1 << 32:
                bad = '--ao_seed must lie in 0 .. 2^32 - 1'
            elif opt.verify_ao is not None and opt.verify_ao < 1:
                bad = '--verify_ao must be positive'
            if bad:
                print('extract_mesh: %s (--texture %d)' % (bad, opt.texture), file=sys.stderr)
                return 2
        if opt.no_materials or opt.geometry or opt.geometry_neus:
            print('extract_mesh: --texture bakes materials: it cannot be combined with --no_materials, --geometry or '
                  '--geometry_neus', file=sys.stderr)
            return 2
    if opt.compare_mesh and not os.path.exists(opt.compare_mesh):
        print('extract_mesh: no mesh at ' + opt.compare_mesh, file=sys.stderr)
        return 2
    if not os.path.exists(opt.conf):
        print('extract_mesh: no conf at ' + opt.conf, file=sys.stderr)
        return 2
    try:
        if not (opt.geometry or opt.geometry_neus):
            ckpt, expdir, timestamp = _resolve_checkpoint(opt)
            if not os.path.exists(ckpt):
                raise FileNotFoundError('no checkpoint at ' + ckpt)
        elif not os.path.exists(opt.geometry or opt.geometry_neus):
            raise FileNotFoundError('no checkpoint at ' + (opt.geometry or opt.geometry_neus))
    except FileNotFoundError as e:
        print('extract_mesh: %s' % e, file=sys.stderr)
        return 2

    from ..mesh import extract_mesh
    from ..utils.ply import write_ply
    torch.set_default_dtype(torch.float32)
    device = torch.device('cuda')
    c = hocon.parse_file(opt.conf)
    t0 = time.perf_counter()
    model, path, epoch, trained_materials = load_model(opt, c, device)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    try:
        mesh = extract_mesh(model, resolution=opt.resolution, level=opt.level, bound=opt.bound,
                            materials=trained_materials and not opt.no_materials, keep=keep, high_res=opt.high_res,
                            low_resolution=opt.low_resolution, margin=opt.grid_margin, simplify=simplify,
                            project=not opt.no_project, **(dict(sparse=True, brick=opt.brick) if opt.sparse else {}))
    except ValueError as e:
        if 'no surface' not in str(e):
            raise
        print('extract_mesh: %s' % e, file=sys.stderr)
        return 1
    t2 = time.perf_counter()
    sm = mesh.meta.get('simplify')
    if mesh.verts.shape[0] == 0 and sm and sm['faces_in'] > 0:
        print('extract_mesh: --simplify %g left no face of %d: its cells of %.6g hold the surface in %d cluster%s; use a '
              'smaller --simplify or a higher --resolution' % (simplify, sm['faces_in'], sm['cell'], sm['clusters'],
                                                               '' if sm['clusters'] == 1 else 's'), file=sys.stderr)
        return 1
    if mesh.verts.shape[0] == 0:
        print('extract_mesh: no surface at level %g inside [-%g, %g]^3 at resolution %d' % (
            opt.level, mesh.meta['bound'], mesh.meta['bound'], opt.resolution), file=sys.stderr)
        return 1
    if opt.texture is not None:
        from ..texture import atlas_capacity
        pad = 2 if opt.texture_pad is None else opt.texture_pad
        if mesh.faces.shape[0] > atlas_capacity(opt.texture, pad):
            print('extract_mesh: --texture %d with --texture_pad %d holds at most %d faces, the mesh has %d; use --simplify or a '
                  'larger --texture' % (opt.texture, pad, atlas_capacity(opt.texture, pad), mesh.faces.shape[0]),
                  file=sys.stderr)
            return 1
    out = opt.out
    if not out:
        out = os.path.join(expdir, timestamp, 'plots', 'surface_%s.ply' % (epoch if epoch is not None else opt.checkpoint))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    comments = ['nefii_amd extract_mesh resolution %d level %r bound %r' % (opt.resolution, opt.level, mesh.meta['bound']),
                'checkpoint %s' % os.path.abspath(path)]
    if opt.high_res or keep != 'all':
        comments.append('grid %d x %d x %d spacing %r keep %s%s' % (mesh.meta['grid_shape'] + (
            mesh.meta['spacing'], opt.keep, ' high_res low_resolution %d margin %r' % (opt.low_resolution, opt.grid_margin)
            if opt.high_res else '')))
        print('extract_mesh: grid %d x %d x %d, spacing %.6g' % (mesh.meta['grid_shape'] + (mesh.meta['spacing'],)))
        for title, key in (('low-resolution mesh', 'low_res_components'), ('mesh', 'components')):
            print_components(title, mesh.meta.get(key), mesh.meta)
    sparse = mesh.meta.get('sparse')
    if sparse:
        comments.append('sparse brick %d active %d of %d evaluated %d of %d fallback %s' % (
            sparse['brick'], sparse['active_bricks'], sparse['bricks'], sparse['evaluated_points'], sparse['dense_points'],
            sparse['fallback']))
        print('extract_mesh: sparse: %d of %d bricks of %d^3 active, %d of %d points evaluated (%.2f %%), %d probes, '
              '%d audit violations, fallback %s' % (sparse['active_bricks'], sparse['bricks'], sparse['brick'],
                                                    sparse['evaluated_points'], sparse['dense_points'],
                                                    100.0 * sparse['evaluated_points'] / sparse['dense_points'],
                                                    sparse['probes'], sparse['audit_violations'], sparse['fallback']))
    if sm:
        comments.append('simplify %r cell %r project %s' % (simplify, sm['cell'], 'no' if opt.no_project else 'yes'))
        print('extract_mesh: simplified %d vertices, %d faces -> %d, %d (cell %.6g, %.4f s)' % (
            sm['verts_in'], sm['faces_in'], sm['verts'], sm['faces'], sm['cell'], sm['simplify_s']))
    write_ply(out, mesh.verts, mesh.faces, normals=mesh.normals, vertex_props=vertex_props(mesh), comments=comments)
    t3 = time.perf_counter()
    print('extract_mesh: %d vertices, %d faces -> %s (grid %.3f s, marching cubes %.3f s, extract %.3f s, load %.3f s, '
          'write %.3f s)' % (mesh.verts.shape[0], mesh.faces.shape[0], out, mesh.meta['grid_s'], mesh.meta['mcubes_s'],
                             t2 - t1, t1 - t0, t3 - t2))
    if opt.texture is not None:
        stem = os.path.splitext(out)[0]
        baked = write_textures(model, mesh, stem, opt.texture, pad, not opt.no_texture_project, opt.texture_exr,
                               None if opt.texture_ao is None else os.path.basename(stem) + '_ao.png')
        if opt.verify_texture is not None:
            from ..texture import verify_textures
            print(json.dumps(verify_textures(model, mesh, baked, opt.verify_texture)))
        if opt.texture_ao is not None:
            occ = write_occlusion(model, mesh, baked, stem, opt.texture_ao, opt.ao_distance, opt.ao_bias or 0.0, opt.ao_seed or 0,
                                  opt.texture_bent_normal, opt.texture_orm, opt.texture_exr)
            if opt.verify_ao is not None:
                from ..texture import verify_occlusion
                print(json.dumps(verify_occlusion(model, mesh, baked, occ, opt.verify_ao)))
        if opt.texture_irradiance:
            irr, light, rotation = write_irradiance(model, mesh, baked, stem, opt)
            if opt.verify_irradiance is not None:
                from ..texture import verify_irradiance
                print(json.dumps(verify_irradiance(model, mesh, baked, irr, light, opt.verify_irradiance, rotation=rotation)))
    if opt.compare_mesh:
        r = compare(mesh, opt.compare_mesh, opt.compare_samples, not opt.no_scale_to_unit, device)
        print(json.dumps(r))
    return 0


if __name__ == '__main__':
    sys.exit(main())
