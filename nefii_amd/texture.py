"""Baking the materials of an exported mesh into textures: albedo, roughness and object-space normal maps over a per-face-chart
atlas, evaluated by the networks at every texel's own surface point.

    atlas = triangle_atlas(F, 2048)                               # every face its own chart, two faces to a square cell
    uv = corner_uv(atlas)                                         # [F, 3, 2] float64, OBJ convention
    baked = bake_textures(model, mesh, 2048)                      # BakedTextures: float maps on the GPU
    images = encode_textures(baked)                               # 8-bit RGBA / grey levels, as the PNGs hold them
    got = sample_textures(baked, face, bary)                      # bilinear lookups at (face, barycentrics)
    report = verify_textures(model, mesh, baked, 20000)           # texture and per-vertex interpolation against the networks
    occ = bake_occlusion(model, mesh, baked, rays=64)             # BakedOcclusion: ambient occlusion and bent normals (6r)
    images = encode_occlusion(baked, occ)                         # 8-bit ao, bent_normal and the glTF ORM packing
    report = verify_occlusion(model, mesh, baked, occ, 2000)      # the map against a direct estimate and its noise floor
    irr = bake_irradiance(model, mesh, baked, light, rays=64)     # BakedIrradiance: the diffuse lightmap under a map light (6u)
    images = encode_irradiance(baked, irr)                        # the linear map and the lit 8-bit preview
    report = verify_irradiance(model, mesh, baked, irr, light, 2000)

The atlas - stated once in include/nefii_amd.h, mirrored here and in tests/texbake_ref.py: a T x T image of n x n square
cells of c = T // n texels, n = ceil(sqrt(ceil(F / 2))); face f lives in cell q = f // 2 at column q % n, row q // n, origin
(x0, y0) = (c (q % n), c (q // n)); texel (i, j) has its centre at (i + 1/2, j + 1/2), j counts rows from the top.  With p the
pad and s = c - 3 p the leg, an even face has its corners 0, 1, 2 at (x0 + p, y0 + p), (x0 + p + s, y0 + p), (x0 + p, y0 + p +
s), an odd one at (x0 + c - p, y0 + c - p), (x0 + c - p - s, y0 + c - p), (x0 + c - p, y0 + c - p - s).  A texel of the cell
with (i - x0) + (j - y0) + 1 < c belongs to the even face, every other one to the odd face; to nobody (-1) when that face is
>= F or the texel lies in the margin i >= n c or j >= n c.  With p >= 2 every texel that a bilinear lookup at a point inside or
on a chart reads with non-zero weight belongs to the chart's face; with p = 1 it does not, so p < 2 is refused.

The atlas functions are torch code that runs on any device, with no loop over faces.  The raster, the 8-bit encoding and the
sampler are csrc/nefii_texbake.hip; the attributes come from the fused evaluators the per-vertex tail of extract_mesh uses.
"""
import math
from dataclasses import dataclass, field

import torch

from . import ops
from .mesh import project_to_level_set, _implicit

MIN_SIZE, MAX_SIZE, MIN_PAD = ops.BAKE_MIN_SIZE, ops.BAKE_MAX_SIZE, ops.BAKE_MIN_PAD
NETWORK_BATCH = 2 ** 20                          # texels per pass through the networks, whatever the chunk


@dataclass(frozen=True)
class TriangleAtlas:
    size: int                                    # T: texels per side
    cells_per_row: int                           # n
    cell: int                                    # c = T // n
    pad: int                                     # p
    leg: int                                     # s = c - 3 p: the texels along a chart's two short edges
    n_faces: int                                 # F


def atlas_capacity(size, pad=2):
    """the largest face count an atlas of `size` texels per side holds with `pad`: 2 (size // (3 pad + 1))^2"""
    return 2 * (int(size) // (3 * int(pad) + 1)) ** 2


def triangle_atlas(n_faces, size, pad=2):
    """The atlas of n_faces per-face charts in a size x size image.  ValueError for a size outside 7 .. 8192, pad < 2, no face,
    and a leg below one texel - the message names the face count this size holds."""
    F, T, p = int(n_faces), int(size), int(pad)
    if not MIN_SIZE <= T <= MAX_SIZE:
        raise ValueError('texture size must lie in %d .. %d, got %d' % (MIN_SIZE, MAX_SIZE, T))
    if p < MIN_PAD:
        raise ValueError('pad must be >= %d (with less a bilinear lookup inside a chart reads its neighbour), got %d'
                         % (MIN_PAD, p))
    if F < 1:
        raise ValueError('an atlas needs at least one face, got %d' % F)
    n = math.isqrt((F + 1) // 2 - 1) + 1         # ceil(sqrt(ceil(F / 2))), in integers
    c = T // n
    s = c - 3 * p
    if s < 1:
        raise ValueError('%d faces do not fit a texture of %d with pad %d: it holds at most %d faces; simplify the mesh '
                         '(--simplify) or use a larger texture (--texture)' % (F, T, p, atlas_capacity(T, p)))
    return TriangleAtlas(T, n, c, p, s, F)


def corner_xy(atlas, device=None):
    """[F, 3, 2] float64: the chart corners of every face in texel units (x to the right, y down)"""
    a = atlas
    f = torch.arange(a.n_faces, device=device, dtype=torch.int64)
    q = f // 2
    x0, y0 = (a.cell * (q % a.cells_per_row)).double(), (a.cell * (q // a.cells_per_row)).double()
    odd = (f % 2 == 1)
    ax = torch.where(odd, x0 + (a.cell - a.pad), x0 + a.pad)
    ay = torch.where(odd, y0 + (a.cell - a.pad), y0 + a.pad)
    d = torch.where(odd, -float(a.leg), float(a.leg)).double()
    x = torch.stack([ax, ax + d, ax], 1)
    y = torch.stack([ay, ay, ay + d], 1)
    return torch.stack([x, y], 2)


def corner_uv(atlas, device=None):
    """[F, 3, 2] float64: the texture coordinates of every face's corners in OBJ convention, u = x / T, v = 1 - y / T"""
    xy = corner_xy(atlas, device)
    return torch.stack([xy[..., 0] / atlas.size, 1.0 - xy[..., 1] / atlas.size], 2)


def texel_owner(atlas, device=None):
    """[T, T] int32 (row j, column i): the face that owns each texel, -1 for nobody - the rule the raster kernel applies"""
    a = atlas
    t = torch.arange(a.size, device=device, dtype=torch.int64)
    j, i = t[:, None], t[None, :]
    cx, cy = i // a.cell, j // a.cell
    q = cy * a.cells_per_row + cx
    even = (i - cx * a.cell) + (j - cy * a.cell) + 1 < a.cell
    f = 2 * q + (~even).long()
    f = torch.where((cx < a.cells_per_row) & (cy < a.cells_per_row) & (f < a.n_faces), f, torch.full_like(f, -1))
    return f.to(torch.int32)


@dataclass
class BakedTextures:
    atlas: TriangleAtlas
    owner: torch.Tensor                          # [T,T] int32: the face of each texel, -1 for nobody
    covered: torch.Tensor                        # [T,T] bool: the texel's centre lies inside its face's chart
    position: torch.Tensor                       # [T,T,3] float32: the surface point each owned texel was evaluated at
    diffuse_albedo: torch.Tensor                 # [T,T,3] float32, linear
    roughness: torch.Tensor                      # [T,T] float32
    normal: torch.Tensor                         # [T,T,3] float32, object space, unit length
    specular_reflection: torch.Tensor            # [3]: the global specular reflection, as the PLY's specular_* hold it
    meta: dict = field(default_factory=dict)


def _max_move(mesh):
    """the bound of the vertex projection of extract_mesh: half the simplify cell, else half the grid spacing"""
    sm = mesh.meta.get('simplify')
    if sm:
        return 0.5 * float(sm['cell'])
    if 'spacing' in mesh.meta:
        return 0.5 * float(mesh.meta['spacing'])
    return math.inf


def _check(model, mesh, what):
    mat_net = getattr(model, 'envmap_material_network', None)
    if mat_net is None:
        raise ValueError('%s needs a model with an envmap_material_network (materials to bake)' % what)
    if mesh.verts.shape[0] == 0 or mesh.faces.shape[0] == 0:
        raise ValueError('%s: the mesh is empty' % what)
    if not mesh.verts.is_cuda or not mesh.faces.is_cuda:
        raise ValueError('%s needs CUDA tensors (the hot path has no CPU fallback)' % what)
    return mat_net


def _attributes(net, mat_net, x, level, max_move, project):
    """(x on the level set, normals, albedo [N,3], roughness [N], specular [3]) at the points x [N,3], in passes of
    NETWORK_BATCH: the per-vertex tail of extract_mesh at points of its own"""
    pts, nrm, alb, rgh, spec3 = [], [], [], [], None
    for s in range(0, x.shape[0], NETWORK_BATCH):
        xs = x[s:s + NETWORK_BATCH].contiguous()
        if project:
            xs = project_to_level_set(lambda y: net.value_feature_gradient(y)[::2], xs, level, max_move=max_move)
        _, feat, g = net.value_feature_gradient(xs)
        out = mat_net(xs, feat)
        N = xs.shape[0]
        pts.append(xs)
        nrm.append(g / g.norm(dim=1, keepdim=True).clamp_min(1e-12))
        alb.append(out['sg_diffuse_albedo'].float().reshape(N, 3))
        rgh.append(out['sg_roughness'].float().expand(N, 1).reshape(N))
        if spec3 is None:
            spec = mat_net.specular_inv_remap(out['sg_specular_reflectance']).float()
            spec3 = spec.reshape(-1, spec.shape[-1])[0].expand(3).contiguous()
    return torch.cat(pts), torch.cat(nrm), torch.cat(alb), torch.cat(rgh), spec3


def bake_textures(model, mesh, size, pad=2, project=True, chunk=2 ** 24):
    """The materials of `model` baked over the faces of `mesh` (a mesh.Mesh on the GPU, as extract_mesh returns it) into
    size x size float maps over triangle_atlas(F, size, pad).  Per chunk of `chunk` texels: ops.bake_raster gives every
    texel's face and the point of that face under the texel's centre (gutter texels extrapolate); the owned texels are
    compacted; with project their points are moved onto the level set mesh.meta['level'] of the model's SDF
    (project_to_level_set, at most half the simplify cell - half the grid spacing for a mesh that was not simplified - per
    component: the rule of the vertex projection); normals are the normalised SDF gradient there and the materials
    envmap_material_network(x, feature) - evaluated at the texel's own point, never interpolated from the vertices.  Texels
    nobody owns hold zeros.  meta: size, cell, leg, pad, owned_texels, covered_texels, project, bake_s = raster_s + network_s
    (HIP events).  Two bakes give the same bits.  ValueError for a model without materials, an empty mesh, CPU tensors, and a
    face count the size does not hold (triangle_atlas)."""
    mat_net = _check(model, mesh, 'bake_textures')
    net = _implicit(model)
    atlas = triangle_atlas(mesh.faces.shape[0], size, pad)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError('chunk must be positive, got %d' % chunk)
    dev = mesh.verts.device
    T = atlas.size
    level, max_move = float(mesh.meta.get('level', 0.0)), _max_move(mesh)
    with torch.no_grad():
        verts = mesh.verts.detach().float().contiguous()
        V = verts.shape[0]
        faces = mesh.faces if mesh.faces.dtype == torch.int32 else mesh.faces.clamp(-1, V).to(torch.int32)
        faces = faces.contiguous()
        owner = torch.empty(T * T, device=dev, dtype=torch.int32)
        covered = torch.empty(T * T, device=dev, dtype=torch.bool)
        position = torch.zeros(T * T, 3, device=dev, dtype=torch.float32)
        albedo = torch.zeros(T * T, 3, device=dev, dtype=torch.float32)
        roughness = torch.zeros(T * T, device=dev, dtype=torch.float32)
        normal = torch.zeros(T * T, 3, device=dev, dtype=torch.float32)
        spec3 = None
        events = []
        for first in range(0, T * T, chunk):
            count = min(chunk, T * T - first)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            o, cov, _, pos = ops.bake_raster(verts, faces, T, atlas.cells_per_row, atlas.cell, atlas.pad, first, count)
            ev[1].record()
            owner[first:first + count] = o
            covered[first:first + count] = cov != 0
            idx = (o >= 0).nonzero()[:, 0]
            if idx.shape[0]:
                x, nrm, alb, rgh, spec = _attributes(net, mat_net, pos[idx], level, max_move, project)
                spec3 = spec if spec3 is None else spec3
                at = idx + first
                position[at], normal[at], albedo[at], roughness[at] = x, nrm, alb, rgh
            ev[2].record()
            events.append(ev)
        n_owned, n_covered = int((owner >= 0).sum()), int(covered.sum())
        torch.cuda.synchronize(dev)
    raster_s = sum(ev[0].elapsed_time(ev[1]) for ev in events) / 1e3
    network_s = sum(ev[1].elapsed_time(ev[2]) for ev in events) / 1e3
    meta = dict(size=T, cell=atlas.cell, leg=atlas.leg, pad=atlas.pad, owned_texels=n_owned, covered_texels=n_covered,
                project=bool(project), bake_s=raster_s + network_s, raster_s=raster_s, network_s=network_s)
    return BakedTextures(atlas, owner.view(T, T), covered.view(T, T), position.view(T, T, 3), albedo.view(T, T, 3),
                         roughness.view(T, T), normal.view(T, T, 3), spec3, meta)


def encode_textures(baked):
    """dict(albedo [T,T,4], normal [T,T,4], roughness [T,T]) uint8 on the GPU, as the PNGs hold them (ops.bake_encode): the
    albedo tone-mapped as the PLY's vertex colours, the normal as 0.5 n + 0.5 in object space, alpha 255 on owned texels"""
    T = baked.atlas.size
    a, n, r = ops.bake_encode(baked.diffuse_albedo.reshape(-1, 3), baked.roughness.reshape(-1), baked.normal.reshape(-1, 3),
                              baked.owner.reshape(-1))
    return {'albedo': a.view(T, T, 4), 'normal': n.view(T, T, 4), 'roughness': r.view(T, T)}


def sample_textures(baked, face, bary):
    """dict(diffuse_albedo [N,3], roughness [N,1], normal [N,3]) float32: bilinear lookups of the baked maps at the points
    with barycentrics bary [N,3] of the faces face [N] (ops.texture_sample)"""
    a = baked.atlas
    face = face.to(torch.int32).contiguous()
    bary = bary.double().contiguous()
    look = lambda tex: ops.texture_sample(tex.contiguous(), face, bary, a.cells_per_row, a.cell, a.pad)    # noqa: E731
    return {'diffuse_albedo': look(baked.diffuse_albedo), 'roughness': look(baked.roughness.unsqueeze(2)),
            'normal': look(baked.normal)}


def sample_faces(verts, faces, count, generator=None):
    """(face [count] int64, bary [count,3] float64): area-weighted random points of a mesh, drawn as
    datasets.sdf_dataset.MeshSDF.sample_surface draws them (one torch.rand(count, 3) of fp64 on the host)"""
    v = verts.double()
    a, b, c = (v[faces.long()[:, k]] for k in range(3))
    area = 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1)
    cdf = torch.cumsum(area, 0) / area.sum()
    u = torch.rand(count, 3, dtype=torch.float64, generator=generator).to(verts.device)
    tri = torch.searchsorted(cdf, u[:, 0].contiguous()).clamp_(max=cdf.shape[0] - 1)
    r1 = u[:, 1].sqrt()
    return tri, torch.stack([1 - r1, r1 * (1 - u[:, 2]), r1 * u[:, 2]], 1)


def verify_textures(model, mesh, baked, samples, seed=0):
    """What the textures lose, and what per-vertex attributes lose, measured against the networks: `samples` area-weighted
    random points of the mesh (sample_faces) are moved onto the level set as bake_textures moves its texels, the networks
    evaluated there, and compared with the bilinear texture lookup at the same (face, barycentrics) and with the barycentric
    interpolation of the mesh's per-vertex attributes.  -> dict: samples, size, and texture_albedo_mean / _max,
    texture_roughness_mean / _max, vertex_albedo_mean / _max, vertex_roughness_mean / _max (mean and max |difference|)."""
    mat_net = _check(model, mesh, 'verify_textures')
    if mesh.diffuse_albedo is None or mesh.roughness is None:
        raise ValueError('verify_textures needs the per-vertex materials of the mesh to compare with')
    samples = int(samples)
    if samples < 1:
        raise ValueError('samples must be positive, got %d' % samples)
    net = _implicit(model)
    with torch.no_grad():
        faces = mesh.faces.long()
        face, bary = sample_faces(mesh.verts, faces, samples, torch.Generator().manual_seed(int(seed)))
        corners = faces[face]                                                   # [N,3]
        x = (bary[:, :, None] * mesh.verts.double()[corners]).sum(1).float()
        _, _, alb, rgh, _ = _attributes(net, mat_net, x, float(mesh.meta.get('level', 0.0)), _max_move(mesh),
                                        bool(baked.meta.get('project', True)))
        tex = sample_textures(baked, face, bary)
        w = bary.float()[:, :, None]
        v_alb = (w * mesh.diffuse_albedo[corners]).sum(1)
        v_rgh = (w * mesh.roughness.reshape(-1, 1)[corners]).sum(1)[:, 0]
        r = {'samples': samples, 'size': baked.atlas.size}
        for name, got, want in (('texture_albedo', tex['diffuse_albedo'], alb), ('texture_roughness', tex['roughness'][:, 0], rgh),
                                ('vertex_albedo', v_alb, alb), ('vertex_roughness', v_rgh, rgh)):
            d = (got.double() - want.double()).abs()
            r[name + '_mean'], r[name + '_max'] = d.mean().item(), d.max().item()
    return r


# ---- ambient occlusion and bent normals, traced against the SDF ------------------------------------------
MAX_AO_RAYS = ops.BAKE_AO_MAX_RAYS


@dataclass
class BakedOcclusion:
    ao: torch.Tensor                             # [T,T] float32: the unoccluded share of the cosine-weighted hemisphere
    bent_normal: torch.Tensor                    # [T,T,3] float32, object space: the mean unoccluded direction, unit length
    meta: dict = field(default_factory=dict)


def _check_occlusion(what, rays, distance, bias, seed):
    """(rays, distance or None, bias, seed) as numbers; ValueError outside what the kernels take"""
    rays = int(rays)
    if not 1 <= rays <= MAX_AO_RAYS:
        raise ValueError('%s: rays must lie in 1 .. %d, got %d' % (what, MAX_AO_RAYS, rays))
    if distance is not None:
        distance = float(distance)
        if not distance > 0.0:
            raise ValueError('%s: distance must be positive (None: unbounded), got %r' % (what, distance))
    bias = float(bias)
    if not bias >= 0.0:
        raise ValueError('%s: bias must not be negative, got %r' % (what, bias))
    seed = int(seed)
    if not 0 <= seed < 1 << 32:
        raise ValueError('%s: seed must lie in 0 .. 2^32 - 1, got %d' % (what, seed))
    return rays, distance, bias, seed


def _occlusion(model, x, normal, texel, rays, distance, bias, seed, per, level, max_move):
    """(ao [N], bent [N,3], how many points lie further than max_move from the level set) of the points x [N,3] with unit
    normals and sequence indices texel [N] int64, in slices of `per` points: the SDF and |gradient| at x, the ray kernel, one
    trace of the slice's rays against the model's own surface, the accumulate kernel"""
    from .model.path_tracing_render import trace_occluders
    net = _implicit(model)
    N = x.shape[0]
    ao = torch.empty(N, device=x.device, dtype=torch.float32)
    bent = torch.empty(N, 3, device=x.device, dtype=torch.float32)
    off = torch.zeros((), device=x.device, dtype=torch.int64)
    for s in range(0, N, per):
        xs, ns, g = x[s:s + per].contiguous(), normal[s:s + per].contiguous(), texel[s:s + per].contiguous()
        m = xs.shape[0]
        sdf, _, grad = net.value_feature_gradient(xs)
        sdf = sdf.float().reshape(m).contiguous()
        if level != 0.0:
            sdf = sdf - level
        gnorm = grad.float().norm(dim=1).clamp_min(1e-12)
        off += (sdf.abs() / gnorm > max_move).sum()
        origins, dirs, _ = ops.bake_ao_rays(xs, ns, sdf, gnorm, g, rays, seed, bias)
        pts, hit = trace_occluders(origins.unsqueeze(0).expand(rays, m, 3).reshape(-1, 3), dirs, model)
        ao[s:s + m], bent[s:s + m] = ops.bake_ao_accumulate(hit.view(rays, m), pts.float().contiguous().view(rays, m, 3), origins,
                                                            dirs, ns, 0.0 if distance is None else distance)
    return ao, bent, off


def bake_occlusion(model, mesh, baked, rays=64, distance=None, bias=0.0, seed=0, ray_chunk=2 ** 22):
    """Ambient occlusion and bent normals of the texels of `baked` (bake_textures of `model` over `mesh`), traced against the
    model's own SDF -> BakedOcclusion(ao [T,T], bent_normal [T,T,3], meta), float32 on the GPU, zeros on unowned texels.
    Every owned texel (the gutters too: bilinear lookups read them) sends `rays` cosine-weighted rays from its surface point
    baked.position - lifted to first order onto the level set and by `bias` along baked.normal - through the eval-mode tracer
    the renderer's secondary rays use; a ray occludes when it hits the surface, within `distance` if that is given.  ao is the
    share of rays that do not, bent_normal their normalised sum.  Texels are taken in slices of ray_chunk // rays; a texel's
    directions depend on its index, the sample, rays and seed alone, so the slicing changes no bit, and two bakes give the
    same bits.  meta: rays, distance, bias, seed, traced_rays, off_surface_texels (owned texels further than the mesh's
    projection bound from the level set, to first order), ao_s (HIP events), mean_ao_covered.
    ValueError for a bake with project=False (points left on the faces may lie inside the surface), rays outside 1 .. 1024,
    a distance that is not positive, a negative bias, a ray_chunk below one texel's rays."""
    rays, distance, bias, seed = _check_occlusion('bake_occlusion', rays, distance, bias, seed)
    ray_chunk = int(ray_chunk)
    if ray_chunk < rays:
        raise ValueError('bake_occlusion: ray_chunk must hold the %d rays of one texel, got %d' % (rays, ray_chunk))
    if not baked.meta.get('project', False):
        raise ValueError('bake_occlusion needs a bake with project=True: texels left on the faces of the mesh may lie inside '
                         'the surface, where every ray is occluded')
    _check(model, mesh, 'bake_occlusion')
    T = baked.atlas.size
    dev = baked.owner.device
    with torch.no_grad():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        idx = (baked.owner.reshape(-1) >= 0).nonzero()[:, 0]
        x, normal = baked.position.reshape(-1, 3)[idx], baked.normal.reshape(-1, 3)[idx]
        ao, bent, off = _occlusion(model, x, normal, idx, rays, distance, bias, seed, min(ray_chunk // rays, NETWORK_BATCH),
                                   float(mesh.meta.get('level', 0.0)), _max_move(mesh))
        ao_map = torch.zeros(T * T, device=dev, dtype=torch.float32)
        bent_map = torch.zeros(T * T, 3, device=dev, dtype=torch.float32)
        ao_map[idx], bent_map[idx] = ao, bent
        ev[1].record()
        covered = baked.covered.reshape(-1)
        mean_covered = ao_map[covered].double().mean().item() if idx.shape[0] else 0.0
        torch.cuda.synchronize(dev)
    meta = dict(rays=rays, distance=distance, bias=bias, seed=seed, traced_rays=rays * int(idx.shape[0]),
                off_surface_texels=int(off), ao_s=ev[0].elapsed_time(ev[1]) / 1e3, mean_ao_covered=mean_covered)
    return BakedOcclusion(ao_map.view(T, T), bent_map.view(T, T, 3), meta)


def encode_occlusion(baked, occ):
    """dict(ao [T,T], bent_normal [T,T,4], orm [T,T,4]) uint8 on the GPU, as the PNGs hold them, through ops.bake_encode with
    the occlusion in the roughness slot and the bent normal in the normal slot: ao linear, bent_normal as 0.5 n + 0.5 in object
    space; orm is the glTF packing R = occlusion, G = roughness, B = 0 (no metal), alpha 255 on owned texels"""
    T = baked.atlas.size
    albedo, owner = baked.diffuse_albedo.reshape(-1, 3), baked.owner.reshape(-1)
    bent = occ.bent_normal.reshape(-1, 3)
    _, n8, ao8 = ops.bake_encode(albedo, occ.ao.reshape(-1), bent, owner)
    _, _, r8 = ops.bake_encode(albedo, baked.roughness.reshape(-1), bent, owner)
    orm = torch.stack([ao8, r8, torch.zeros_like(ao8), n8[:, 3]], 1)
    return {'ao': ao8.view(T, T), 'bent_normal': n8.view(T, T, 4), 'orm': orm.view(T, T, 4)}


def verify_occlusion(model, mesh, baked, occ, samples, rays=256, seed=0):
    """What the occlusion map loses, measured against a direct estimate: `samples` area-weighted random points of the mesh
    (sample_faces) are moved onto the level set as bake_textures moves its texels, and the occlusion is estimated there with
    `rays` rays of their own (the sample's index plays the texel's part in the sequence; distance and bias are the bake's).
    -> dict: samples, size, rays, bake_rays, ao_mean / ao_max (mean and max |bilinear lookup - estimate|), direct_mean,
    noise_floor = mean sqrt(a (1 - a) / bake_rays) over the estimates a - the binomial spread a texel of the bake has by
    itself - and verify_noise_floor, the same with `rays`.  A report, not an assertion."""
    _check(model, mesh, 'verify_occlusion')
    samples = int(samples)
    if samples < 1:
        raise ValueError('samples must be positive, got %d' % samples)
    rays, distance, bias, seed = _check_occlusion('verify_occlusion', rays, occ.meta['distance'], occ.meta['bias'], seed)
    net = _implicit(model)
    level, max_move = float(mesh.meta.get('level', 0.0)), _max_move(mesh)
    a = baked.atlas
    with torch.no_grad():
        faces = mesh.faces.long()
        face, bary = sample_faces(mesh.verts, faces, samples, torch.Generator().manual_seed(int(seed)))
        x = (bary[:, :, None] * mesh.verts.double()[faces[face]]).sum(1).float().contiguous()
        x = project_to_level_set(lambda y: net.value_feature_gradient(y)[::2], x, level, max_move=max_move)
        g = net.value_feature_gradient(x)[2]
        normal = (g / g.norm(dim=1, keepdim=True).clamp_min(1e-12)).float().contiguous()
        texel = torch.arange(samples, device=x.device, dtype=torch.int64)
        est, _, _ = _occlusion(model, x, normal, texel, rays, distance, bias, seed, max(1, min(2 ** 22 // rays, NETWORK_BATCH)),
                               level, max_move)
        got = ops.texture_sample(occ.ao.unsqueeze(2).contiguous(), face.to(torch.int32).contiguous(), bary.contiguous(),
                                 a.cells_per_row, a.cell, a.pad)[:, 0]
        d = (got.double() - est.double()).abs()
        var = (est.double() * (1.0 - est.double())).clamp_min(0.0)
        K = int(occ.meta['rays'])
        return {'samples': samples, 'size': a.size, 'rays': rays, 'bake_rays': K, 'ao_mean': d.mean().item(),
                'ao_max': d.max().item(), 'direct_mean': est.double().mean().item(),
                'noise_floor': (var / K).sqrt().mean().item(), 'verify_noise_floor': (var / rays).sqrt().mean().item()}


# ---- the diffuse lightmap under a map light, MIS-sampled and traced against the SDF ---------------------
@dataclass
class BakedIrradiance:
    irradiance: torch.Tensor                     # [T,T,3] float32, linear: the direct irradiance E of each owned texel
    noise: torch.Tensor                          # [T,T] float32: the estimated standard error of E's luminance (mean of rgb)
    meta: dict = field(default_factory=dict)


def _check_irradiance(what, light, rays, map_share, bias, seed, rotation):
    """(K_cos, K_map, bias, seed, R or None): the shares of the rays, and the light's rotation composed with `rotation` as a
    float32 [3,3] tensor on the light's device (None: the identity); ValueError outside what the kernels take"""
    from .lighting import EnvmapLight, is_identity_rotation
    if not isinstance(light, EnvmapLight):
        raise ValueError('%s: light must be a lighting.EnvmapLight, got %s' % (what, type(light).__name__))
    map_share = float(map_share)
    if not 0.0 <= map_share <= 1.0:
        raise ValueError('%s: map_share must lie in [0, 1], got %r' % (what, map_share))
    rays, _, bias, seed = _check_occlusion(what, rays, None, bias, seed)
    K_map = int(round(rays * map_share))
    R = light.rotation if rotation is None else light._composed(rotation)[0]
    if R is not None and is_identity_rotation(R):
        R = None
    return rays - K_map, K_map, bias, seed, None if R is None else R.to(light.envmap.device).contiguous()


def _irradiance(model, x, normal, texel, K_cos, K_map, light, R, bias, seed, per, level, max_move):
    """(E [N,3], noise [N], points further than max_move from the level set, rays traced, rays skipped) of the points x [N,3]
    with unit normals and sequence indices texel [N] int64, in slices of `per` points: the SDF and |gradient| at x, the ray
    kernel, one trace of the slice's rays that carry a weight - compacted, their hit mask scattered back - and the accumulate
    kernel, which never reads the mask of the others"""
    from .model.path_tracing_render import trace_occluders
    net = _implicit(model)
    N, K = x.shape[0], K_cos + K_map
    E = torch.empty(N, 3, device=x.device, dtype=torch.float32)
    noise = torch.empty(N, device=x.device, dtype=torch.float32)
    off = torch.zeros((), device=x.device, dtype=torch.int64)
    traced = 0
    for s in range(0, N, per):
        xs, ns, g = x[s:s + per].contiguous(), normal[s:s + per].contiguous(), texel[s:s + per].contiguous()
        m = xs.shape[0]
        sdf, _, grad = net.value_feature_gradient(xs)
        sdf = sdf.float().reshape(m).contiguous()
        if level != 0.0:
            sdf = sdf - level
        gnorm = grad.float().norm(dim=1).clamp_min(1e-12)
        off += (sdf.abs() / gnorm > max_move).sum()
        origins, dirs, weight, _ = ops.bake_irradiance_rays(xs, ns, sdf, gnorm, g, K_cos, K_map, light.envmap, light.table,
                                                            light.coordinate_type, seed, bias, rot=R)
        lit = (weight != 0).any(dim=2).reshape(-1).nonzero()[:, 0]         # row s of texel k sits at s m + k
        hit = torch.zeros(K * m, device=x.device, dtype=torch.uint8)
        if lit.shape[0]:
            _, h = trace_occluders(origins[lit % m], dirs.reshape(-1, 3)[lit], model)
            hit[lit] = h.to(torch.uint8)
        traced += int(lit.shape[0])
        E[s:s + m], noise[s:s + m] = ops.bake_irradiance_accumulate(hit.view(K, m), weight, K_cos, K_map)
    return E, noise, off, traced, K * N - traced


def bake_irradiance(model, mesh, baked, light, rays=64, map_share=0.5, bias=0.0, seed=0, rotation=None, ray_chunk=2 ** 22):
    """The diffuse lightmap of the texels of `baked` (bake_textures of `model` over `mesh`) under the map light `light` (a
    lighting.EnvmapLight) -> BakedIrradiance(irradiance [T,T,3], noise [T,T], meta), float32 on the GPU, zeros on unowned
    texels: the direct irradiance E(x) = integral of L(R^T w) V(x, w) max(n . w, 0) dw, with L the map's nearest texel as the
    renderer reads it, V the visibility against the model's own SDF and R the light's rotation (its own, with `rotation` [3,3],
    world-from-light, on top).  There is no interreflection: a ray that hits the surface contributes nothing.
    Every owned texel sends `rays` rays from its surface point (lifted as bake_occlusion lifts it): rays - K_map
    cosine-weighted ones - bake_occlusion's own sequence - and K_map = round(rays map_share) drawn from the map's distribution,
    combined by the multi-sample balance heuristic (ops.bake_irradiance_rays).  Only rays with a non-zero weight are traced
    (a map ray below the horizon, a ray into a black texel have none).  noise is the estimated standard error of E's luminance.
    Texels are taken in slices of ray_chunk // rays; neither the slicing nor the compaction changes a bit, and two bakes give
    the same bits.  meta: rays, rays_cos, rays_map, bias, seed, traced_rays, skipped_rays, off_surface_texels, irradiance_s
    (HIP events), mean_irradiance_covered (the luminance of E) and mean_noise_covered.
    ValueError for a light that is no EnvmapLight, a bake with project=False, rays outside 1 .. 1024, a map_share outside
    [0, 1], a negative bias, a ray_chunk below one texel's rays."""
    K_cos, K_map, bias, seed, R = _check_irradiance('bake_irradiance', light, rays, map_share, bias, seed, rotation)
    rays = K_cos + K_map
    ray_chunk = int(ray_chunk)
    if ray_chunk < rays:
        raise ValueError('bake_irradiance: ray_chunk must hold the %d rays of one texel, got %d' % (rays, ray_chunk))
    if not baked.meta.get('project', False):
        raise ValueError('bake_irradiance needs a bake with project=True: texels left on the faces of the mesh may lie inside '
                         'the surface, where every ray is occluded')
    _check(model, mesh, 'bake_irradiance')
    T = baked.atlas.size
    dev = baked.owner.device
    with torch.no_grad():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        idx = (baked.owner.reshape(-1) >= 0).nonzero()[:, 0]
        x, normal = baked.position.reshape(-1, 3)[idx], baked.normal.reshape(-1, 3)[idx]
        E, noise, off, traced, skipped = _irradiance(model, x, normal, idx, K_cos, K_map, light, R, bias, seed,
                                                     min(ray_chunk // rays, NETWORK_BATCH),
                                                     float(mesh.meta.get('level', 0.0)), _max_move(mesh))
        e_map = torch.zeros(T * T, 3, device=dev, dtype=torch.float32)
        n_map = torch.zeros(T * T, device=dev, dtype=torch.float32)
        e_map[idx], n_map[idx] = E, noise
        ev[1].record()
        covered = baked.covered.reshape(-1)
        any_covered = bool(covered.any())
        mean_e = e_map[covered].double().mean().item() if any_covered else 0.0
        mean_n = n_map[covered].double().mean().item() if any_covered else 0.0
        torch.cuda.synchronize(dev)
    meta = dict(rays=rays, rays_cos=K_cos, rays_map=K_map, bias=bias, seed=seed, traced_rays=traced, skipped_rays=skipped,
                off_surface_texels=int(off), irradiance_s=ev[0].elapsed_time(ev[1]) / 1e3, mean_irradiance_covered=mean_e,
                mean_noise_covered=mean_n)
    return BakedIrradiance(e_map.view(T, T, 3), n_map.view(T, T), meta)


def encode_irradiance(baked, irr, exposure=1.0):
    """dict(irradiance [T,T,3] float32 - the linear map, as the EXR holds it - and lit [T,T,4] uint8 on the GPU, as the PNG
    holds it): the diffuse radiance exposure albedo E / pi of every texel (the product in fp64, rounded once) through the
    transfer of the renderer's own PNGs and of the albedo map - clamp at 0, power 1 / 2.2, clamp to [0, 1], floor(255 x + 0.5)
    (ops.bake_encode) - alpha 255 on owned texels, all bytes 0 elsewhere"""
    T = baked.atlas.size
    exposure = float(exposure)
    if not exposure >= 0.0 or math.isinf(exposure):
        raise ValueError('encode_irradiance: exposure must be finite and not negative, got %r' % exposure)
    radiance = (exposure * baked.diffuse_albedo.double() * irr.irradiance.double() / math.pi).float().reshape(-1, 3).contiguous()
    lit, _, _ = ops.bake_encode(radiance, baked.roughness.reshape(-1), baked.normal.reshape(-1, 3), baked.owner.reshape(-1))
    return {'irradiance': irr.irradiance, 'lit': lit.view(T, T, 4)}


def verify_irradiance(model, mesh, baked, irr, light, samples, rays=256, seed=0, rotation=None):
    """What the lightmap loses, measured against a direct estimate: `samples` area-weighted random points of the mesh
    (sample_faces) are moved onto the level set as bake_textures moves its texels, and the irradiance is estimated there with
    `rays` rays of their own (the sample's index plays the texel's part in the sequence; the map's share of the rays and the
    bias are the bake's; light and rotation must be the bake's too).  -> dict: samples, size, rays, bake_rays,
    irradiance_mean / irradiance_max (mean and max |bilinear lookup - estimate| of the luminance), direct_mean (the mean
    luminance of the estimates), noise_mean (the bake's own mean noise over its covered texels) and verify_noise_mean (the
    estimates' own).  A report, not an assertion."""
    _check(model, mesh, 'verify_irradiance')
    samples = int(samples)
    if samples < 1:
        raise ValueError('samples must be positive, got %d' % samples)
    share = irr.meta['rays_map'] / irr.meta['rays']
    K_cos, K_map, bias, seed, R = _check_irradiance('verify_irradiance', light, rays, share, irr.meta['bias'], seed, rotation)
    rays = K_cos + K_map
    net = _implicit(model)
    level, max_move = float(mesh.meta.get('level', 0.0)), _max_move(mesh)
    a = baked.atlas
    with torch.no_grad():
        faces = mesh.faces.long()
        face, bary = sample_faces(mesh.verts, faces, samples, torch.Generator().manual_seed(int(seed)))
        x = (bary[:, :, None] * mesh.verts.double()[faces[face]]).sum(1).float().contiguous()
        x = project_to_level_set(lambda y: net.value_feature_gradient(y)[::2], x, level, max_move=max_move)
        g = net.value_feature_gradient(x)[2]
        normal = (g / g.norm(dim=1, keepdim=True).clamp_min(1e-12)).float().contiguous()
        texel = torch.arange(samples, device=x.device, dtype=torch.int64)
        est, est_noise, _, _, _ = _irradiance(model, x, normal, texel, K_cos, K_map, light, R, bias, seed,
                                              max(1, min(2 ** 22 // rays, NETWORK_BATCH)), level, max_move)
        got = ops.texture_sample(irr.irradiance.contiguous(), face.to(torch.int32).contiguous(), bary.contiguous(),
                                 a.cells_per_row, a.cell, a.pad)
        want = est.double().mean(dim=1)
        d = (got.double().mean(dim=1) - want).abs()
        return {'samples': samples, 'size': a.size, 'rays': rays, 'bake_rays': int(irr.meta['rays']),
                'irradiance_mean': d.mean().item(), 'irradiance_max': d.max().item(), 'direct_mean': want.mean().item(),
                'noise_mean': float(irr.meta['mean_noise_covered']), 'verify_noise_mean': est_noise.double().mean().item()}
