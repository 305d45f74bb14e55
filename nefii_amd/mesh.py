"""Mesh export of a trained SDF and the materials on it (utils/plots.py:127-241, get_surface_trace /
get_surface_high_res_mesh, without skimage or trimesh).

    verts, faces = marching_cubes(volume, level)                  # skimage-like primitive on CUDA tensors
    vol = sdf_grid(model.implicit_network, 512, bound)            # the SDF on linspace(-bound, bound, 512)^3
    mesh = extract_mesh(model, resolution=512)                    # vertices, normals, per-vertex materials
    labels = connected_components(faces, V)                       # smallest vertex index of each vertex's component
    mesh = select_components(mesh, 'largest')                     # drop the floaters
    mesh = extract_mesh(model, resolution=512, high_res=True, keep='largest')   # re-meshed on a tight aligned grid

The grid is evaluated by the tracer's evaluator and meshed by csrc/nefii_mcubes.hip; normals and materials come from the
fused evaluators the renderer uses.  Vertices stay in the model's normalised object space.  Components are labelled by
csrc/nefii_meshcc.hip; the tables and the selection around it are torch code that runs on any device.
"""
import math
import os
import time
from dataclasses import dataclass, field, replace
from typing import Optional

import numpy as np
import torch

from . import ops


def marching_cubes(volume, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """(verts [V,3] float32, faces [F,3] int64) of the level set of volume [nx, ny, nz] (a CUDA tensor), like
    skimage.measure.marching_cubes: vertex = origin + index * spacing, faces wound so that their normals point towards
    increasing values (outward for an SDF).  Welded vertices, deterministic order (include/nefii_amd.h, ABI 17).  A
    volume with no crossing gives [0, 3] tensors.  ValueError for CPU tensors, non-finite values and volumes of 2^31
    points or more."""
    if not torch.is_tensor(volume) or not volume.is_cuda:
        raise ValueError('marching_cubes needs a CUDA tensor (the hot path has no CPU fallback)')
    if volume.dim() != 3 or min(volume.shape) < 2:
        raise ValueError('volume must be [nx, ny, nz] with every dim >= 2, got %s' % (tuple(volume.shape),))
    if volume.numel() > ops.MCUBES_MAX_POINTS:
        raise ValueError('volume of %d points: marching_cubes needs fewer than 2^31' % volume.numel())
    if not math.isfinite(float(level)):
        raise ValueError('level must be finite')
    vol = volume.detach().to(torch.float32).contiguous()
    if not bool(torch.isfinite(vol).all()):
        raise ValueError('volume holds non-finite values')
    verts, faces = ops.marching_cubes(vol, level, origin, spacing)
    return verts, faces.long()


def _tracer_precision(model):
    rt = getattr(model, 'ray_tracer', None)
    return getattr(rt, 'precision', None) or os.environ.get('NEFII_TRACER_PRECISION', 'f16x3w')


def grid_axis(resolution, bound, device):
    """the grid points along one axis: linspace(-bound, bound, resolution) (plots.get_grid_uniform)"""
    return torch.linspace(-bound, bound, resolution, device=device, dtype=torch.float32)


def sdf_grid(implicit_network, resolution, bound, chunk=2 ** 24, precision=None):
    """vol [r, r, r] float32: the SDF at linspace(-bound, bound, r)^3, x slowest (vol[i, j, k] at (x_i, y_j, z_k)).  The
    tracer's evaluator for this net: ops.sdf_eval on the split-precision packing (precision 'f16x3*', the default), else
    implicit_network(x).  Evaluated in chunks of `chunk` points, under no_grad (frozen geometry, as when rendering)."""
    if resolution < 2:
        raise ValueError('resolution must be >= 2')
    if resolution ** 3 > ops.MCUBES_MAX_POINTS:
        raise ValueError('resolution %d: the grid needs fewer than 2^31 points' % resolution)
    precision = precision or os.environ.get('NEFII_TRACER_PRECISION', 'f16x3w')
    dev = next(implicit_network.parameters()).device
    ax = grid_axis(resolution, float(bound), dev)
    n = resolution ** 3
    out = torch.empty(n, device=dev, dtype=torch.float32)
    with torch.no_grad():
        split = precision.startswith('f16x3')
        pm = implicit_network.packed(f16x3=True) if split else None
        for s in range(0, n, chunk):
            idx = torch.arange(s, min(n, s + chunk), device=dev, dtype=torch.int64)
            x = torch.stack([ax[idx // (resolution * resolution)], ax[(idx // resolution) % resolution],
                             ax[idx % resolution]], 1)
            out[s:s + idx.shape[0]] = ops.sdf_eval(pm, x) if split else implicit_network(x)[:, 0]
    return out.view(resolution, resolution, resolution)


@dataclass
class Mesh:
    verts: torch.Tensor                          # [V,3] float32, normalised object space
    faces: torch.Tensor                          # [F,3] int64
    normals: Optional[torch.Tensor] = None       # [V,3] normalised SDF gradient
    diffuse_albedo: Optional[torch.Tensor] = None        # [V,3]
    roughness: Optional[torch.Tensor] = None             # [V,1]
    specular_reflection: Optional[torch.Tensor] = None   # [V,3], specular_inv_remap of the reflectance
    meta: dict = field(default_factory=dict)     # resolution, level, bound, timings (s)


VERTEX_ATTRIBUTES = ('normals', 'diffuse_albedo', 'roughness', 'specular_reflection')
COMPONENT_ROWS = 16                              # rows of the component table kept in Mesh.meta


def _implicit(model):
    return model.implicit_network if hasattr(model, 'implicit_network') else model


# ---- connected components (plots.py:186-189: trimesh's split, the component of the largest area) ---------------------
def _components(faces, n_verts):
    """(labels [V] int64, rounds) through ops.mesh_components.  int64 indices that int32 cannot hold become -1 or V,
    which the kernel refuses like any other index outside [0, V)."""
    if not torch.is_tensor(faces) or not faces.is_cuda:
        raise ValueError('connected_components needs a CUDA tensor (the hot path has no CPU fallback)')
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError('faces must be [F, 3], got %s' % (tuple(faces.shape),))
    n_verts = int(n_verts)
    if n_verts < 0 or n_verts >= 1 << 31:
        raise ValueError('n_verts = %d must lie in 0 .. 2^31 - 1' % n_verts)
    if faces.dtype != torch.int32:
        faces = faces.clamp(-1, n_verts).to(torch.int32)
    label, rounds = ops.mesh_components(faces.contiguous(), n_verts)
    return label.long(), rounds


def connected_components(faces, n_verts):
    """labels [V] int64: labels[v] = the smallest vertex index of the edge-connected component of vertex v of the mesh
    faces [F,3] (int32 or int64, as marching_cubes returns them, on the GPU); a vertex in no face labels itself.  Bitwise
    the same for any order of the faces.  ValueError for CPU tensors and for an index outside [0, n_verts)."""
    return _components(faces, n_verts)[0]


def component_table(verts, faces, labels):
    """(ids [C] int64 ascending, n_verts [C] int64, n_faces [C] int64, area [C] float64): one row per component of labels
    [V] (any labelling constant on components).  A face belongs to the component of its first vertex.  No float atomics:
    the faces are sorted (stably) by label and their fp64 areas summed by cumsum, so the table is bitwise reproducible.
    Works on any device."""
    labels = labels.long()
    faces = faces.long()
    ids, n_v = torch.unique(labels, sorted=True, return_counts=True)
    fl = labels[faces[:, 0]]
    fl, order = torch.sort(fl, stable=True)
    v = verts.double()
    a, b, c = (v[faces[order, k]] for k in range(3))
    area = 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1)
    csum = torch.cat([area.new_zeros(1), torch.cumsum(area, 0)])
    lo = torch.searchsorted(fl, ids, right=False)
    hi = torch.searchsorted(fl, ids, right=True)
    return ids, n_v, hi - lo, csum[hi] - csum[lo]


def _parse_keep(keep):
    if isinstance(keep, str):
        if keep in ('all', 'largest'):
            return keep
        try:
            keep = float(keep)
        except ValueError:
            raise ValueError("keep must be 'all', 'largest' or a fraction in (0, 1], got %r" % (keep,))
    keep = float(keep)
    if not 0.0 < keep <= 1.0:
        raise ValueError("keep must be 'all', 'largest' or a fraction in (0, 1], got %r" % (keep,))
    return keep


def select_components(mesh, keep, labels=None):
    """The components of `mesh` that `keep` names: 'all' - the mesh itself, untouched; 'largest' - the one of the largest
    area (ties: the smaller id); a fraction x in (0, 1] - every component of at least x times the largest area.  A new
    Mesh: the kept vertices in their old order, the faces re-indexed in their old order, every per-vertex attribute carried
    along.  meta['components'] is the table of the INPUT (count, and the COMPONENT_ROWS largest rows).  labels: the
    components, when the caller has them (then any device will do); else connected_components labels them, and meta gains
    cc_rounds and cc_s (s, host clock around the labelling, which synchronises)."""
    keep = _parse_keep(keep)
    if keep == 'all':
        return mesh
    V = mesh.verts.shape[0]
    meta = dict(mesh.meta)
    if labels is None:
        t0 = time.perf_counter()
        labels, rounds = _components(mesh.faces, V)
        meta['cc_rounds'] = meta.get('cc_rounds', 0) + rounds
        meta['cc_s'] = meta.get('cc_s', 0.0) + time.perf_counter() - t0
    labels = labels.long()
    ids, n_v, n_f, area = component_table(mesh.verts, mesh.faces, labels)
    if ids.numel() == 0:
        meta['components'] = dict(count=0, ids=[], n_verts=[], n_faces=[], area=[])
        return replace(mesh, meta=meta)
    top = area.max()
    if keep == 'largest':
        kept = ids[(area == top).nonzero()[:1, 0]]               # ids ascend: the first of the largest is the smaller id
    else:
        kept = ids[area >= keep * top]
    rows = torch.sort(area, descending=True, stable=True)[1][:COMPONENT_ROWS]
    meta['components'] = dict(count=int(ids.numel()), ids=ids[rows].tolist(), n_verts=n_v[rows].tolist(),
                              n_faces=n_f[rows].tolist(), area=area[rows].tolist())
    vmask = torch.isin(labels, kept)
    new_index = torch.cumsum(vmask, 0) - 1
    faces = mesh.faces.long()
    faces = new_index[faces[vmask[faces[:, 0]]]]
    out = Mesh(mesh.verts[vmask], faces, meta=meta)
    for name in VERTEX_ATTRIBUTES:
        t = getattr(mesh, name)
        if t is not None:
            setattr(out, name, t[vmask])
    return out


# ---- the aligned grid of get_surface_high_res_mesh (plots.py:194-204, get_grid :257-288) -----------------------------
@dataclass
class AlignedGrid:
    mean: np.ndarray                             # [3] float64, the frame's origin in world space
    vecs: np.ndarray                             # [3,3] float64, rows = the frame's axes: local = vecs @ (p - mean)
    axes: list                                   # three float64 arrays: the grid points along the local x, y, z
    spacing: float                               # the step of all three axes
    shortest_axis: int

    @property
    def shape(self):
        return tuple(len(a) for a in self.axes)

    @property
    def origin(self):
        """the local coordinates of grid point (0, 0, 0)"""
        return tuple(float(a[0]) for a in self.axes)

    def numel(self):
        return len(self.axes[0]) * len(self.axes[1]) * len(self.axes[2])

    def to_local(self, p):
        """[N,3] world -> [N,3] float64 local"""
        p = p.double()
        return (p - torch.as_tensor(self.mean, device=p.device)) @ torch.as_tensor(self.vecs, device=p.device).T

    def to_world(self, local_verts):
        """[N,3] local -> [N,3] float64 world: vecs^T local + mean"""
        q = local_verts.double()
        return q @ torch.as_tensor(self.vecs, device=q.device) + torch.as_tensor(self.mean, device=q.device)

    def points(self, start, stop, device=None):
        """[stop - start, 3] float32: the world-space grid points of the linear indices start .. stop - 1, x slowest (point
        (i * ny + j) * nz + k sits at the local (x_i, y_j, z_k)); fp64 arithmetic, rounded once"""
        nx, ny, nz = self.shape
        ax = [torch.as_tensor(a, device=device) for a in self.axes]
        idx = torch.arange(start, stop, device=device, dtype=torch.int64)
        local = torch.stack([ax[0][idx // (ny * nz)], ax[1][(idx // nz) % ny], ax[2][idx % nz]], 1)
        return self.to_world(local).float()


def grid_axes(lo, hi, resolution, margin):
    """get_grid (plots.py:257-288) in its own expressions: the axis of the shortest extent has `resolution` points from
    min - margin to max + margin, the others the same step.  lo, hi: [3] float64 arrays -> (axes, step, shortest axis)"""
    shortest = int(np.argmin(hi - lo))
    s = np.linspace(lo[shortest] - margin, hi[shortest] + margin, resolution)
    length = np.max(s) - np.min(s)
    step = length / (s.shape[0] - 1)
    axes = [s if a == shortest else np.arange(lo[a] - margin, hi[a] + step + margin, step) for a in range(3)]
    return axes, float(step), shortest


def aligned_grid(points, resolution, margin=0.2):
    """The PCA-aligned grid around points [N,3]: the frame of plots.py:194-204 and the grid of get_grid.  Mean and 3 x 3
    scatter in fp64; torch.linalg.eigh on the host; the rows of vecs are the eigenvectors in ascending eigenvalue order,
    each signed so that its entry of the largest magnitude is positive, then row 0 negated if det < 0 (a proper rotation,
    and a deterministic one).  The reference fits the frame to 10 000 random surface samples; here the caller passes all
    vertices of the kept component, whose box contains the box of any sample.  ValueError, before anything is allocated,
    for a grid of more than ops.MCUBES_MAX_POINTS points."""
    resolution = int(resolution)
    if resolution < 2:
        raise ValueError('resolution must be >= 2')
    if not float(margin) >= 0.0 or not math.isfinite(float(margin)):
        raise ValueError('margin must be finite and not negative')
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise ValueError('points must be [N, 3] with N >= 1, got %s' % (tuple(points.shape),))
    p = points.detach().double()
    mean = p.mean(0)
    d = p - mean
    scatter = (d.T @ d).cpu()
    vecs = torch.linalg.eigh(scatter)[1].T.contiguous()
    for r in range(3):
        if vecs[r, vecs[r].abs().argmax()] < 0:
            vecs[r] = -vecs[r]
    if torch.det(vecs) < 0:
        vecs[0] = -vecs[0]
    local = d @ vecs.to(p.device).T
    lo, hi = local.min(0)[0].cpu().numpy(), local.max(0)[0].cpu().numpy()
    axes, step, shortest = grid_axes(lo, hi, resolution, float(margin))
    grid = AlignedGrid(mean.cpu().numpy(), vecs.numpy(), axes, step, shortest)
    if grid.numel() > ops.MCUBES_MAX_POINTS:
        raise ValueError('aligned grid %d x %d x %d = %d points: marching_cubes needs fewer than 2^31'
                         % (grid.shape + (grid.numel(),)))
    return grid


def sdf_grid_on(implicit_network, grid, chunk=2 ** 24, precision=None):
    """vol [nx, ny, nz] float32: the SDF at the points of an AlignedGrid, x slowest; the evaluator is chosen as in
    sdf_grid."""
    precision = precision or os.environ.get('NEFII_TRACER_PRECISION', 'f16x3w')
    dev = next(implicit_network.parameters()).device
    n = grid.numel()
    out = torch.empty(n, device=dev, dtype=torch.float32)
    with torch.no_grad():
        split = precision.startswith('f16x3')
        pm = implicit_network.packed(f16x3=True) if split else None
        for s in range(0, n, chunk):
            x = grid.points(s, min(n, s + chunk), dev)
            out[s:s + x.shape[0]] = ops.sdf_eval(pm, x) if split else implicit_network(x)[:, 0]
    return out.view(*grid.shape)


def extract_mesh(model, resolution=512, level=0.0, bound=None, materials=True, chunk=2 ** 24, keep='all', high_res=False,
                 low_resolution=100, margin=0.2):
    """Mesh of the level set `level` of the SDF of `model` (an IDRNetwork or a bare ImplicitNetwork) on
    linspace(-bound, bound, resolution)^3; bound defaults to model.object_bounding_sphere.  Normals: the normalised SDF
    gradient at the vertices.  With an IDRNetwork and materials=True, also diffuse_albedo / roughness from
    envmap_material_network(verts, feats) and specular_reflection as render.py writes it (global parameters broadcast).

    high_res (plots.get_surface_high_res_mesh): the uniform grid is meshed at low_resolution, its largest component kept,
    and the surface re-meshed on aligned_grid(that component's vertices, resolution, margin) - `resolution` points along
    the component's shortest axis; ValueError when the low-resolution grid has no crossing.  keep ('all', 'largest' or a
    fraction, see select_components) applies to the final mesh before normals and materials are computed.  With the
    defaults the path and the output are those of the uniform grid alone."""
    keep = _parse_keep(keep)
    net = _implicit(model)
    if bound is None:
        if not hasattr(model, 'object_bounding_sphere'):
            raise ValueError('a bare ImplicitNetwork needs an explicit bound')
        bound = model.object_bounding_sphere
    bound = float(bound)
    dev = next(net.parameters()).device
    if dev.type != 'cuda':
        raise ValueError('extract_mesh needs a model on the GPU (the hot path has no CPU fallback)')
    timing = {}
    extra = dict(cc_rounds=0, cc_s=0.0)
    with torch.no_grad():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        if high_res:
            low = sdf_grid(net, low_resolution, bound, chunk=chunk, precision=_tracer_precision(model))
            sp = 2.0 * bound / (low_resolution - 1)
            lv, lf = marching_cubes(low, level, spacing=(sp, sp, sp), origin=(-bound, -bound, -bound))
            del low
            if lv.shape[0] == 0:
                raise ValueError('no surface at level %g inside [-%g, %g]^3 at the low resolution %d'
                                 % (level, bound, bound, low_resolution))
            low_mesh = select_components(Mesh(lv, lf, meta=extra), 'largest')
            extra = dict(cc_rounds=low_mesh.meta['cc_rounds'], cc_s=low_mesh.meta['cc_s'],
                         low_res_components=low_mesh.meta['components'])
            grid = aligned_grid(low_mesh.verts, resolution, margin)
            del lv, lf, low_mesh
            vol = sdf_grid_on(net, grid, chunk=chunk, precision=_tracer_precision(model))
            sp, origin, shape = grid.spacing, grid.origin, grid.shape
        else:
            vol = sdf_grid(net, resolution, bound, chunk=chunk, precision=_tracer_precision(model))
            sp = 2.0 * bound / (resolution - 1)
            origin, shape = (-bound, -bound, -bound), (int(resolution),) * 3
        ev[1].record()
        verts, faces = marching_cubes(vol, level, spacing=(sp, sp, sp), origin=origin)
        ev[2].record()
        del vol
        if high_res:
            verts = grid.to_world(verts).float()
        mesh = Mesh(verts, faces, meta=extra)
        if keep != 'all' and verts.shape[0]:
            mesh = select_components(mesh, keep)
            verts = mesh.verts
        extra = mesh.meta
        if verts.shape[0]:
            _, feat, g = net.value_feature_gradient(verts)
            mesh.normals = g / g.norm(dim=1, keepdim=True).clamp_min(1e-12)
            mat_net = getattr(model, 'envmap_material_network', None)
            if materials and mat_net is not None:
                out = mat_net(verts, feat)
                V = verts.shape[0]
                mesh.diffuse_albedo = out['sg_diffuse_albedo'].float().reshape(V, 3).contiguous()
                mesh.roughness = out['sg_roughness'].float().expand(V, 1).contiguous()
                spec = mat_net.specular_inv_remap(out['sg_specular_reflectance']).float()
                mesh.specular_reflection = spec.expand(V, 3).contiguous()
        torch.cuda.synchronize(dev)
    timing['grid_s'] = ev[0].elapsed_time(ev[1]) / 1e3
    timing['mcubes_s'] = ev[1].elapsed_time(ev[2]) / 1e3
    mesh.meta = dict(resolution=int(resolution), level=float(level), bound=bound, grid_shape=tuple(shape), spacing=float(sp),
                     **timing, **extra)
    return mesh
