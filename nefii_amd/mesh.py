"""Mesh export of a trained SDF and the materials on it (utils/plots.py:127-241, get_surface_trace /
get_surface_high_res_mesh, without skimage or trimesh).

    verts, faces = marching_cubes(volume, level)                  # skimage-like primitive on CUDA tensors
    vol = sdf_grid(model.implicit_network, 512, bound)            # the SDF on linspace(-bound, bound, 512)^3
    mesh = extract_mesh(model, resolution=512)                    # vertices, normals, per-vertex materials
    labels = connected_components(faces, V)                       # smallest vertex index of each vertex's component
    mesh = select_components(mesh, 'largest')                     # drop the floaters
    mesh = extract_mesh(model, resolution=512, high_res=True, keep='largest')   # re-meshed on a tight aligned grid
    small = simplify_mesh(mesh, cell=3 * mesh.meta['spacing'])    # vertex clustering, quadric positions
    mesh = extract_mesh(model, resolution=512, simplify=3)        # simplified, snapped to the level set, re-attributed
    mesh = extract_mesh(model, resolution=2048, sparse=True)      # only the bricks the SDF interval grid cannot rule out

extract_mesh runs in stages: choose the final grid (a UniformGrid, or under high_res the AlignedGrid around a low-resolution
pass), mesh it (_dense_mesh: sdf_on_grid, the tracer's evaluator, then csrc/nefii_mcubes.hip; _sparse_mesh: only the bricks
the network's SDF interval grid leaves undecided, by csrc/nefii_mcubes_sparse.hip - the same mesh, since both ask the grid
object for their points and share csrc/mc_cell.h), then _finish_mesh: keep, simplify, and normals and
materials from the fused evaluators the renderer uses.  Vertices stay in the model's normalised object space.
Components are labelled by csrc/nefii_meshcc.hip; the tables and the selection around it are torch code that runs on any device.
Simplification is vertex clustering with quadric error metrics (Lindstrom 2000): csrc/nefii_meshsimplify.hip places each
cluster's vertex; the clustering, the corner sort and the face bookkeeping are torch code again.
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


class Grid:
    """What the exporter asks of a grid of nx x ny x nz points, x slowest (point (i * ny + j) * nz + k sits at the local
    (x_i, y_j, z_k)): shape, origin (the local coordinates of point (0, 0, 0)), spacing (the step of all three axes),
    points_at(idx, device), frame() and to_world(local).  The dense export evaluates points(start, stop), the sparse one
    points_at(idx): one expression, so the same bits."""

    def numel(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    def points(self, start, stop, device=None):
        """[stop - start, 3] float32: the world-space grid points of the linear indices start .. stop - 1"""
        return self.points_at(torch.arange(start, stop, device=device, dtype=torch.int64), device)

    def _gather(self, ax, idx):
        nx, ny, nz = self.shape
        return torch.stack([ax[0][idx // (ny * nz)], ax[1][(idx // nz) % ny], ax[2][idx % nz]], 1)


class UniformGrid(Grid):
    """linspace(-bound, bound, resolution)^3 (plots.get_grid_uniform); local and world coordinates are the same"""

    def __init__(self, resolution, bound):
        self.resolution, self.bound = int(resolution), float(bound)
        self.shape, self.origin = (self.resolution,) * 3, (-self.bound,) * 3
        self.spacing = 2.0 * self.bound / (self.resolution - 1)

    def axis(self, device):
        return torch.linspace(-self.bound, self.bound, self.resolution, device=device, dtype=torch.float32)

    def points_at(self, idx, device=None):
        """[N,3] float32: the grid points of the linear indices idx [N] (int64, any order), gathered from the fp32 axis"""
        return self._gather([self.axis(idx.device if device is None else device)] * 3, idx)

    def frame(self):
        """(p0, steps) for ops.classify_bricks, as AlignedGrid.frame"""
        sp = self.spacing
        return [-self.bound] * 3, [[sp, 0.0, 0.0], [0.0, sp, 0.0], [0.0, 0.0, sp]]

    def to_world(self, local):
        return local


def uniform_grid(resolution, bound, max_points=None):
    """UniformGrid(resolution, bound); ValueError, before anything is allocated, for fewer than 2 points per axis and for
    more than ops.MCUBES_MAX_POINTS points (max_points as in aligned_grid)"""
    if resolution < 2:
        raise ValueError('resolution must be >= 2')
    if resolution ** 3 > (ops.MCUBES_MAX_POINTS if max_points is None else max_points):
        raise ValueError('resolution %d: the grid needs fewer than 2^31 points' % resolution)
    return UniformGrid(resolution, bound)


def grid_axis(resolution, bound, device):
    """the grid points along one axis: linspace(-bound, bound, resolution) (plots.get_grid_uniform)"""
    return UniformGrid(resolution, bound).axis(device)


def grid_points_at(idx, resolution, bound, device=None):
    """[N,3] float32: the points of sdf_grid's grid at the linear indices idx [N]: UniformGrid.points_at"""
    return UniformGrid(resolution, bound).points_at(idx, device)


def sdf_on_grid(implicit_network, grid, chunk=2 ** 24, precision=None):
    """vol [nx, ny, nz] float32: the SDF at the points of `grid` (a UniformGrid or an AlignedGrid), x slowest (vol[i, j, k]
    at (x_i, y_j, z_k)).  The tracer's evaluator for this net: ops.sdf_eval on the split-precision packing (precision
    'f16x3*', the default), else implicit_network(x).  Evaluated in chunks of `chunk` points, under no_grad (frozen
    geometry, as when rendering)."""
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


def sdf_grid(implicit_network, resolution, bound, chunk=2 ** 24, precision=None):
    """vol [r, r, r] float32: sdf_on_grid on linspace(-bound, bound, r)^3"""
    return sdf_on_grid(implicit_network, uniform_grid(resolution, bound), chunk, precision)


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


# ---- simplification: vertex clustering with quadric error metrics (Lindstrom 2000) ---------------------
def _check_faces(faces, n_verts):
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError('faces must be [F, 3], got %s' % (tuple(faces.shape),))
    if faces.shape[0] and (int(faces.min()) < 0 or int(faces.max()) >= n_verts):
        raise ValueError('faces hold an index outside [0, %d)' % n_verts)


def cluster_vertices(verts, faces, cell):
    """(cluster [V] int64, centre [C,3] float64, C): the uniform grid of cubes of edge `cell` that starts at lo = the least
    corner of the vertices some face uses; vertex v lies in cell floor((v - lo) / cell), in fp64.  The occupied cells are
    numbered by ascending (i, j, k); cluster[v] = -1 for a vertex no face uses; centre = lo + (ijk + 1/2) cell.  Works on any
    device.  ValueError for a cell that is not positive and finite and for a face index outside [0, V)."""
    cell = float(cell)
    if not 0.0 < cell < math.inf:
        raise ValueError('cell must be positive and finite, got %r' % (cell,))
    V = verts.shape[0]
    faces = faces.long()
    _check_faces(faces, V)
    cluster = torch.full((V,), -1, dtype=torch.int64, device=verts.device)
    if faces.shape[0] == 0:
        return cluster, torch.zeros(0, 3, dtype=torch.float64, device=verts.device), 0
    used = torch.zeros(V, dtype=torch.bool, device=verts.device)
    used[faces.reshape(-1)] = True
    v = verts.double()[used]
    lo = v.min(0)[0]
    ijk = torch.floor((v - lo) / cell).long()
    n = ijk.max(0)[0] + 1
    if float(n[0]) * float(n[1]) * float(n[2]) >= 2.0 ** 62:
        raise ValueError('cell %r: the grid of %d x %d x %d cells cannot be numbered' % ((cell,) + tuple(n.tolist())))
    key = (ijk[:, 0] * n[1] + ijk[:, 1]) * n[2] + ijk[:, 2]
    cells, inverse = torch.unique(key, sorted=True, return_inverse=True)
    cluster[used] = inverse
    cijk = torch.stack([cells // (n[1] * n[2]), (cells // n[2]) % n[1], cells % n[2]], 1)
    centre = lo + (cijk.double() + 0.5) * cell
    return cluster, centre, int(cells.shape[0])


def corner_runs(faces, cluster, n_clusters):
    """(corners [3F] int32, seg [C+1] int64): the corners 3 face + k sorted stably by the cluster of their vertex, and each
    cluster's run in that list - what ops.mesh_cluster_quadrics reads.  Every vertex a face uses must have a cluster."""
    key = cluster.long()[faces.long().reshape(-1)]
    key, corners = torch.sort(key, stable=True)
    seg = torch.searchsorted(key, torch.arange(n_clusters + 1, device=key.device, dtype=torch.int64))
    return corners.to(torch.int32), seg


def _cluster_faces(faces, cluster):
    faces = faces.long()
    m = cluster.long()[faces]
    a, b, c = m[:, 0], m[:, 1], m[:, 2]
    idx = ((a != b) & (b != c) & (a != c) & (a >= 0) & (b >= 0) & (c >= 0)).nonzero()[:, 0]
    m = m[idx]
    if m.shape[0] == 0:
        return m, idx, 0
    # rotate the least index to the front: (s0, x, y); the face is an even permutation of its sorted set iff x < y
    first = m.argmin(1)
    ar = torch.arange(m.shape[0], device=m.device)
    x, y = m[ar, (first + 1) % 3], m[ar, (first + 2) % 3]
    even = x < y
    s0, s1, s2 = m[ar, first], torch.minimum(x, y), torch.maximum(x, y)
    n = int(cluster.max()) + 1
    pair = torch.unique(s0 * n + s1, return_inverse=True)[1]           # < F: pair * n + s2 stays far inside int64
    sets, group = torch.unique(pair * n + s2, return_inverse=True)
    n_even = torch.bincount(group[even], minlength=sets.shape[0])
    n_odd = torch.bincount(group[~even], minlength=sets.shape[0])
    cancelled = int((n_even == n_odd).sum())
    wanted = (even & (n_even > n_odd)[group]) | (~even & (n_odd > n_even)[group])     # of the majority orientation
    cand = wanted.nonzero()[:, 0]                                       # ascending: input order
    g, order = torch.sort(group[cand], stable=True)
    head = torch.ones_like(g, dtype=torch.bool)
    head[1:] = g[1:] != g[:-1]
    kept = torch.sort(cand[order[head]])[0]                             # the first of each set, back in input order
    return m[kept], idx[kept], cancelled


def cluster_faces(faces, cluster):
    """(new faces [F',3] int64, kept_face [F'] int64): faces [F,3] with every index replaced by its cluster.  Dropped: a face
    with a repeated index (or a vertex without a cluster); and, among the faces over the same three clusters, all but one -
    the first, in input order, of the orientation (even or odd permutation of the sorted set) that more of them have; where
    both orientations are equally frequent the set is a collapsed thin sheet and all its faces go.  The survivors keep
    their input order; kept_face holds their input indices.  No host loop over the faces; works on any device."""
    return _cluster_faces(faces, cluster)[:2]


def simplify_mesh(mesh, cell, eps=1e-3, clamp=0.5):
    """`mesh` simplified by vertex clustering on a grid of cubes of edge `cell` (cluster_vertices, cluster_faces), every
    cluster's vertex placed by ops.mesh_cluster_quadrics: the minimiser of the summed squared distances to the planes of
    the faces around the cluster's vertices, regularised (eps) towards their mean and kept within clamp cells of the cell's
    centre.  A new Mesh: the clusters some surviving face uses, in ascending cluster order; per-vertex attributes None (they
    would have to be recomputed at the new positions, as extract_mesh does).  meta['simplify'] = cell, clusters, verts_in,
    faces_in, verts, faces, cancelled_sets (vertex sets dropped as collapsed sheets) and timings by HIP events (s):
    simplify_s = cluster_s (clustering and the corner sort) + kernel_s (the op's three launches and the 8-byte read-back
    of its flags) + faces_s (face bookkeeping and re-indexing).
    Clustering does not preserve manifoldness: an edge of the output may carry more than two faces.  An empty mesh comes
    back as it is.  ValueError for a cell that is not positive and finite and for CPU tensors (no CPU fallback)."""
    cell = float(cell)
    if not 0.0 < cell < math.inf:
        raise ValueError('cell must be positive and finite, got %r' % (cell,))
    V, F = mesh.verts.shape[0], mesh.faces.shape[0]
    if V == 0 or F == 0:
        return mesh
    if not mesh.verts.is_cuda or not mesh.faces.is_cuda:
        raise ValueError('simplify_mesh needs CUDA tensors (the hot path has no CPU fallback)')
    dev = mesh.verts.device
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    with torch.no_grad():
        ev[0].record()
        verts = mesh.verts.detach().float().contiguous()
        cluster, centre, C = cluster_vertices(verts, mesh.faces, cell)
        corners, seg = corner_runs(mesh.faces, cluster, C)
        faces32 = mesh.faces.to(torch.int32).contiguous()
        ev[1].record()
        pos = ops.mesh_cluster_quadrics(verts, faces32, cluster.to(torch.int32), corners, seg, centre.contiguous(), cell,
                                        eps, clamp)
        ev[2].record()
        faces, _, cancelled = _cluster_faces(mesh.faces, cluster)
        used = torch.zeros(C, dtype=torch.bool, device=dev)
        used[faces.reshape(-1)] = True
        new_index = torch.cumsum(used, 0) - 1
        faces = new_index[faces]
        pos = pos[used]
        ev[3].record()
        torch.cuda.synchronize(dev)
    t = [ev[i].elapsed_time(ev[i + 1]) / 1e3 for i in range(3)]
    meta = dict(mesh.meta)
    meta['simplify'] = dict(cell=cell, clusters=C, verts_in=V, faces_in=F, verts=int(pos.shape[0]), faces=int(faces.shape[0]),
                            cancelled_sets=cancelled, simplify_s=sum(t), cluster_s=t[0], kernel_s=t[1], faces_s=t[2])
    return Mesh(pos, faces, meta=meta)


def project_to_level_set(value_and_gradient, verts, level=0.0, max_move=math.inf, steps=2):
    """verts [N,3] moved onto the level set `level` of a field by `steps` Newton steps along its gradient, x <- x - (f -
    level) g / max(|g|^2, 1e-12); after each step the displacement from the START is clamped per component to +-max_move.
    value_and_gradient(x [N,3]) -> (f [N] or [N,1], g [N,3]); for a network: lambda x: net.value_feature_gradient(x)[::2].
    The steps are taken in fp64 and rounded to verts' dtype; under no_grad; works on any device."""
    max_move = float(max_move)
    if not max_move >= 0.0:
        raise ValueError('max_move must not be negative, got %r' % (max_move,))
    with torch.no_grad():
        start = verts.detach().double()
        x = verts.detach()
        for _ in range(int(steps)):
            f, g = value_and_gradient(x)
            f, g = f.detach().double().reshape(-1, 1), g.detach().double()
            moved = x.double() - (f - float(level)) * g / (g * g).sum(1, keepdim=True).clamp_min(1e-12)
            x = (start + (moved - start).clamp(-max_move, max_move)).to(verts.dtype)
    return x


def _parse_simplify(simplify):
    simplify = float(simplify)
    if simplify != 0.0 and not 1.0 < simplify < math.inf:
        raise ValueError('simplify must be 0 (off) or a cell size above 1 grid spacing, got %r' % (simplify,))
    return simplify


# ---- the aligned grid of get_surface_high_res_mesh (plots.py:194-204, get_grid :257-288) -----------------------------
@dataclass
class AlignedGrid(Grid):
    mean: np.ndarray                             # [3] float64, the frame's origin in world space
    vecs: np.ndarray                             # [3,3] float64, rows = the frame's axes: local = vecs @ (p - mean)
    axes: list                                   # three float64 arrays: the grid points along the local x, y, z
    spacing: float                               # the step of all three axes
    shortest_axis: int

    def __post_init__(self):
        self.shape, self.origin = tuple(len(a) for a in self.axes), tuple(float(a[0]) for a in self.axes)

    def to_local(self, p):
        """[N,3] world -> [N,3] float64 local"""
        p = p.double()
        return (p - torch.as_tensor(self.mean, device=p.device)) @ torch.as_tensor(self.vecs, device=p.device).T

    def to_world(self, local_verts):
        """[N,3] local -> [N,3] float64 world: vecs^T local + mean"""
        q = local_verts.double()
        return q @ torch.as_tensor(self.vecs, device=q.device) + torch.as_tensor(self.mean, device=q.device)

    def points_at(self, idx, device=None):
        """[N,3] float32: the world-space grid points of the linear indices idx [N] (int64, any order); fp64 arithmetic,
        rounded once"""
        device = idx.device if device is None else device
        return self.to_world(self._gather([torch.as_tensor(a, device=device) for a in self.axes], idx)).float()

    def frame(self):
        """(p0, steps) for ops.classify_bricks: the world position of grid point (0, 0, 0) and the world steps of one index
        along the local x, y, z (fp64 lists)"""
        p0 = self.mean + self.vecs.T @ np.array(self.origin, np.float64)
        return p0.tolist(), [(self.spacing * self.vecs[a]).tolist() for a in range(3)]


def grid_axes(lo, hi, resolution, margin):
    """get_grid (plots.py:257-288) in its own expressions: the axis of the shortest extent has `resolution` points from
    min - margin to max + margin, the others the same step.  lo, hi: [3] float64 arrays -> (axes, step, shortest axis)"""
    shortest = int(np.argmin(hi - lo))
    s = np.linspace(lo[shortest] - margin, hi[shortest] + margin, resolution)
    length = np.max(s) - np.min(s)
    step = length / (s.shape[0] - 1)
    axes = [s if a == shortest else np.arange(lo[a] - margin, hi[a] + step + margin, step) for a in range(3)]
    return axes, float(step), shortest


def aligned_grid(points, resolution, margin=0.2, max_points=None):
    """The PCA-aligned grid around points [N,3]: the frame of plots.py:194-204 and the grid of get_grid.  Mean and 3 x 3
    scatter in fp64; torch.linalg.eigh on the host; the rows of vecs are the eigenvectors in ascending eigenvalue order,
    each signed so that its entry of the largest magnitude is positive, then row 0 negated if det < 0 (a proper rotation,
    and a deterministic one).  The reference fits the frame to 10 000 random surface samples; here the caller passes all
    vertices of the kept component, whose box contains the box of any sample.  ValueError, before anything is allocated,
    for a grid of more than ops.MCUBES_MAX_POINTS points (max_points, for a caller that does not hold the grid densely:
    extract_mesh(sparse=True) passes math.inf and leaves the limits to ops.brick_dims)."""
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
    if grid.numel() > (ops.MCUBES_MAX_POINTS if max_points is None else max_points):
        raise ValueError('aligned grid %d x %d x %d = %d points: marching_cubes needs fewer than 2^31'
                         % (grid.shape + (grid.numel(),)))
    return grid


# ---- sparse export: only the bricks the SDF interval grid cannot rule out (DESIGN.md 6f "Sparse export") ----------------
SPARSE_PROBE_ONE_IN = 64                         # skipped bricks probed at their centre: about one in 64 ...
SPARSE_PROBE_CAP = 65536                         # ... and at most this many


class _IntervalAudit:
    """Holds evaluated values against the interval of the interval-grid cell that contains their point: the cell of
    (int)((x + radius) * (float)(G / (2 radius))) per axis, as the tracer looks it up; points outside the cube have no
    interval.  Accumulates on the GPU; read() synchronises once."""

    def __init__(self, cells, radius):
        self.G = cells.shape[0]
        self.lo_hi = cells.view(torch.float16).view(-1, 2)             # little-endian halves of a word: lo, hi
        self.radius = torch.tensor(float(radius), device=cells.device, dtype=torch.float32)
        self.inv_h = torch.tensor(self.G / (2.0 * float(radius)), device=cells.device, dtype=torch.float32)
        self.violations = torch.zeros((), device=cells.device, dtype=torch.int64)
        self.excess = torch.zeros((), device=cells.device, dtype=torch.float32)

    def hold(self, x, v):
        if x.shape[0] == 0:
            return
        f = (x + self.radius) * self.inv_h
        inside = ((f >= 0.0) & (f < float(self.G))).all(1)
        c = f.long().clamp_(0, self.G - 1)
        b = self.lo_hi[(c[:, 0] * self.G + c[:, 1]) * self.G + c[:, 2]].float()
        over = torch.maximum(b[:, 0] - v, v - b[:, 1])
        over = torch.where(inside & (over > 0.0), over, torch.zeros_like(over))
        self.violations += (over > 0.0).sum()
        self.excess = torch.maximum(self.excess, over.max())

    def read(self):
        return int(self.violations), float(self.excess)


def _probe_indices(active, shape, brick):
    """linear grid indices of the centre points of about one in SPARSE_PROBE_ONE_IN skipped bricks (a hash of the brick
    index picks them), at most SPARSE_PROBE_CAP - beyond the cap the picks are thinned evenly, so that the probes still span
    the whole grid"""
    skipped = (active == 0).reshape(-1).nonzero()[:, 0]
    h = (skipped * 2654435761 + 40503) >> 9
    skipped = skipped[h % SPARSE_PROBE_ONE_IN == 0]
    n = skipped.shape[0]
    if n > SPARSE_PROBE_CAP:
        skipped = skipped[torch.arange(SPARSE_PROBE_CAP, device=skipped.device, dtype=torch.int64) * n // SPARSE_PROBE_CAP]
    by, bz = active.shape[1], active.shape[2]
    half = brick // 2
    i = ((skipped // (by * bz)) * brick + half).clamp_(max=shape[0] - 1)
    j = (((skipped // bz) % by) * brick + half).clamp_(max=shape[1] - 1)
    k = ((skipped % bz) * brick + half).clamp_(max=shape[2] - 1)
    return (i * shape[1] + j) * shape[2] + k


def _dense_mesh(net, precision, level, grid, chunk):
    """(verts, faces, the event between evaluation and meshing) of one grid held densely; verts in the grid's local frame"""
    vol = sdf_on_grid(net, grid, chunk=chunk, precision=precision)
    mid = torch.cuda.Event(enable_timing=True)
    mid.record()
    return marching_cubes(vol, level, spacing=(grid.spacing,) * 3, origin=grid.origin) + (mid,)


def _sparse_mesh(net, precision, radius, level, grid, brick, chunk):
    """_dense_mesh's triple and meta['sparse'] of one grid, through the SDF interval grid of `net` where there is one; where
    there is none, or it fails its audit, through _dense_mesh where the grid fits it; ValueError where neither path can run."""
    import warnings
    shape = grid.shape
    cb, _ = ops.brick_dims(shape, brick)
    n_points = shape[0] * shape[1] * shape[2]
    meta = dict(brick=int(brick), bricks=cb[0] * cb[1] * cb[2], active_bricks=None, evaluated_points=None,
                dense_points=n_points, audit_violations=0, probes=0, fallback=None)
    dense_fits = n_points <= ops.MCUBES_MAX_POINTS

    def densely(**why):
        meta.update(active_bricks=meta['bricks'], evaluated_points=n_points, **why)
        return _dense_mesh(net, precision, level, grid, chunk) + (meta,)

    def fall_back(reason, why):
        if not dense_fits:
            raise ValueError('sparse export of %d x %d x %d points needs the SDF interval grid, and %s; the dense path takes '
                             'fewer than 2^31 points' % (shape + (why,)))
        return densely(fallback=reason)

    if not precision.startswith('f16x3'):
        return fall_back('precision', 'its intervals bound the split evaluator only (precision %s)' % precision)
    cells = net.bound_grid(radius=radius)
    if cells is None:
        return fall_back('no_grid', 'this network has none (no coarse pass, or an audit dropped it)')
    pm = net.packed(f16x3=True)
    active = ops.classify_bricks(cells, radius, (shape,) + tuple(grid.frame()), level, brick)
    audit = _IntervalAudit(cells, radius)

    def sample(idx):
        x = grid.points_at(idx)
        v = ops.sdf_eval(pm, x)
        audit.hold(x, v)
        return v

    def run(active):
        stats = {}
        verts, faces = ops.marching_cubes_sparse(sample, shape, active, level, grid.origin, (grid.spacing,) * 3, brick, chunk,
                                                 stats)
        mid = stats.pop('eval_done', None)
        if mid is None:
            mid = torch.cuda.Event(enable_timing=True)
            mid.record()
        meta.update(active_bricks=stats['active_bricks'], evaluated_points=stats['evaluated_points'])
        return verts, faces, mid

    out = run(active)
    probes = _probe_indices(active, shape, int(brick))
    meta['probes'] = int(probes.shape[0])
    for s in range(0, probes.shape[0], chunk):
        sample(probes[s:s + chunk])
    violations, excess = audit.read()
    if violations:
        # the intervals are measured bounds: one that fails may have hidden a crossing - nothing of this mesh is kept
        meta.update(audit_violations=violations, fallback='audit')
        warnings.warn('sparse mesh export: %d evaluated values lie outside the SDF interval grid by up to %.3e; the grid is '
                      'dropped and the export repeated without it' % (violations, excess))
        net.note_lipschitz_audit(excess, net.minsdf_lipschitz(radius))
        del out
        if dense_fits:
            return densely()
        audit.hold = lambda x, v: None
        out = run(torch.ones_like(active))
    return out + (meta,)


def _aligned_final_grid(net, precision, level, bound, chunk, low_resolution, resolution, margin, max_points):
    """(grid, extra) of extract_mesh(high_res=True): the uniform grid meshed densely at low_resolution, its largest component
    kept, and the AlignedGrid around that component's vertices; extra: the pass's entries of meta"""
    lv, lf, _ = _dense_mesh(net, precision, level, uniform_grid(low_resolution, bound), chunk)
    if lv.shape[0] == 0:
        raise ValueError('no surface at level %g inside [-%g, %g]^3 at the low resolution %d'
                         % (level, bound, bound, low_resolution))
    low_mesh = select_components(Mesh(lv, lf, meta=dict(cc_rounds=0, cc_s=0.0)), 'largest')
    extra = dict(cc_rounds=low_mesh.meta['cc_rounds'], cc_s=low_mesh.meta['cc_s'],
                 low_res_components=low_mesh.meta['components'])
    return aligned_grid(low_mesh.verts, resolution, margin, max_points=max_points), extra


def _finish_mesh(model, mesh, level, sp, materials, keep, simplify, project):
    """extract_mesh's tail on the world-space mesh of a grid of spacing sp: keep, simplify and project, then normals and
    materials at the final vertices"""
    net = _implicit(model)
    if keep != 'all' and mesh.verts.shape[0]:
        mesh = select_components(mesh, keep)
    if simplify > 0.0 and mesh.verts.shape[0]:
        mesh = simplify_mesh(mesh, simplify * sp)
        if 'simplify' in mesh.meta:                  # not there for a mesh without faces, which comes back as it is
            if project and mesh.verts.shape[0]:
                mesh.verts = project_to_level_set(lambda x: net.value_feature_gradient(x)[::2], mesh.verts, level,
                                                  max_move=0.5 * simplify * sp)
            mesh.meta['simplify']['project'] = bool(project)
    V = mesh.verts.shape[0]
    if V:
        _, feat, g = net.value_feature_gradient(mesh.verts)
        mesh.normals = g / g.norm(dim=1, keepdim=True).clamp_min(1e-12)
        mat_net = getattr(model, 'envmap_material_network', None)
        if materials and mat_net is not None:
            out = mat_net(mesh.verts, feat)
            mesh.diffuse_albedo = out['sg_diffuse_albedo'].float().reshape(V, 3).contiguous()
            mesh.roughness = out['sg_roughness'].float().expand(V, 1).contiguous()
            spec = mat_net.specular_inv_remap(out['sg_specular_reflectance']).float()
            mesh.specular_reflection = spec.expand(V, 3).contiguous()
    return mesh


def extract_mesh(model, resolution=512, level=0.0, bound=None, materials=True, chunk=2 ** 24, keep='all', high_res=False,
                 low_resolution=100, margin=0.2, simplify=0.0, project=True, sparse=False, brick=8):
    """Mesh of the level set `level` of the SDF of `model` (an IDRNetwork or a bare ImplicitNetwork) on
    linspace(-bound, bound, resolution)^3; bound defaults to model.object_bounding_sphere.  Normals: the normalised SDF
    gradient at the vertices.  With an IDRNetwork and materials=True, also diffuse_albedo / roughness from
    envmap_material_network(verts, feats) and specular_reflection as render.py writes it (global parameters broadcast).

    high_res (plots.get_surface_high_res_mesh): the uniform grid is meshed at low_resolution, its largest component kept,
    and the surface re-meshed on aligned_grid(that component's vertices, resolution, margin) - `resolution` points along
    the component's shortest axis; ValueError when the low-resolution grid has no crossing.  keep ('all', 'largest' or a
    fraction, see select_components) applies to the final mesh before normals and materials are computed.  With the
    defaults the path and the output are those of the uniform grid alone.

    simplify: 0 - off; else the edge of the clustering cells in units of the final grid's spacing (above 1: a cell of one
    spacing or less merges next to nothing), applied after `keep` through simplify_mesh; with project the new vertices are
    then moved onto the level set of the model's own SDF (project_to_level_set, at most half a cell per component).  Normals
    and materials are evaluated at the final vertices, never interpolated.  meta gains 'simplify' (simplify_mesh's record,
    plus project) only then - and not for a mesh without faces, which simplify_mesh hands back untouched.  Cells so large
    that no face survives give a mesh of 0 vertices whose meta['simplify'] says what went in.

    sparse (DESIGN.md 6f "Sparse export"; off: no path and no output changes): the final grid - the uniform one, or the
    aligned one under high_res, whose low-resolution pass stays dense - is cut into bricks of `brick` cells; the SDF interval
    grid of the network (net.bound_grid(model.object_bounding_sphere), the split evaluator's bounds) rules bricks out, and only
    the others, dilated by one brick, are evaluated - every point once, by the dense path's expressions - and meshed
    (ops.marching_cubes_sparse): the same vertices and faces, and grids the dense path cannot hold (up to 4096 points per
    axis).  The intervals are measured bounds, so every evaluated point inside the cube is held against its cell's interval
    and about 1 in 64 skipped bricks is probed at its centre; a violation warns, drops the grid (note_lipschitz_audit) and
    repeats the export densely, or with every brick active where the dense path cannot hold the grid.  Without a grid (no
    coarse pass, dropped by an audit) or under a precision other than f16x3* the dense path runs, where the grid fits it.
    meta['sparse'] = brick, bricks, active_bricks, evaluated_points, dense_points, audit_violations, probes, fallback (None,
    'no_grid', 'precision' or 'audit').  ValueError, before anything is allocated, for an axis of more than 4096 points and
    for a grid neither path can take."""
    keep = _parse_keep(keep)
    simplify = _parse_simplify(simplify)
    sparse = bool(sparse)
    if sparse:                                           # under high_res the final shape is not known yet: the brick alone
        ops.brick_dims((2, 2, 2) if high_res else (int(resolution),) * 3, brick)
    net = _implicit(model)
    if bound is None:
        if not hasattr(model, 'object_bounding_sphere'):
            raise ValueError('a bare ImplicitNetwork needs an explicit bound')
        bound = model.object_bounding_sphere
    bound = float(bound)
    dev = next(net.parameters()).device
    if dev.type != 'cuda':
        raise ValueError('extract_mesh needs a model on the GPU (the hot path has no CPU fallback)')
    precision = _tracer_precision(model)
    with torch.no_grad():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        max_points = math.inf if sparse else None
        if high_res:
            grid, extra = _aligned_final_grid(net, precision, level, bound, chunk, low_resolution, resolution, margin, max_points)
        else:
            grid, extra = uniform_grid(resolution, bound, max_points), dict(cc_rounds=0, cc_s=0.0)
        if sparse:
            verts, faces, ev[1], extra['sparse'] = _sparse_mesh(
                net, precision, float(getattr(model, 'object_bounding_sphere', bound)), level, grid, brick, chunk)
        else:
            verts, faces, ev[1] = _dense_mesh(net, precision, level, grid, chunk)
        ev[2].record()
        mesh = _finish_mesh(model, Mesh(grid.to_world(verts).float(), faces, meta=extra), level, grid.spacing, materials, keep,
                            simplify, project)
        torch.cuda.synchronize(dev)
    mesh.meta = dict(resolution=int(resolution), level=float(level), bound=bound, grid_shape=tuple(grid.shape),
                     spacing=float(grid.spacing), grid_s=ev[0].elapsed_time(ev[1]) / 1e3,
                     mcubes_s=ev[1].elapsed_time(ev[2]) / 1e3, **mesh.meta)
    return mesh
