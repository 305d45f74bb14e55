"""Mesh kernels: marching cubes, BVH distance and winding-number queries, connected components, quadric vertex clustering, texture baking."""
import ctypes
import math

import torch

from .. import _lib
from ._call import _ptr, call, check_tensor, need_gpu
from .envlight import _envlight_coord, _envlight_map, _envlight_table


# ---- marching cubes (utils/plots.py get_surface_trace: skimage marching_cubes_lewiner) -----------------
MCUBES_MAX_POINTS = (1 << 31) - 1           # nx * ny * nz must stay below 2^31 (int32 grid-point indices)


def _placement(level, origin, spacing):
    """(level, origin, spacing) as a float and two lists of 3 floats; ValueError unless all are finite"""
    level, origin, spacing = float(level), [float(v) for v in origin], [float(v) for v in spacing]
    if len(origin) != 3 or len(spacing) != 3 or not all(math.isfinite(v) for v in origin + spacing + [level]):
        raise ValueError('level, origin and spacing must be finite, origin and spacing 3 values each')
    return level, origin, spacing


def marching_cubes(volume, level, origin, spacing):
    """(verts [V,3] float32, faces [F,3] int32) of the level set of volume [nx, ny, nz] (float32, contiguous, on the GPU;
    inside: v < level), vertices at origin + index * spacing.  Counts, reads the two counts back (the one host
    synchronisation), then emits into buffers of exactly that size."""
    if volume.dim() != 3 or min(volume.shape) < 2:
        raise ValueError('volume must be [nx, ny, nz] with every dim >= 2, got %s' % (tuple(volume.shape),))
    if volume.numel() > MCUBES_MAX_POINTS:
        raise ValueError('volume of %d points: marching_cubes needs fewer than 2^31' % volume.numel())
    need_gpu(volume)
    if volume.dtype != torch.float32 or not volume.is_contiguous():
        raise RuntimeError('marching_cubes needs a contiguous float32 volume, got %s' % (volume.dtype,))
    level, origin, spacing = _placement(level, origin, spacing)
    lib = _lib.lib()
    nx, ny, nz = volume.shape
    dev = volume.device
    ws = torch.empty(lib.nefii_mcubes_workspace_bytes(nx, ny, nz), device=dev, dtype=torch.uint8)
    counts = torch.empty(2, device=dev, dtype=torch.int64)
    call('nefii_mcubes_count', _ptr(volume), nx, ny, nz, level, _ptr(ws), _ptr(counts))
    n_verts, n_tris = counts.tolist()
    if n_verts >= 1 << 31:
        raise ValueError('%d vertices: int32 face indices cannot address them' % n_verts)
    verts = torch.empty(n_verts, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(n_tris, 3, device=dev, dtype=torch.int32)
    if n_verts and n_tris:
        call('nefii_mcubes_emit', _ptr(volume), nx, ny, nz, level, *origin, *spacing, _ptr(ws), _ptr(verts), n_verts,
             _ptr(faces), n_tris)
    return verts, faces


# ---- sparse marching cubes over the bricks an SDF interval grid cannot rule out (DESIGN.md 6f "Sparse export") ----------
MCUBES_SPARSE_MAX_AXIS = 4096               # grid points per axis (include/nefii_amd.h)
MCUBES_SPARSE_MAX_BRICK = 8


def brick_dims(shape, brick=8):
    """(cell bricks per axis, point bricks per axis) of a fine grid of `shape` points cut into bricks of `brick` cells:
    ceil((n - 1) / brick) bricks of cells, (n - 1) // brick + 1 bricks of owned points.  ValueError, before anything is
    allocated, for an axis outside 2 .. 4096, a brick outside 2 .. 8 and 2^31 bricks or more."""
    shape, brick = tuple(int(n) for n in shape), int(brick)
    if len(shape) != 3 or min(shape) < 2:
        raise ValueError('shape must be (nx, ny, nz) with every dim >= 2, got %s' % (shape,))
    if max(shape) > MCUBES_SPARSE_MAX_AXIS:
        raise ValueError('grid of %d x %d x %d points: sparse marching cubes takes at most %d per axis'
                         % (shape + (MCUBES_SPARSE_MAX_AXIS,)))
    if not 2 <= brick <= MCUBES_SPARSE_MAX_BRICK:
        raise ValueError('brick must lie in 2 .. %d cells, got %d' % (MCUBES_SPARSE_MAX_BRICK, brick))
    cb = tuple((n - 2) // brick + 1 for n in shape)
    pb = tuple((n - 1) // brick + 1 for n in shape)
    if cb[0] * cb[1] * cb[2] >= 1 << 31:
        raise ValueError('%d x %d x %d bricks: fewer than 2^31 are needed, use a larger brick' % cb)
    return cb, pb


def classify_bricks(cells, radius, grid, level, brick=8):
    """active [bx, by, bz] uint8: 1 where a brick of the fine grid may hold a crossing of `level` according to the SDF interval
    grid cells [G, G, G] int32 over [-radius, radius]^3 (build_bound_grid), 0 where the intervals of every cell the brick's
    box overlaps exclude the level (nefii_mcubes_classify_bricks; include/nefii_amd.h states the rule).  grid = (shape, p0,
    steps): the fine grid's (nx, ny, nz), the world position of its point (0, 0, 0) and the three world steps of one index
    along x, y, z - axis-aligned for a uniform grid, rotated for an AlignedGrid.  A brick outside the cube is active."""
    shape, p0, steps = grid
    cb, _ = brick_dims(shape, brick)
    need_gpu(cells)
    check_tensor('cells', cells, torch.int32, (None, None, None))
    G = cells.shape[0]
    if cells.shape != (G, G, G):
        raise ValueError('cells must be [G, G, G], got %s' % (tuple(cells.shape),))
    frame = [float(v) for v in p0] + [float(v) for s in steps for v in s]
    radius, level = float(radius), float(level)
    if len(frame) != 12 or not all(math.isfinite(v) for v in frame + [radius, level]) or not radius > 0.0:
        raise ValueError('p0 and the three steps must be 3 finite values each, level finite, radius positive and finite')
    out = torch.empty(cb, device=cells.device, dtype=torch.uint8)
    call('nefii_mcubes_classify_bricks', _ptr(cells), G, radius, *[int(n) for n in shape], (ctypes.c_double * 12)(*frame),
         level, int(brick), _ptr(out))
    return out


def dilate_bricks(active, shape, brick=8):
    """evaluated [pbx, pby, pbz] bool: the point bricks that the cell bricks of `active` touch - the brick itself and its 7
    upper neighbours, whose owned points are the far corners of its last layer of cells"""
    cb, pb = brick_dims(shape, brick)
    if tuple(active.shape) != cb:
        raise ValueError('active must be %s for a grid of %s points in bricks of %d, got %s'
                         % (cb, tuple(shape), brick, tuple(active.shape)))
    a = torch.zeros(pb, device=active.device, dtype=torch.bool)
    a[:cb[0], :cb[1], :cb[2]] = active != 0
    ev = a.clone()
    for d in range(1, 8):
        dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
        ev[dx:, dy:, dz:] |= a[:pb[0] - dx, :pb[1] - dy, :pb[2] - dz]
    return ev


def _eval_bricks(sample, shape, pb, eb, B, chunk, stats):
    """(vals [n_slots, B^3] float32, finite): sample() on every grid point the point bricks eb [n_slots] own, each point
    once, in chunks of about `chunk`; +inf where a brick runs past the grid.  finite: a GPU flag, all samples were finite -
    left unread here.  stats gains evaluated_points and eval_done."""
    nx, ny, nz = shape
    dev = eb.device
    n_slots = eb.shape[0]
    vals = torch.empty(n_slots, B ** 3, device=dev, dtype=torch.float32)
    loc = torch.arange(B, device=dev, dtype=torch.int64)
    finite = torch.ones((), device=dev, dtype=torch.bool)
    per = max(1, int(chunk) // B ** 3)
    evaluated = 0
    for s in range(0, n_slots, per):
        b = eb[s:s + per]
        gx = (b // (pb[1] * pb[2]))[:, None] * B + loc
        gy = ((b // pb[2]) % pb[1])[:, None] * B + loc
        gz = (b % pb[2])[:, None] * B + loc
        lin = ((gx[:, :, None, None] * ny + gy[:, None, :, None]) * nz + gz[:, None, None, :]).reshape(-1)
        inside = ((gx < nx)[:, :, None, None] & (gy < ny)[:, None, :, None] & (gz < nz)[:, None, None, :]).reshape(-1)
        idx = lin[inside]
        v = sample(idx)
        if v.shape != idx.shape:
            raise ValueError('sample must return one value per index, got %s for %d' % (tuple(v.shape), idx.shape[0]))
        v = v.to(torch.float32)
        finite &= torch.isfinite(v).all()
        out = vals[s:s + per].view(-1)
        out.fill_(math.inf)
        out[inside] = v
        evaluated += idx.shape[0]
    if stats is not None:
        stats['evaluated_points'] = evaluated
        stats['eval_done'] = torch.cuda.Event(enable_timing=True)      # where the evaluation ends and the meshing starts
        stats['eval_done'].record()
    return vals, finite


def _sparse_launches(vals, slot_map, shape, B, alist, level, origin, spacing, finite):
    """(vkeys [n], vpos [n,3], fcell [m], fkeys [m,3]) of the active bricks alist, shared edges twice, or None where nothing
    crosses: count, one read-back (the counts, and with them the flag of _eval_bricks), emit into buffers of that size"""
    dev = vals.device
    n_slots, n_active = vals.shape[0], alist.shape[0]
    counts = torch.empty(n_active, 2, device=dev, dtype=torch.int32)
    call('nefii_mcubes_sparse_count', _ptr(vals), _ptr(slot_map), n_slots, *shape, B, _ptr(alist), n_active, level, _ptr(counts))
    ends = torch.cumsum(counts.long(), 0)
    n_verts, n_tris = ends[-1].tolist()
    if not bool(finite):
        raise ValueError('sample returned non-finite values')
    if n_verts >= 1 << 31 or n_tris >= 1 << 31:
        raise ValueError('%d vertices, %d faces: both must stay below 2^31' % (n_verts, n_tris))
    if n_verts == 0 or n_tris == 0:
        return None
    offsets = (ends - counts).contiguous()
    vkeys = torch.empty(n_verts, device=dev, dtype=torch.int64)
    vpos = torch.empty(n_verts, 3, device=dev, dtype=torch.float32)
    fcell = torch.empty(n_tris, device=dev, dtype=torch.int64)
    fkeys = torch.empty(n_tris, 3, device=dev, dtype=torch.int64)
    call('nefii_mcubes_sparse_emit', _ptr(vals), _ptr(slot_map), n_slots, *shape, B, _ptr(alist), n_active, level, *origin,
         *spacing, _ptr(offsets), _ptr(vkeys), _ptr(vpos), n_verts, _ptr(fcell), _ptr(fkeys), n_tris)
    return vkeys, vpos, fcell, fkeys


def _weld(vkeys, vpos, fcell, fkeys):
    # an edge on a face two active bricks share comes twice, bit-equal: keep one; the keys' order is the dense order
    vkeys, order = torch.sort(vkeys)
    first = torch.ones_like(vkeys, dtype=torch.bool)
    first[1:] = vkeys[1:] != vkeys[:-1]
    vkeys = vkeys[first]
    verts = vpos[order[first]]
    forder = torch.sort(fcell, stable=True)[1]
    faces = torch.searchsorted(vkeys, fkeys[forder].reshape(-1)).view(-1, 3)
    return verts, faces


def marching_cubes_sparse(sample, shape, active, level, origin, spacing, brick=8, chunk=2 ** 24, stats=None):
    """(verts [V,3] float32, faces [F,3] int64) of the level set over the cell bricks marked in active [bx, by, bz] (uint8 or
    bool, on the GPU) of a grid of `shape` points that is never held densely.  sample(idx): float32 values at an int64
    tensor of linear grid indices ((i * ny + j) * nz + k); it is called on chunks of about `chunk` points, and on every point
    of the evaluated bricks (dilate_bricks) exactly once - two evaluations of one point that differed in a bit would cut a
    shared face two ways.  Given the same values and an active set that covers every crossing cell, verts and faces are
    bitwise those of marching_cubes on the dense volume, in its order: the kernels emit 64-bit keys (owner * 3 + axis per
    vertex; cell and vertex keys per triangle), torch.sort / searchsorted give the order and the indices.  The grid may
    exceed 2^31 points; V and F stay below 2^31.  stats (a dict) gains bricks, active_bricks, evaluated_points and, when
    anything was evaluated, eval_done: a HIP event recorded between the evaluation and the meshing.
    ValueError, before anything is allocated, for shapes and bricks brick_dims refuses; and for non-finite samples."""
    cb, pb = brick_dims(shape, brick)
    shape, B = tuple(int(n) for n in shape), int(brick)
    level, origin, spacing = _placement(level, origin, spacing)
    need_gpu(active)
    dev = active.device
    ev = dilate_bricks(active, shape, B)
    alist = (active != 0).reshape(-1).nonzero()[:, 0].to(torch.int32)
    if stats is not None:
        stats.update(bricks=cb[0] * cb[1] * cb[2], active_bricks=alist.shape[0], evaluated_points=0)
    empty = (torch.empty(0, 3, device=dev, dtype=torch.float32), torch.empty(0, 3, device=dev, dtype=torch.int64))
    if alist.shape[0] == 0:
        return empty
    eb = ev.reshape(-1).nonzero()[:, 0]
    slot_map = torch.full((pb[0] * pb[1] * pb[2],), -1, device=dev, dtype=torch.int32)
    slot_map[eb] = torch.arange(eb.shape[0], device=dev, dtype=torch.int32)
    vals, finite = _eval_bricks(sample, shape, pb, eb, B, chunk, stats)
    emitted = _sparse_launches(vals, slot_map, shape, B, alist, level, origin, spacing, finite)
    del vals
    return empty if emitted is None else _weld(*emitted)


def mesh_sdf_query(node_box, n_leaves, tris, leaf_size, points, want_sign=True):
    """Exact distance from points [P, 3] to the mesh behind a mesh_bvh.MeshBVH (nefii_mesh_sdf_query): node_box
    [2 n_leaves - 1, 6], tris [F, 9] in tree order and points, all contiguous float64 on the GPU and in the tree's frame ->
    [P] float64, negative inside the (closed) mesh when want_sign, unsigned otherwise.  No gradient."""
    for name, t, cols in (('node_box', node_box, 6), ('tris', tris, 9), ('points', points, 3)):
        check_tensor(name, t, torch.float64, (None, cols))
    need_gpu(node_box, tris, points)
    if node_box.shape[0] != 2 * int(n_leaves) - 1:
        raise ValueError('node_box must hold 2 n_leaves - 1 = %d boxes, got %d' % (2 * int(n_leaves) - 1, node_box.shape[0]))
    out = torch.empty(points.shape[0], dtype=torch.float64, device=points.device)
    if points.shape[0] == 0:
        return out
    call('nefii_mesh_sdf_query', _ptr(node_box), int(n_leaves), _ptr(tris), tris.shape[0], int(leaf_size), _ptr(points),
         points.shape[0], 1 if want_sign else 0, _ptr(out))
    return out


def check_winding_beta(beta):
    """float(beta); ValueError unless it is 0 (exact) or >= 1: the dipole expansion means nothing inside a node's sphere"""
    beta = float(beta)
    if not (beta == 0.0 or beta >= 1.0):
        raise ValueError('beta must be 0 (no approximation) or >= 1, got %r' % (beta,))
    return beta


def mesh_winding_query(node_box, node_moment, n_leaves, tris, leaf_size, points, beta):
    """Generalized winding number of points [P, 3] about the mesh behind a mesh_bvh.MeshBVH (nefii_mesh_winding_query,
    DESIGN.md 6s): node_box [2 n_leaves - 1, 6], node_moment [2 n_leaves - 1, 8] (mesh_bvh.build_moments), tris [F, 9] in tree
    order and points, all contiguous float64 on the GPU and in the tree's frame -> [P] float64: 1 inside a closed, outward-
    oriented mesh, 0 outside.  beta = 0: the exact sum over all faces; beta >= 1: a node farther than beta times its radius
    is taken as one dipole.  No gradient."""
    for name, t, cols in (('node_box', node_box, 6), ('node_moment', node_moment, 8), ('tris', tris, 9), ('points', points, 3)):
        check_tensor(name, t, torch.float64, (None, cols))
    beta = check_winding_beta(beta)
    need_gpu(node_box, node_moment, tris, points)
    rows = 2 * int(n_leaves) - 1
    if node_box.shape[0] != rows or node_moment.shape[0] != rows:
        raise ValueError('node_box and node_moment must hold 2 n_leaves - 1 = %d rows, got %d and %d'
                         % (rows, node_box.shape[0], node_moment.shape[0]))
    out = torch.empty(points.shape[0], dtype=torch.float64, device=points.device)
    if points.shape[0] == 0:
        return out
    call('nefii_mesh_winding_query', _ptr(node_box), _ptr(node_moment), int(n_leaves), _ptr(tris), tris.shape[0],
         int(leaf_size), _ptr(points), points.shape[0], beta, _ptr(out))
    return out


# ---- connected components of a mesh (utils/plots.py:186-189, trimesh's split) ---------------------------
def mesh_cc_round_cap(n_verts):
    """rounds after which mesh_components gives up: 4 ceil(log2(max(V, 2))) + 8 (measured: 4 to 11)"""
    return 4 * (max(int(n_verts), 2) - 1).bit_length() + 8


def mesh_components(faces, n_verts):
    """(label [V] int32, rounds): label[v] = the smallest vertex index of the edge-connected component of vertex v in the
    mesh faces [F,3] (contiguous int32 on the GPU) over n_verts vertices; a vertex in no face is its own component.  The
    same bits for any order of the faces and from run to run.  Duplicated faces and faces with repeated indices are legal.
    nefii_mesh_cc_init, then rounds of nefii_mesh_cc_round; the 8 bytes of flags are read back after every round and the
    loop ends when none changed anything - the one kind of host synchronisation here.  ValueError for a face index outside
    [0, n_verts) (such a face is never followed on the device), RuntimeError beyond mesh_cc_round_cap(n_verts) rounds."""
    need_gpu(faces)
    check_tensor('faces', faces, torch.int32, (None, 3))
    n_verts, n_faces = int(n_verts), faces.shape[0]
    if n_verts < 0 or n_verts >= 1 << 31 or n_faces >= 1 << 31:
        raise ValueError('n_verts = %d, %d faces: both must lie in 0 .. 2^31 - 1' % (n_verts, n_faces))
    dev = faces.device
    parent = torch.empty(n_verts, device=dev, dtype=torch.int32)
    if n_verts == 0:
        if n_faces:
            raise ValueError('%d faces over no vertices' % n_faces)
        return parent, 0
    flags = torch.empty(2, device=dev, dtype=torch.int32)
    call('nefii_mesh_cc_init', _ptr(parent), n_verts, _ptr(flags))
    if n_faces == 0:
        return parent, 0
    cap = mesh_cc_round_cap(n_verts)
    for rounds in range(1, cap + 1):
        call('nefii_mesh_cc_round', _ptr(faces), n_faces, _ptr(parent), n_verts, _ptr(flags))
        changed, bad = flags.tolist()
        if bad:
            raise ValueError('faces hold an index outside [0, %d)' % n_verts)
        if not changed:
            return parent, rounds
    raise RuntimeError('mesh_components: no fixpoint after %d rounds over %d vertices' % (cap, n_verts))


# ---- vertex clustering with quadric error metrics (Lindstrom 2000) --------------------------------------
def mesh_cluster_quadrics(verts, faces, cluster, corners, seg, centre, h, eps=1e-3, clamp=0.5):
    """pos [C,3] float32: the representative vertex of each of the C = centre.shape[0] clusters, the regularised minimiser of
    the cluster's quadric error (nefii_mesh_cluster_quadrics; include/nefii_amd.h states the arithmetic).  verts [V,3]
    float32, faces [F,3] int32, cluster [V] int32, corners [3F] int32 (the corners 3 face + k sorted stably by the cluster of
    their vertex), seg [C+1] int64 (the clusters' runs in corners), centre [C,3] float64, all contiguous and on the GPU; h,
    eps, clamp: host numbers.  The same bits from call to call.  The 8 bytes of flags are read back - the one host
    synchronisation here: ValueError for a face index outside [0, V), for a used vertex whose cluster is outside [0, C) and
    for a corner list that does not match the clustering (none of them is ever followed on the device)."""
    for name, t, dtype, shape in (('verts', verts, torch.float32, (None, 3)), ('faces', faces, torch.int32, (None, 3)),
                                  ('cluster', cluster, torch.int32, (None,)), ('corners', corners, torch.int32, (None,)),
                                  ('seg', seg, torch.int64, (None,)), ('centre', centre, torch.float64, (None, 3))):
        need_gpu(t)
        check_tensor(name, t, dtype, shape)
    V, F, C = verts.shape[0], faces.shape[0], centre.shape[0]
    if cluster.shape[0] != V or corners.shape[0] != 3 * F or seg.shape[0] != C + 1:
        raise ValueError('cluster must hold V = %d entries, corners 3 F = %d, seg C + 1 = %d; got %d, %d, %d'
                         % (V, 3 * F, C + 1, cluster.shape[0], corners.shape[0], seg.shape[0]))
    if V >= 1 << 31 or 3 * F >= 1 << 31 or C >= 1 << 31:
        raise ValueError('%d vertices, %d corners, %d clusters: all must stay below 2^31' % (V, 3 * F, C))
    h, eps, clamp = float(h), float(eps), float(clamp)
    if not (0.0 < h < math.inf) or not (0.0 <= eps < math.inf) or not (0.0 < clamp < math.inf):
        raise ValueError('h and clamp must be positive and finite, eps finite and not negative; got %r, %r, %r'
                         % (h, eps, clamp))
    pos = torch.empty(C, 3, device=verts.device, dtype=torch.float32)
    if C == 0:
        return pos
    if F == 0:
        raise ValueError('%d clusters over no faces' % C)
    flags = torch.empty(2, device=verts.device, dtype=torch.int32)
    call('nefii_mesh_cluster_quadrics', _ptr(verts), V, _ptr(faces), F, _ptr(cluster), _ptr(corners), _ptr(seg), _ptr(centre),
         C, h, eps, clamp, _ptr(pos), _ptr(flags))
    bad_index, bad_cluster = flags.tolist()
    if bad_index:
        raise ValueError('faces hold an index outside [0, %d)' % V)
    if bad_cluster:
        raise ValueError('a used vertex has a cluster outside [0, %d), or the corner list does not match the clustering' % C)
    return pos


# ---- texture baking over a per-face-chart atlas (include/nefii_amd.h states the atlas) --------------------
BAKE_MIN_SIZE, BAKE_MAX_SIZE = 7, 8192           # texels per side of the atlas
BAKE_MIN_PAD = 2                                 # below it a bilinear lookup inside a chart reads its neighbour's texels


def _atlas_numbers(size, cells_per_row, cell, pad):
    """(T, n, c, p) as ints; ValueError outside the limits of include/nefii_amd.h"""
    T, n, c, p = int(size), int(cells_per_row), int(cell), int(pad)
    if not BAKE_MIN_SIZE <= T <= BAKE_MAX_SIZE:
        raise ValueError('size must lie in %d .. %d, got %d' % (BAKE_MIN_SIZE, BAKE_MAX_SIZE, T))
    if p < BAKE_MIN_PAD:
        raise ValueError('pad must be >= %d, got %d' % (BAKE_MIN_PAD, p))
    if n < 1 or c < 1 or n * c > T or c - 3 * p < 1:
        raise ValueError('%d x %d cells of %d texels with pad %d do not make an atlas of %d texels' % (n, n, c, p, T))
    return T, n, c, p


def bake_raster(verts, faces, size, cells_per_row, cell, pad, first=0, count=None):
    """(owner [count] int32, covered [count] uint8, bary [count,2] float32, pos [count,3] float32) of the texels first ..
    first + count - 1 (linear index j T + i; count defaults to the rest of the image) of the per-face-chart atlas
    (nefii_bake_raster): the face that owns each texel or -1, whether the texel's centre lies inside the face's chart, the
    barycentric weights (b1, b2) of that centre (b0 = 1 - b1 - b2; gutter texels extrapolate) and the point b0 v0 + b1 v1 +
    b2 v2 of the face.  verts [V,3] float32, faces [F,3] int32, contiguous and on the GPU.  The 8 bytes of flags are read
    back - the one host synchronisation: ValueError for a face index outside [0, V) (never followed on the device) and for a
    position that is not finite."""
    need_gpu(verts, faces)
    check_tensor('verts', verts, torch.float32, (None, 3))
    check_tensor('faces', faces, torch.int32, (None, 3))
    T, n, c, p = _atlas_numbers(size, cells_per_row, cell, pad)
    V, F = verts.shape[0], faces.shape[0]
    if V >= 1 << 31 or 3 * F >= 1 << 31 or F > 2 * n * n:
        raise ValueError('%d vertices, %d faces: an atlas of %d x %d cells holds %d faces' % (V, F, n, n, 2 * n * n))
    first = int(first)
    count = T * T - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > T * T:
        raise ValueError('texels %d .. %d lie outside the image of %d' % (first, first + count - 1, T * T))
    dev = verts.device
    owner = torch.empty(count, device=dev, dtype=torch.int32)
    covered = torch.empty(count, device=dev, dtype=torch.uint8)
    bary = torch.empty(count, 2, device=dev, dtype=torch.float32)
    pos = torch.empty(count, 3, device=dev, dtype=torch.float32)
    flags = torch.empty(2, device=dev, dtype=torch.int32)
    call('nefii_bake_raster', _ptr(verts), V, _ptr(faces), F, T, n, c, p, first, count, _ptr(owner), _ptr(covered), _ptr(bary),
         _ptr(pos), _ptr(flags))
    bad_index, bad_pos = flags.tolist()
    if bad_index:
        raise ValueError('faces hold an index outside [0, %d)' % V)
    if bad_pos:
        raise ValueError('verts hold values that are not finite')
    return owner, covered, bary, pos


def bake_encode(albedo, roughness, normal, owner):
    """(rgba_albedo [N,4], rgba_normal [N,4], grey_roughness [N]) uint8 of N baked texels (nefii_bake_encode): albedo through
    the tone map of the PLY's vertex colours (clamp at 0, power 1 / 2.2, clamp to [0, 1]), the normal as 0.5 n + 0.5, the
    roughness clamped to [0, 1], each to floor(255 x + 0.5) in fp64; alpha 255 where owner >= 0, all bytes 0 elsewhere.
    albedo, normal [N,3], roughness [N] float32, owner [N] int32, contiguous and on the GPU."""
    need_gpu(albedo, roughness, normal, owner)
    N = owner.shape[0] if owner.dim() == 1 else -1
    check_tensor('owner', owner, torch.int32, (None,))
    check_tensor('albedo', albedo, torch.float32, (N, 3))
    check_tensor('roughness', roughness, torch.float32, (N,))
    check_tensor('normal', normal, torch.float32, (N, 3))
    if N > BAKE_MAX_SIZE ** 2:
        raise ValueError('%d texels: an atlas holds at most %d' % (N, BAKE_MAX_SIZE ** 2))
    dev = owner.device
    rgba_albedo = torch.empty(N, 4, device=dev, dtype=torch.uint8)
    rgba_normal = torch.empty(N, 4, device=dev, dtype=torch.uint8)
    grey = torch.empty(N, device=dev, dtype=torch.uint8)
    if N:
        call('nefii_bake_encode', _ptr(albedo), _ptr(roughness), _ptr(normal), _ptr(owner), N, _ptr(rgba_albedo),
             _ptr(rgba_normal), _ptr(grey))
    return rgba_albedo, rgba_normal, grey


def texture_sample(tex, face, bary, cells_per_row, cell, pad):
    """out [N,C] float32: the bilinear lookup of tex [T,T,C] (float32, C in 1 .. 4) at the atlas positions of face [N] int32
    and bary [N,3] float64 (nefii_texture_sample; fp64 arithmetic, texel indices clamped to the image).  A face below 0 or
    without a cell gives zeros.  All contiguous and on the GPU."""
    need_gpu(tex, face, bary)
    check_tensor('tex', tex, torch.float32, (None, None, None))
    T, C = tex.shape[0], tex.shape[2]
    if tex.shape[1] != T or not 1 <= C <= 4:
        raise ValueError('tex must be [T, T, C] with C in 1 .. 4, got %s' % (tuple(tex.shape),))
    T, n, c, p = _atlas_numbers(T, cells_per_row, cell, pad)
    check_tensor('face', face, torch.int32, (None,))
    N = face.shape[0]
    check_tensor('bary', bary, torch.float64, (N, 3))
    if N >= 1 << 31:
        raise ValueError('%d samples: fewer than 2^31 are needed' % N)
    out = torch.empty(N, C, device=tex.device, dtype=torch.float32)
    if N:
        call('nefii_texture_sample', _ptr(tex), T, C, _ptr(face), _ptr(bary), n, c, p, N, _ptr(out))
    return out


# ---- ambient occlusion and bent normals of the baked texels ----------------------------------------------
BAKE_AO_MAX_RAYS = 1024


def _ao_rays(K):
    K = int(K)
    if not 1 <= K <= BAKE_AO_MAX_RAYS:
        raise ValueError('rays must lie in 1 .. %d, got %d' % (BAKE_AO_MAX_RAYS, K))
    return K


def bake_ao_rays(pos, normal, sdf, gnorm, texel, rays, seed=0, bias=0.0, want_uniforms=False):
    """(origins [m,3], dirs [K,m,3], uniforms [K,m,2] or None) float32: the K = rays cosine-weighted hemisphere rays of m
    texels (nefii_bake_ao_rays; include/nefii_amd.h states the sequence).  pos, normal [m,3] (normal of unit length), sdf,
    gnorm [m] float32 - the texels' points, the SDF there and the norm of its gradient; texel [m] int64, the texels' global
    indices j T + i, which with (sample, K, seed) alone decide a direction: a bake in chunks gives the same bits.  origins =
    pos + (bias - sdf / gnorm) normal.  All contiguous and on the GPU."""
    need_gpu(pos, normal, sdf, gnorm, texel)
    m = texel.shape[0] if texel.dim() == 1 else -1
    check_tensor('texel', texel, torch.int64, (None,))
    check_tensor('pos', pos, torch.float32, (m, 3))
    check_tensor('normal', normal, torch.float32, (m, 3))
    check_tensor('sdf', sdf, torch.float32, (m,))
    check_tensor('gnorm', gnorm, torch.float32, (m,))
    K, seed, bias = _ao_rays(rays), int(seed), float(bias)
    if not 0 <= seed < 1 << 32:
        raise ValueError('seed must lie in 0 .. 2^32 - 1, got %d' % seed)
    if m >= 1 << 31:
        raise ValueError('%d texels: fewer than 2^31 are needed' % m)
    dev = pos.device
    origins = torch.empty(m, 3, device=dev, dtype=torch.float32)
    dirs = torch.empty(K, m, 3, device=dev, dtype=torch.float32)
    uniforms = torch.empty(K, m, 2, device=dev, dtype=torch.float32) if want_uniforms else None
    if m:
        call('nefii_bake_ao_rays', _ptr(pos), _ptr(normal), _ptr(sdf), _ptr(gnorm), _ptr(texel), m, K, seed, bias, _ptr(origins),
             _ptr(dirs), _ptr(uniforms))
    return origins, dirs, uniforms


def bake_ao_accumulate(hit, hit_pts, origins, dirs, normal, distance=0.0):
    """(ao [m], bent [m,3]) float32 of m texels from the trace of their K rays (nefii_bake_ao_accumulate): hit [K,m] bool or
    uint8, hit_pts [K,m,3], origins [m,3], dirs [K,m,3], normal [m,3] float32, contiguous and on the GPU.  A hit occludes when
    distance <= 0 or it lies within distance of the origin; ao = the unoccluded share of the K rays, bent = the normalised
    sum of the unoccluded directions (fp64, rounded once), the normal where every ray is occluded."""
    need_gpu(hit, hit_pts, origins, dirs, normal)
    if hit.dtype == torch.bool:
        hit = hit.view(torch.uint8)
    check_tensor('hit', hit, torch.uint8, (None, None))
    K, m = hit.shape
    _ao_rays(K)
    check_tensor('hit_pts', hit_pts, torch.float32, (K, m, 3))
    check_tensor('origins', origins, torch.float32, (m, 3))
    check_tensor('dirs', dirs, torch.float32, (K, m, 3))
    check_tensor('normal', normal, torch.float32, (m, 3))
    if m >= 1 << 31:
        raise ValueError('%d texels: fewer than 2^31 are needed' % m)
    ao = torch.empty(m, device=hit.device, dtype=torch.float32)
    bent = torch.empty(m, 3, device=hit.device, dtype=torch.float32)
    if m:
        call('nefii_bake_ao_accumulate', _ptr(hit), _ptr(hit_pts), _ptr(origins), _ptr(dirs), _ptr(normal), m, K, float(distance),
             _ptr(ao), _ptr(bent))
    return ao, bent


# ---- the diffuse lightmap of the baked texels under a map light ------------------------------------------
def _irradiance_shares(rays_cos, rays_map):
    K_cos, K_map = int(rays_cos), int(rays_map)
    if K_cos < 0 or K_map < 0:
        raise ValueError('the shares of the rays must not be negative, got %d cosine and %d map rays' % (K_cos, K_map))
    _ao_rays(K_cos + K_map)
    return K_cos, K_map


def bake_irradiance_rays(pos, normal, sdf, gnorm, texel, rays_cos, rays_map, envmap, table, coordinate_type, seed=0, bias=0.0,
                         rot=None, want_uniforms=False):
    """(origins [m,3], dirs [K,m,3], weight [K,m,3], uniforms [K,m,2] or None) float32: the K = rays_cos + rays_map rays of m
    texels under the map light envmap [H,W,3] with its envlight_table, and their balance-heuristic weights
    (nefii_bake_irradiance_rays; include/nefii_amd.h states the sequence and the weight).  pos .. texel, seed, bias: as
    bake_ao_rays, whose origins and directions rows 0 .. rays_cos - 1 reproduce bit for bit for rays = rays_cos; the other
    rows are drawn from the map.  rot: None or the rotation R [3,3] (float32, on the GPU, world-from-light) of the light.  The
    irradiance is the sum of the weights of the rows that reach the light unoccluded.  All contiguous and on the GPU."""
    need_gpu(pos, normal, sdf, gnorm, texel)
    m = texel.shape[0] if texel.dim() == 1 else -1
    check_tensor('texel', texel, torch.int64, (None,))
    check_tensor('pos', pos, torch.float32, (m, 3))
    check_tensor('normal', normal, torch.float32, (m, 3))
    check_tensor('sdf', sdf, torch.float32, (m,))
    check_tensor('gnorm', gnorm, torch.float32, (m,))
    K_cos, K_map = _irradiance_shares(rays_cos, rays_map)
    K, seed, bias = K_cos + K_map, int(seed), float(bias)
    if not 0 <= seed < 1 << 32:
        raise ValueError('seed must lie in 0 .. 2^32 - 1, got %d' % seed)
    if m >= 1 << 31:
        raise ValueError('%d texels: fewer than 2^31 are needed' % m)
    coord = _envlight_coord(coordinate_type)
    H, W = _envlight_map(envmap)
    _envlight_table(table, H, W)
    identity = 1
    if rot is not None:
        check_tensor('rot', rot, torch.float32, (3, 3))
        need_gpu(rot)
        identity = int(torch.equal(rot, torch.eye(3, device=rot.device)))
    dev = pos.device
    origins = torch.empty(m, 3, device=dev, dtype=torch.float32)
    dirs = torch.empty(K, m, 3, device=dev, dtype=torch.float32)
    weight = torch.empty(K, m, 3, device=dev, dtype=torch.float32)
    uniforms = torch.empty(K, m, 2, device=dev, dtype=torch.float32) if want_uniforms else None
    if m:
        call('nefii_bake_irradiance_rays', _ptr(pos), _ptr(normal), _ptr(sdf), _ptr(gnorm), _ptr(texel), m, K_cos, K_map, seed, bias,
             _ptr(envmap), _ptr(table), H, W, coord, _ptr(rot), identity, _ptr(origins), _ptr(dirs), _ptr(weight), _ptr(uniforms))
    return origins, dirs, weight, uniforms


def bake_irradiance_accumulate(hit, weight, rays_cos, rays_map):
    """(irradiance [m,3], noise [m]) float32 of m texels from the trace of their rays (nefii_bake_irradiance_accumulate): hit
    [K,m] bool or uint8, weight [K,m,3] float32 as bake_irradiance_rays gave it, K = rays_cos + rays_map, contiguous and on the
    GPU.  irradiance = the sum of the weights of the rows with hit == 0, in fp64 in order of the rows, rounded once; noise = the
    estimated standard error of its luminance.  A row whose weight is zero is never looked up in hit."""
    need_gpu(hit, weight)
    if hit.dtype == torch.bool:
        hit = hit.view(torch.uint8)
    check_tensor('hit', hit, torch.uint8, (None, None))
    K, m = hit.shape
    K_cos, K_map = _irradiance_shares(rays_cos, rays_map)
    if K != K_cos + K_map:
        raise ValueError('hit holds %d rows, the shares %d + %d' % (K, K_cos, K_map))
    check_tensor('weight', weight, torch.float32, (K, m, 3))
    if m >= 1 << 31:
        raise ValueError('%d texels: fewer than 2^31 are needed' % m)
    irradiance = torch.empty(m, 3, device=hit.device, dtype=torch.float32)
    noise = torch.empty(m, device=hit.device, dtype=torch.float32)
    if m:
        call('nefii_bake_irradiance_accumulate', _ptr(hit), _ptr(weight), m, K_cos, K_map, _ptr(irradiance), _ptr(noise))
    return irradiance, noise
