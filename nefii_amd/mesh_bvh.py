"""A bounding-volume hierarchy over the faces of a triangle mesh, for the exact signed-distance query of
datasets/sdf_dataset.py:MeshSDF (kernel: csrc/nefii_meshsdf.hip).

The build is a handful of torch ops on whatever device the triangles live on (CPU included), one-off per mesh:
  * 63-bit Morton codes of the face centroids, 21 bits per axis over the centroids' bounding box, as int64;
  * a stable sort of the codes gives the face permutation;
  * LEAF consecutive faces form a leaf; the leaf count is padded to a power of two N;
  * the tree is the implicit complete binary tree in heap order over those N leaves - node i has the children 2 i + 1 and
    2 i + 2, the leaves are the nodes N - 1 .. 2 N - 2 - so it has no pointers;
  * node boxes [2 N - 1, 6] = (lo.xyz, hi.xyz) are the plain fp64 min / max of the fp64 vertices, bottom-up, one reshaped
    amin / amax per level.  Padding leaves are empty: lo = +inf, hi = -inf, which every box test rejects.
Contract: every face lies inside its leaf's box, every box contains its children's.  No atomics: two builds are bitwise equal.
build_moments adds, on first use, what the winding-number query needs per node: dipole moment, centre, radius.
"""
import torch

LEAF = 4
MAX_FACES = (1 << 26) - 1           # the query kernel's stack holds 26 levels: N <= 2^26 leaves


def _spread21(x):
    """the low 21 bits of int64 x, two zero bits inserted after each"""
    x = x & 0x1fffff
    x = (x | (x << 32)) & 0x1f00000000ffff
    x = (x | (x << 16)) & 0x1f0000ff0000ff
    x = (x | (x << 8)) & 0x100f00f00f00f00f
    x = (x | (x << 4)) & 0x10c30c30c30c30c3
    x = (x | (x << 2)) & 0x1249249249249249
    return x


def morton63(points, lo, hi):
    """63-bit Morton codes (int64) of points [P, 3] on the 2^21 grid over the box lo .. hi (points outside are clamped)"""
    extent = (hi - lo).clamp_min(torch.finfo(points.dtype).tiny)
    cell = ((points - lo) / extent * float((1 << 21) - 1)).floor().clamp(0, (1 << 21) - 1).to(torch.int64)
    return (_spread21(cell[:, 0]) << 2) | (_spread21(cell[:, 1]) << 1) | _spread21(cell[:, 2])


class MeshBVH:
    """perm [F] int64: sorted position -> face; tris [F, 9] fp64: the sorted faces (a | b | c); node_box [2 N - 1, 6] fp64;
    n_leaves = N (a power of two); leaf_size"""

    def __init__(self, perm, tris, node_box, n_leaves, leaf_size):
        self.perm, self.tris, self.node_box, self.n_leaves, self.leaf_size = perm, tris, node_box, n_leaves, leaf_size
        self.node_moment = None                     # build_moments fills it on first use

    @property
    def n_faces(self):
        return self.tris.shape[0]

    @property
    def levels(self):
        return self.n_leaves.bit_length()           # levels of nodes, the root's and the leaves' included


def build_bvh(a, b, c, leaf_size=LEAF):
    """a, b, c [F, 3] fp64: the corners of F faces of non-zero area, 1 <= F < 2^26 -> MeshBVH on their device"""
    if not 1 <= leaf_size <= 8:
        raise ValueError('leaf_size must lie in 1 .. 8, got %r' % (leaf_size,))
    F = a.shape[0]
    if not 1 <= F <= MAX_FACES:
        raise ValueError('a BVH takes 1 .. 2^26 - 1 faces, got %d' % F)
    tris = torch.stack([a, b, c], 1).to(torch.float64)                   # [F, 3 corners, 3]
    centroid = tris.mean(1)
    perm = torch.sort(morton63(centroid, centroid.amin(0), centroid.amax(0)), stable=True).indices
    tris = tris[perm]
    n_leaves = 1
    while n_leaves * leaf_size < F:
        n_leaves *= 2
    pad = n_leaves * leaf_size - F
    inf = torch.full((pad, 3), float('inf'), dtype=torch.float64, device=tris.device)
    lo = torch.cat([tris.amin(1), inf], 0).reshape(n_leaves, leaf_size, 3).amin(1)
    hi = torch.cat([tris.amax(1), -inf], 0).reshape(n_leaves, leaf_size, 3).amax(1)
    levels = [torch.cat([lo, hi], 1)]
    while lo.shape[0] > 1:
        lo, hi = lo.reshape(-1, 2, 3).amin(1), hi.reshape(-1, 2, 3).amax(1)
        levels.append(torch.cat([lo, hi], 1))
    node_box = torch.cat(levels[::-1], 0).contiguous()                   # heap order: root first, leaves last
    return MeshBVH(perm, tris.reshape(F, 9).contiguous(), node_box, n_leaves, leaf_size)


RADIUS_GROW = 1.0 + 2.0 ** -40      # keeps "every vertex within r of p" true under the rounding of the two norms


def build_moments(bvh):
    """node_moment [2 N - 1, 8] fp64 = (p.xyz, r, n.xyz, area) per node of the tree, for the winding-number query
    (csrc/nefii_meshsdf.hip); cached on the MeshBVH.
      n     the sum over the node's faces of the area vectors 0.5 (b - a) x (c - a): the dipole moment of the node;
      area  the sum of the faces' areas; 0 marks an empty (padding) node, whose row is all zeros;
      p     the area-weighted mean of the faces' centroids;
      r     the distance from p to the farthest corner of the node's box, norm(max(p - lo, hi - p)), times 1 + 2^-40.
    Contract: every vertex of a node lies within r of p.  n, area and sum(area centroid) are summed bottom-up, one reshaped
    sum per level, padding faces adding zeros; no atomics: two builds are bitwise equal."""
    if bvh.node_moment is not None:
        return bvh.node_moment
    F, N, leaf = bvh.n_faces, bvh.n_leaves, bvh.leaf_size
    a, b, c = bvh.tris[:, 0:3], bvh.tris[:, 3:6], bvh.tris[:, 6:9]
    n = 0.5 * torch.cross(b - a, c - a, dim=1)
    area = n.norm(dim=1, keepdim=True)
    face = torch.cat([n, area, area * ((a + b + c) / 3.0)], 1)           # [F, 7]: n, area, area * centroid
    face = torch.cat([face, face.new_zeros(N * leaf - F, 7)], 0)
    level = face.reshape(N, leaf, 7).sum(1)
    levels = [level]
    while level.shape[0] > 1:
        level = level.reshape(-1, 2, 7).sum(1)
        levels.append(level)
    s = torch.cat(levels[::-1], 0)                                       # heap order, as node_box
    area = s[:, 3:4]
    full = area > 0
    p = torch.where(full, s[:, 4:7] / torch.where(full, area, torch.ones_like(area)), torch.zeros_like(area))
    lo, hi = bvh.node_box[:, :3], bvh.node_box[:, 3:]
    r = torch.where(full[:, 0], torch.maximum(p - lo, hi - p).norm(dim=1) * RADIUS_GROW, torch.zeros_like(area[:, 0]))
    bvh.node_moment = torch.cat([p, r[:, None], s[:, 0:3], area], 1).contiguous()
    return bvh.node_moment
