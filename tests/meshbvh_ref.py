"""Shared pieces of the mesh-BVH tests (test_mesh_bvh_cpu.py, test_gpu_mesh_sdf.py): the test meshes, a slow numpy walk of
the tree under the query kernel's two pruning rules, brute-force numpy counterparts, and the sign-fragility measure.
Nothing here touches the kernel: the reference of every comparison is MeshSDF(method='brute') or numpy."""
import numpy as np
import torch

TORUS_R, TORUS_r = 0.6, 0.25
BOX_SHRINK = 1.0 - 2.0 ** -40          # csrc/nefii_meshsdf.hip: the box test's safety factor


def torus_mesh(nu, nv, R=TORUS_R, r=TORUS_r):
    """closed torus about the z axis: nu x nv quads, two triangles each -> (vertices [nu nv, 3], faces [2 nu nv, 3])"""
    u, v = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing='ij')
    verts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing='ij')
    i1, j1 = (i + 1) % nu, (j + 1) % nv
    v00, v10, v11, v01 = i * nv + j, i1 * nv + j, i1 * nv + j1, i * nv + j1
    faces = np.stack([np.stack([v00, v10, v11], -1), np.stack([v00, v11, v01], -1)], 2).reshape(-1, 3)
    return verts, faces.astype(np.int64)


def torus_sdf(p, R=TORUS_R, r=TORUS_r):
    return np.sqrt((np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - R) ** 2 + p[:, 2] ** 2) - r


def equal_morton_mesh():
    """64 copies of one triangle and 32 copies scaled by powers of two about its centroid (the origin, exactly): every
    centroid is the same point, so every Morton code is equal and the sort decides nothing"""
    tri = np.array([[0.5, 0.25, 0.125], [-0.125, 0.25, -0.5], [-0.375, -0.5, 0.375]])
    assert np.all(tri.sum(0) == 0)
    scales = [1.0] * 64 + [2.0 ** -(1 + k % 5) for k in range(32)]
    verts = np.concatenate([tri * s for s in scales])
    return verts, np.arange(len(verts)).reshape(-1, 3).astype(np.int64)


def surface_points(verts, faces, count, rng):
    f = faces[rng.integers(0, len(faces), count)]
    w = rng.dirichlet(np.ones(3), count)
    return (verts[f] * w[:, :, None]).sum(1)


# ---- numpy counterparts of MeshSDF's per-face terms (broadcasting over leading axes) -----------------------------------
def _dot(a, b):
    return (a * b).sum(-1)


def _segment_d2(p, a, ab):
    t = np.clip(_dot(p - a, ab) / np.maximum(_dot(ab, ab), 1e-300), 0, 1)
    d = p - (a + t[..., None] * ab)
    return _dot(d, d)


def triangle_d2(p, a, b, c):
    n = np.cross(b - a, c - a)
    inside = (_dot(np.cross(b - a, p - a), n) >= 0) & (_dot(np.cross(c - b, p - b), n) >= 0) & \
             (_dot(np.cross(a - c, p - c), n) >= 0)
    d_plane = _dot(p - a, n) ** 2 / _dot(n, n)
    d_edge = np.minimum(np.minimum(_segment_d2(p, a, b - a), _segment_d2(p, b, c - b)), _segment_d2(p, c, a - c))
    return np.where(inside, d_plane, d_edge)


def edge_functions(q, a, b, c):
    def edge(u, v):
        return (v[..., 0] - u[..., 0]) * (q[..., 1] - u[..., 1]) - (v[..., 1] - u[..., 1]) * (q[..., 0] - u[..., 0])
    return edge(a, b), edge(b, c), edge(c, a)


def ray_crosses(q, a, b, c):
    e0, e1, e2 = edge_functions(q, a, b, c)
    covers = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
    area2 = e0 + e1 + e2
    z = (e1 * a[..., 2] + e2 * b[..., 2] + e0 * c[..., 2]) / np.where(area2 == 0, 1.0, area2)
    return covers & (area2 != 0) & (z > q[..., 2])


def brute_numpy(q, tris):
    """q [P, 3], tris [F, 9] in one frame -> (distance [P], crossing count [P]) over ALL faces"""
    a, b, c = tris[None, :, 0:3], tris[None, :, 3:6], tris[None, :, 6:9]
    p = q[:, None, :]
    return np.sqrt(triangle_d2(p, a, b, c).min(1)), ray_crosses(p, a, b, c).sum(1)


def walk_tree(bvh, q):
    """The kernel's two traversals in numpy, one query at a time: q [P, 3] in the tree's frame -> (distance [P], crossing
    count [P], faces evaluated by pass A [P]).  Pass A skips a node only when box d^2 (1 - 2^-40) > best or the node is
    empty; pass B enters a node only if q.xy is inside its xy box and its hi.z > q.z."""
    box, tris = bvh.node_box.cpu().numpy(), bvh.tris.cpu().numpy()
    N, leaf, F = bvh.n_leaves, bvh.leaf_size, bvh.tris.shape[0]
    first_leaf = N - 1

    def faces_of(node):
        f0 = (node - first_leaf) * leaf
        t = tris[f0:min(f0 + leaf, F)]
        return t[:, 0:3], t[:, 3:6], t[:, 6:9]

    def box_d2(node, p):
        d = np.maximum(np.maximum(box[node, :3] - p, p - box[node, 3:]), 0.0)
        return (d * d).sum()

    def cannot_improve(d2, best):
        return d2 * BOX_SHRINK > best or not d2 < np.inf

    def may_cross(node, p):
        lo, hi = box[node, :3], box[node, 3:]
        return lo[0] <= p[0] <= hi[0] and lo[1] <= p[1] <= hi[1] and hi[2] > p[2]

    dist, count, visited = np.empty(len(q)), np.zeros(len(q), dtype=np.int64), np.zeros(len(q), dtype=np.int64)
    for i, p in enumerate(q):
        best, stack = np.inf, [0]
        while stack:
            node = stack.pop()
            if node != 0 and cannot_improve(box_d2(node, p), best):
                continue
            if node >= first_leaf:
                a, b, c = faces_of(node)
                if len(a):
                    best = min(best, triangle_d2(p[None], a, b, c).min())
                    visited[i] += len(a)
                continue
            c0, c1 = 2 * node + 1, 2 * node + 2
            d0, d1 = box_d2(c0, p), box_d2(c1, p)
            near, far = (c1, c0) if d1 < d0 else (c0, c1)
            stack += [far, near]                    # the nearer child is popped first
        dist[i] = np.sqrt(best)
        stack = [0]
        while stack:
            node = stack.pop()
            if not may_cross(node, p):
                continue
            if node >= first_leaf:
                a, b, c = faces_of(node)
                if len(a):
                    count[i] += ray_crosses(p[None], a, b, c).sum()
                continue
            stack += [2 * node + 2, 2 * node + 1]
    return dist, count, visited


def fragile(mesh_sdf, points, tol=1e-12, chunk=1 << 24):
    """[P] bool: queries at which some face's 2-D edge function (MeshSDF's parity terms, in its skewed frame) is smaller in
    magnitude than tol - the only queries whose `covers` a differently rounded product could decide differently.
    Plain array arithmetic on the mesh's device, in chunks; independent of the tree and of the kernel."""
    p = torch.as_tensor(points, dtype=torch.float64, device=mesh_sdf.device).reshape(-1, 3)
    q = p @ mesh_sdf.R.T
    ra, rb, rc = mesh_sdf.ra[None], mesh_sdf.rb[None], mesh_sdf.rc[None]
    out = torch.empty(q.shape[0], dtype=torch.bool, device=q.device)
    step = max(1, chunk // ra.shape[1])
    for s in range(0, q.shape[0], step):
        qq = q[s:s + step, None, :]
        e = torch.stack(edge_functions(qq, ra, rb, rc), -1).abs()
        out[s:s + step] = e.reshape(e.shape[0], -1).min(1).values < tol
    return out.cpu().numpy()
