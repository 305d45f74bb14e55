"""Shared pieces of the winding-number tests (test_mesh_winding_cpu.py, test_gpu_mesh_winding.py): the open and
the overlapping test meshes, their seeded query batches, brute-force winding numbers in numpy, and a numpy walk of the tree
under the kernel's exact accept rule.  Nothing here touches the kernel: the reference of every comparison is this file or
MeshSDF(method='brute').winding."""
import numpy as np

import meshbvh_ref as mr

NU, NV = 48, 24                        # the suite's torus: 2304 faces
HOLE = 6                               # the open torus lacks the quads u 0..5 x v 0..5
SHIFT = np.array([0.3, 0.0, 0.0])      # the second torus of the union
CLEAR = 0.05                           # queries keep this distance from the analytic torus (the mesh is within 0.002 of it)
FRAGILE_TOL = 1e-12

# max |w_walk(beta) - w_brute| over queries('walk') of each mesh, measured on the CPU in fp64 (test_mesh_winding_cpu.py
# prints them): the truncation error of the dipole term, a property of the algorithm and not derivable.
MEASURED_ERROR = {
    ('closed', 2.0): 0.02831, ('open', 2.0): 0.02925, ('union', 2.0): 0.03857,
    ('closed', 4.0): 0.003395, ('open', 4.0): 0.003217, ('union', 4.0): 0.006716,
}


def guard_band(beta):
    """E(beta): twice the largest measured error at beta, the margin being for other seeds - what the tests assert the walk
    and the kernel to stay within of brute force, and how far from 0.5 a winding number must lie for its sign to be held"""
    return 2.0 * max(v for (_, b), v in MEASURED_ERROR.items() if b == beta)


def mesh(kind):
    """(vertices, faces) of 'closed' (the 2304-face torus), 'open' (2232 faces: a patch of 6 x 6 quads removed), 'union' (4608
    faces: the torus and a copy shifted by SHIFT, pushed into each other) and 'inside_out' (the torus, every face reversed)"""
    verts, faces = mr.torus_mesh(NU, NV)
    if kind == 'closed':
        return verts, faces
    if kind == 'open':
        i, j = np.meshgrid(np.arange(NU), np.arange(NV), indexing='ij')
        keep = np.repeat(~((i < HOLE) & (j < HOLE)).reshape(-1), 2)           # two faces per quad, quads in (i, j) order
        return verts, faces[keep]
    if kind == 'union':
        return np.concatenate([verts, verts + SHIFT]), np.concatenate([faces, faces + len(verts)])
    if kind == 'inside_out':
        return verts, np.ascontiguousarray(faces[:, ::-1])
    raise ValueError(kind)


def inside_count(p, kind):
    """how many of the analytic tori behind mesh(kind) hold p: the winding number a closed version of the mesh would have"""
    n = (mr.torus_sdf(p) < 0).astype(np.int64)
    return n + (mr.torus_sdf(p - SHIFT) < 0) if kind == 'union' else n


def queries(kind, batch):
    """seeded queries, uniform in [-1, 1]^3 less those within CLEAR of a torus surface: batch 'table' draws 4096 (the sign
    tables), 'walk' draws 768 (everything that walks the tree in numpy).
    The open torus has no true inside right under its hole: the surface w = 0.5 that closes it dips up to 0.07 below the
    analytic torus there (measured: w = 0.46 .. 0.499 at depths 0.05 .. 0.07 under the hole), so of twenty seeds of 4096 queries
    seven put one or two of them into that layer.  Seed 13 puts none there, in either batch."""
    seed = {'closed': 11, 'open': 13, 'union': 15}[kind] + (0 if batch == 'table' else 100)
    p = np.random.default_rng(seed).uniform(-1, 1, ({'table': 4096, 'walk': 768}[batch], 3))
    keep = np.abs(mr.torus_sdf(p)) >= CLEAR
    if kind == 'union':
        keep &= np.abs(mr.torus_sdf(p - SHIFT)) >= CLEAR
    return p[keep]


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def solid_angle(q, a, b, c):
    """Van Oosterom & Strackee, term for term as csrc/nefii_meshsdf.hip forms it (broadcasting over leading axes)"""
    A, B, C = a - q, b - q, c - q
    la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
    num = _dot(A, np.cross(B, C))
    den = la * lb * lc + _dot(A, B) * lc + _dot(B, C) * la + _dot(C, A) * lb
    return 2.0 * np.arctan2(num, den)


def brute_winding(q, tris, chunk=1 << 21):
    """q [P, 3], tris [F, 9] in one frame -> w [P]: the sum over ALL faces, in the order of tris"""
    out = np.empty(len(q))
    step = max(1, chunk // len(tris))
    for s in range(0, len(q), step):
        p = q[s:s + step, None, :]
        out[s:s + step] = solid_angle(p, tris[None, :, 0:3], tris[None, :, 3:6], tris[None, :, 6:9]).sum(1) / (4.0 * np.pi)
    return out


def walk_winding(bvh, moment, q, beta, tol=FRAGILE_TOL):
    """The kernel's traversal in numpy: q [P, 3] in the tree's frame -> (w [P], decision-fragile [P] bool, faces evaluated
    [P]).  The nodes are visited in pre-order, the left child first, each with the queries that reach it - for every single
    query that is the kernel's order of additions.  An empty node (area == 0) is skipped; a leaf adds its faces' solid angles
    one by one; an inner node with beta > 0 and dot(d, d) > (beta r) (beta r), d = p - q, adds n . d / (dd sqrt(dd)) and is not
    descended.  A query is decision-fragile if at some inner node it visits |dot(d, d) - (beta r)^2| <= tol (beta r)^2."""
    mom, tris = moment.cpu().numpy(), bvh.tris.cpu().numpy()
    N, leaf, F = bvh.n_leaves, bvh.leaf_size, bvh.tris.shape[0]
    first_leaf = N - 1
    total, frag, faces = np.zeros(len(q)), np.zeros(len(q), dtype=bool), np.zeros(len(q), dtype=np.int64)

    def visit(node, idx):
        if len(idx) == 0:
            return
        if node >= first_leaf:
            f0 = (node - first_leaf) * leaf
            for t in tris[f0:min(f0 + leaf, F)]:
                total[idx] += solid_angle(q[idx], t[0:3], t[3:6], t[6:9])
                faces[idx] += 1
            return
        p, r, n, area = mom[node, 0:3], mom[node, 3], mom[node, 4:7], mom[node, 7]
        if area == 0.0:
            return
        d = p - q[idx]
        dd, br = _dot(d, d), beta * r
        far = (dd > br * br) if beta > 0.0 else np.zeros(len(idx), dtype=bool)
        if beta > 0.0:
            frag[idx] |= np.abs(dd - br * br) <= tol * (br * br)
        total[idx[far]] += _dot(n, d[far]) / (dd[far] * np.sqrt(dd[far]))
        visit(2 * node + 1, idx[~far])
        visit(2 * node + 2, idx[~far])

    visit(0, np.arange(len(q)))
    return total / (4.0 * np.pi), frag, faces
