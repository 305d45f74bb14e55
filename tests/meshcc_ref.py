"""The oracle of the component-labelling tests: a plain union-find over the faces' edges that gives every vertex the smallest
vertex index of its component (the contract of csrc/nefii_meshcc.hip), and the meshes and fields those tests are run on."""
import numpy as np


def labels(faces, n_verts):
    """[V] int64: the smallest vertex index of the edge-connected component of each vertex; a vertex in no face: itself"""
    parent = list(range(n_verts))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        ra, rb, rc = find(a), find(b), find(c)
        r = min(ra, rb, rc)
        parent[ra] = parent[rb] = parent[rc] = r
    return np.array([find(v) for v in range(n_verts)], dtype=np.int64)      # roots only ever move down: root = minimum


def same_partition(l0, l1):
    """do two labellings split the vertices into the same sets?"""
    pairs = np.unique(np.stack([np.asarray(l0), np.asarray(l1)], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


# ---- meshes ------------------------------------------------------------------------------------------------------------
TETRA = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int64)


def tetrahedra(n):
    """n disjoint tetrahedra over 4 n vertices -> faces [4 n, 3]"""
    return np.concatenate([TETRA + 4 * i for i in range(n)], 0)


def strip(n_tris, seed=None):
    """a strip of n_tris triangles (i, i + 1, i + 2) over n_tris + 2 vertices, one component that is one long chain;
    seed: the vertex numbers randomly permuted -> (faces, n_verts)"""
    i = np.arange(n_tris, dtype=np.int64)
    faces = np.stack([i, i + 1, i + 2], 1)
    if seed is not None:
        faces = np.random.default_rng(seed).permutation(n_tris + 2)[faces]
    return faces, n_tris + 2


# ---- fields ------------------------------------------------------------------------------------------------------------
SPHERES = (((-0.4, 0.0, 0.0), 0.45), ((0.55, 0.1, 0.0), 0.3), ((0.1, 0.8, 0.7), 0.1))


def sphere_sdf(p, centre, radius):
    return np.linalg.norm(p - np.asarray(centre, dtype=np.float64), axis=-1) - radius


def grid_points(n, bound=1.0):
    """[n, n, n, 3] float64: linspace(-bound, bound, n)^3, x slowest"""
    ax = np.linspace(-bound, bound, n)
    return np.stack(np.meshgrid(ax, ax, ax, indexing='ij'), -1)


def rot(axis, degrees):
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = c, -s, s, c
    return r


BOX_HALF = np.array([0.6, 0.35, 0.2])
BOX_CENTRE = np.array([0.05, -0.1, 0.1])
BOX_ROT = rot(2, 30.0) @ rot(0, 20.0) @ rot(1, -25.0)           # columns: the box's axes in world space
FLOATER = ((-0.8, 0.8, -0.8), 0.08)
BOX_AREA = 8.0 * (BOX_HALF[0] * BOX_HALF[1] + BOX_HALF[1] * BOX_HALF[2] + BOX_HALF[0] * BOX_HALF[2])


def box_sdf(p, half=BOX_HALF, centre=BOX_CENTRE, rotation=BOX_ROT):
    """the exact (1-Lipschitz) signed distance to the rotated box"""
    q = np.abs((np.asarray(p, dtype=np.float64) - centre) @ rotation) - half
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def box_scene_sdf(p):
    """the rotated box and a small sphere far from it"""
    return np.minimum(box_sdf(p), sphere_sdf(p, *FLOATER))


def box_cloud(half, rotation, centre, n, seed, outliers=()):
    """n seeded points uniform in a rotated box, its 8 corners, and for each local axis in `outliers` the two points at
    +-1 along it (they stretch that axis' extent without turning the principal axes)"""
    r = np.random.default_rng(seed)
    half = np.asarray(half, dtype=np.float64)
    local = [r.uniform(-1.0, 1.0, (n, 3)) * half,
             np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64) * half]
    for a in outliers:
        e = np.zeros((2, 3))
        e[0, a], e[1, a] = 1.0, -1.0
        local.append(e)
    return np.concatenate(local, 0) @ rotation.T + np.asarray(centre, dtype=np.float64)
