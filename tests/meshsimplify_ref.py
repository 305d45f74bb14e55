"""The oracle of the simplification tests: vertex clustering with quadric error metrics (Lindstrom 2000) restated in fp64
numpy, independent of nefii_amd/mesh.py and csrc/nefii_meshsimplify.hip - np.add.at sums, np.linalg.solve, a dictionary
over the vertex sets -, the directed-edge balance of a face list, and the meshes the tests run on."""
import numpy as np

import mc_ref
import meshcc_ref


# ---- the algorithm -----------------------------------------------------------------------------------------------------
def cluster_vertices(verts, faces, cell):
    """(cluster [V] int64, -1 for a vertex no face uses; centre [C,3] float64; C): cells floor((v - lo) / cell) over the
    used vertices, numbered by ascending (i, j, k)"""
    v = np.asarray(verts).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    cluster = np.full(len(v), -1, dtype=np.int64)
    if len(f) == 0:
        return cluster, np.zeros((0, 3)), 0
    used = np.zeros(len(v), dtype=bool)
    used[f.reshape(-1)] = True
    lo = v[used].min(0)
    ijk = np.floor((v[used] - lo) / float(cell)).astype(np.int64)
    cells, inverse = np.unique(ijk, axis=0, return_inverse=True)        # rows in lexicographic order
    cluster[used] = inverse.reshape(-1)
    return cluster, lo + (cells + 0.5) * float(cell), len(cells)


def quadric_positions(verts, faces, cluster, centre, h, eps=1e-3, clamp=0.5):
    """(pos [C,3] float64, mean [C,3] float64 - the corner-weighted cell means in world space, clamped [C] bool)"""
    v = np.asarray(verts).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    C = len(centre)
    A, b, s, m = np.zeros((C, 3, 3)), np.zeros((C, 3)), np.zeros((C, 3)), np.zeros(C)
    for k in range(3):
        c = cluster[f[:, k]]                                            # the cluster of every face's corner k
        p = [(v[f[:, j]] - centre[c]) / h for j in range(3)]            # the face in that cluster's frame
        nn = np.cross(p[1] - p[0], p[2] - p[0])
        ln = np.linalg.norm(nn, axis=1)
        ok = ln > 0
        n = np.zeros_like(nn)
        n[ok] = nn[ok] / ln[ok, None]
        w = np.where(ok, 0.5 * ln, 0.0)
        d = -(n * p[0]).sum(1)
        np.add.at(A, c, w[:, None, None] * n[:, :, None] * n[:, None, :])
        np.add.at(b, c, (w * d)[:, None] * n)
        np.add.at(s, c, p[k])
        np.add.at(m, c, 1.0)
    x0 = s / m[:, None]
    x = x0.copy()
    trace = A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2]
    for c in np.nonzero(trace > 0)[0]:
        M = A[c] + eps * trace[c] * np.eye(3)
        x[c] = x0[c] + np.linalg.solve(M, -(b[c] + A[c] @ x0[c]))
    clamped = (np.abs(x) > clamp).any(1)
    x = np.clip(x, -clamp, clamp)
    return centre + h * x, centre + h * x0, clamped


def cluster_faces(faces, cluster):
    """(new faces [F',3], kept_face [F'], vertex sets cancelled): the faces over cluster indices; without the faces with a
    repeated index; one face per vertex set, the first of the majority orientation, none where the orientations tie"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    sets = {}
    for i, tri in enumerate(cluster[f].tolist()):
        if len(set(tri)) < 3 or min(tri) < 0:
            continue
        key = tuple(sorted(tri))
        even = tri in ([key[0], key[1], key[2]], [key[1], key[2], key[0]], [key[2], key[0], key[1]])
        sets.setdefault(key, ([], []))[0 if even else 1].append(i)
    kept, cancelled = [], 0
    for even, odd in sets.values():
        if len(even) == len(odd):
            cancelled += 1
        else:
            kept.append(even[0] if len(even) > len(odd) else odd[0])
    kept = np.array(sorted(kept), dtype=np.int64)
    return cluster[f[kept]].reshape(-1, 3), kept, cancelled


def simplify(verts, faces, cell, eps=1e-3, clamp=0.5):
    """-> dict(verts [V',3] float64, faces [F',3], kept_face, clusters, unused (clusters no face uses), cancelled, mean [V',3],
    clamped [C] bool, cluster [V], used [C] bool)"""
    cluster, centre, C = cluster_vertices(verts, faces, cell)
    if C == 0:
        z = np.zeros((0, 3))
        return dict(verts=z, faces=np.zeros((0, 3), dtype=np.int64), kept_face=np.zeros(0, dtype=np.int64), clusters=0,
                    unused=0, cancelled=0, mean=z, clamped=np.zeros(0, dtype=bool), cluster=cluster,
                    used=np.zeros(0, dtype=bool))
    pos, mean, clamped = quadric_positions(verts, faces, cluster, centre, float(cell), eps, clamp)
    nf, kept, cancelled = cluster_faces(faces, cluster)
    used = np.zeros(C, dtype=bool)
    used[nf.reshape(-1)] = True
    new_index = np.cumsum(used) - 1
    return dict(verts=pos[used], faces=new_index[nf], kept_face=kept, clusters=C, unused=int(C - used.sum()),
                cancelled=cancelled, mean=mean[used], clamped=clamped, cluster=cluster, used=used)


def project(value_and_gradient, verts, level=0.0, max_move=np.inf, steps=2):
    start = np.asarray(verts, dtype=np.float64)
    x = start.copy()
    for _ in range(steps):
        f, g = value_and_gradient(x)
        x = x - ((f - level) / np.maximum((g * g).sum(1), 1e-12))[:, None] * g
        x = start + np.clip(x - start, -max_move, max_move)
    return x


# ---- checks ------------------------------------------------------------------------------------------------------------
def unbalanced_edges(faces):
    """the number of directed edges (a, b) that occur another number of times than (b, a): 0 for a closed oriented surface,
    also where an edge carries more than one pair of faces"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    count = {}
    for a, b in np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0).tolist():
        count[(a, b)] = count.get((a, b), 0) + 1
    return sum(1 for (a, b), n in count.items() if count.get((b, a), 0) != n)


def repeated_index_faces(faces):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum())


def shared_vertex_sets(faces):
    f = np.sort(np.asarray(faces, dtype=np.int64).reshape(-1, 3), 1)
    return len(f) - len(np.unique(f, axis=0))


# ---- meshes ------------------------------------------------------------------------------------------------------------
SPHERE = meshcc_ref.SPHERES[0]
THIN_HALF = np.array([0.6, 0.35, 0.03])
_cache = {}


def grid_mesh(name):
    """(verts float32, faces int64, grid spacing) of 'box' / 'sphere' (48^3) or 'thin' (64^3), marching cubes of the exact
    SDF on [-1, 1]^3; computed once, handed out read-only"""
    if name not in _cache:
        n = 64 if name == 'thin' else 48
        p = meshcc_ref.grid_points(n)
        vol = {'box': lambda: meshcc_ref.box_sdf(p), 'sphere': lambda: meshcc_ref.sphere_sdf(p, *SPHERE),
               'thin': lambda: meshcc_ref.box_sdf(p, half=THIN_HALF)}[name]()
        sp = 2.0 / (n - 1)
        v, f = mc_ref.marching_cubes(vol.astype(np.float32), 0.0, origin=(-1.0, -1.0, -1.0), spacing=(sp, sp, sp))
        v.setflags(write=False)
        f.setflags(write=False)
        _cache[name] = (v, f, sp)
    return _cache[name]


def field(name):
    """the exact SDF of a grid_mesh, as a function of points [N,3]"""
    return {'box': meshcc_ref.box_sdf, 'sphere': lambda q: meshcc_ref.sphere_sdf(q, *SPHERE),
            'thin': lambda q: meshcc_ref.box_sdf(q, half=THIN_HALF)}[name]


# (mesh, cell in grid spacings): the closed inputs of the issue
CASES = [('box', 2.0), ('box', 3.0), ('box', 4.5), ('sphere', 2.0), ('sphere', 3.0), ('sphere', 4.5), ('thin', 4.0)]


def fan(n, radius=0.4, centre=(0.05, 0.02, 0.01), lift=0.1, seed=0, scale=(1.0, 1.0, 1.0)):
    """n triangles around vertex 0 (a cone of height `lift` with a slightly irregular rim, stretched by `scale` along the
    axes) -> (verts float32, faces)"""
    r = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n) / n
    rad = radius * (1.0 + 0.1 * r.uniform(-1, 1, n))
    rim = np.stack([rad * np.cos(ang), rad * np.sin(ang), 0.02 * r.uniform(-1, 1, n)], 1)
    verts = np.concatenate([[[0.0, 0.0, lift]], rim], 0) * np.asarray(scale) + np.asarray(centre)
    i = np.arange(n, dtype=np.int64)
    faces = np.stack([np.zeros(n, dtype=np.int64), 1 + i, 1 + (i + 1) % n], 1)
    return verts.astype(np.float32), faces
