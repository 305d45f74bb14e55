"""fp64 numpy restatement of the texture bake (include/nefii_amd.h "THE ATLAS", csrc/nefii_texbake.hip, nefii_amd/texture.py):
the per-face-chart atlas, the raster, the 8-bit encoding, the bilinear sampler and a whole bake of an analytic field.  Written
from the contract, with loops and dictionaries where the product has index arithmetic; nothing here imports the package."""
import math

import numpy as np

CASES = [(1, 7), (2, 7), (3, 14), (37, 61), (200, 160)]         # (faces, size): the shapes every layer is held to


def atlas(n_faces, size, pad=2):
    """dict(T, n, c, p, s, F) - ValueError where the contract refuses"""
    F, T, p = int(n_faces), int(size), int(pad)
    if not 7 <= T <= 8192 or p < 2 or F < 1:
        raise ValueError('outside the limits')
    n = int(math.ceil(math.sqrt(math.ceil(F / 2))))
    while n * n < (F + 1) // 2:                                   # sqrt in floating point: settle it in integers
        n += 1
    while n > 1 and (n - 1) * (n - 1) >= (F + 1) // 2:
        n -= 1
    c = T // n
    s = c - 3 * p
    if s < 1:
        raise ValueError('leg below one texel')
    return dict(T=T, n=n, c=c, p=p, s=s, F=F)


def corners_xy(a, f):
    """[3, 2] float64: the chart corners of face f in texel units"""
    q = f // 2
    x0, y0 = a['c'] * (q % a['n']), a['c'] * (q // a['n'])
    c, p, s = a['c'], a['p'], a['s']
    if f % 2 == 0:
        return np.array([[x0 + p, y0 + p], [x0 + p + s, y0 + p], [x0 + p, y0 + p + s]], dtype=np.float64)
    return np.array([[x0 + c - p, y0 + c - p], [x0 + c - p - s, y0 + c - p], [x0 + c - p, y0 + c - p - s]], dtype=np.float64)


def corner_uv(a):
    xy = np.stack([corners_xy(a, f) for f in range(a['F'])])
    return np.stack([xy[..., 0] / a['T'], 1.0 - xy[..., 1] / a['T']], -1)


def owner_of(a, i, j):
    c, n = a['c'], a['n']
    if i >= n * c or j >= n * c:
        return -1
    q = (j // c) * n + (i // c)
    if q >= (a['F'] + 1) // 2:
        return -1
    f = 2 * q if (i % c) + (j % c) + 1 < c else 2 * q + 1
    return f if f < a['F'] else -1


def owner_image(a):
    T = a['T']
    return np.array([[owner_of(a, i, j) for i in range(T)] for j in range(T)], dtype=np.int32)


def raster(a, verts, faces):
    """(owner [T,T] int32, covered [T,T] bool, bary [T,T,2] float64 = (b1, b2), pos [T,T,3] float64), texel by texel: the
    barycentrics of the texel's centre by solving the chart's 2 x 2 system in exact integers over 2 s"""
    T, s = a['T'], a['s']
    verts = np.asarray(verts, dtype=np.float64)
    owner = owner_image(a)
    covered = np.zeros((T, T), dtype=bool)
    bary = np.zeros((T, T, 2))
    pos = np.zeros((T, T, 3))
    for j in range(T):
        for i in range(T):
            f = owner[j, i]
            if f < 0:
                continue
            C = corners_xy(a, f)
            sign = 1 if f % 2 == 0 else -1
            # twice the centre's offset from corner 0, along the legs (which run in +x, +y or -x, -y): integers
            k1 = sign * ((2 * i + 1) - 2 * int(C[0, 0]))
            k2 = sign * ((2 * j + 1) - 2 * int(C[0, 1]))
            k0 = 2 * s - k1 - k2
            covered[j, i] = k0 >= 0 and k1 >= 0 and k2 >= 0
            b0, b1, b2 = k0 / (2 * s), k1 / (2 * s), k2 / (2 * s)
            bary[j, i] = (b1, b2)
            v0, v1, v2 = verts[faces[f][0]], verts[faces[f][1]], verts[faces[f][2]]
            pos[j, i] = b0 * v0 + b1 * v1 + b2 * v2
    return owner, covered, bary, pos


def level_value(x):
    """255 clamp(x, 0, 1) + 0.5, before the floor"""
    return 255.0 * np.clip(np.asarray(x, dtype=np.float64), 0.0, 1.0) + 0.5


def encode(albedo, roughness, normal, owner):
    """(rgba_albedo [N,4], rgba_normal [N,4], grey [N]) uint8 and the three arrays of fp64 values before the floor"""
    albedo, normal = np.asarray(albedo, dtype=np.float64), np.asarray(normal, dtype=np.float64)
    own = np.asarray(owner) >= 0
    va = level_value(np.maximum(albedo, 0.0) ** (1.0 / 2.2))
    vn = level_value(0.5 * normal + 0.5)
    vr = level_value(np.asarray(roughness, dtype=np.float64))
    N = len(own)
    ra, rn = np.zeros((N, 4), dtype=np.uint8), np.zeros((N, 4), dtype=np.uint8)
    ra[:, :3], rn[:, :3] = np.floor(va), np.floor(vn)
    ra[:, 3] = rn[:, 3] = 255
    grey = np.floor(vr).astype(np.uint8)
    ra[~own], rn[~own], grey[~own] = 0, 0, 0
    return ra, rn, grey, (va, vn, vr)


def atlas_position(a, face, bary):
    """[N, 2] float64: where (face, barycentrics) falls in the atlas, in texel units"""
    out = np.zeros((len(face), 2))
    for k, (f, b) in enumerate(zip(face, np.asarray(bary, dtype=np.float64))):
        C = corners_xy(a, int(f))
        out[k] = b[0] * C[0] + b[1] * C[1] + b[2] * C[2]
    return out


def footprint(a, xy):
    """the bilinear footprint of one atlas position: [(i, j, weight)] of the (up to) four texels, indices clamped to the image"""
    T = a['T']
    u, v = xy[0] - 0.5, xy[1] - 0.5
    fu, fv = math.floor(u), math.floor(v)
    wx, wy = u - fu, v - fv
    clamp = lambda t: min(max(int(t), 0), T - 1)                            # noqa: E731
    return [(clamp(fu), clamp(fv), (1 - wx) * (1 - wy)), (clamp(fu + 1), clamp(fv), wx * (1 - wy)),
            (clamp(fu), clamp(fv + 1), (1 - wx) * wy), (clamp(fu + 1), clamp(fv + 1), wx * wy)]


def sample(a, tex, face, bary):
    """[N, C] float64: the bilinear lookup of tex [T, T, C] at (face, barycentrics)"""
    tex = np.asarray(tex, dtype=np.float64)
    out = np.zeros((len(face), tex.shape[2]))
    for k, xy in enumerate(atlas_position(a, face, bary)):
        for i, j, w in footprint(a, xy):
            out[k] += w * tex[j, i]
    return out


def chart_points(a, rng, per_face):
    """(face [N], bary [N, 3]): for every face its three corners, its three edge midpoints, a point on each edge and
    per_face random interior points"""
    fixed = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]]
    face, bary = [], []
    for f in range(a['F']):
        t = rng.random()
        pts = fixed + [[t, 1 - t, 0], [0, t, 1 - t], [1 - t, 0, t]]
        r = rng.random((per_face, 2))
        r1 = np.sqrt(r[:, 0])
        pts += np.stack([1 - r1, r1 * (1 - r[:, 1]), r1 * r[:, 1]], 1).tolist()
        face += [f] * len(pts)
        bary += pts
    return np.array(face, dtype=np.int64), np.array(bary, dtype=np.float64)


# ---- a whole bake of an analytic field on the unit sphere --------------------------------------------------------------------
def icosphere(subdivisions):
    """(verts [V,3] float64 on the unit sphere, faces [F,3] int64, outward): F = 20 x 4^subdivisions"""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a_, b_, c_ in f:
            ab, bc, ca = m(a_, b_), m(b_, c_), m(c_, a_)
            nf += [(a_, ab, ca), (b_, bc, ab), (c_, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, dtype=np.int64)


def sphere_material(x):
    """[N, 4]: an analytic albedo (3) and roughness (1) on the unit sphere, a few periods around it"""
    x = np.asarray(x, dtype=np.float64)
    a = 0.5 + 0.4 * np.stack([np.sin(5.0 * x[:, 0] + 1.0) * np.cos(4.0 * x[:, 1]), np.sin(6.0 * x[:, 1] - 0.5) * np.cos(3.0 * x[:, 2]),
                              np.sin(4.0 * x[:, 2] + 0.3) * np.cos(5.0 * x[:, 0])], 1)
    r = 0.5 + 0.4 * np.sin(3.0 * x[:, 0] + 2.0 * x[:, 1] - 4.0 * x[:, 2])
    return np.concatenate([a, r[:, None]], 1)


def project_sphere(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def bake_sphere(verts, faces, size, pad=2):
    """(atlas, tex [T,T,4] float64, owner): the analytic material baked at every owned texel's own point, moved onto the sphere"""
    a = atlas(len(faces), size, pad)
    owner, _, _, pos = raster(a, verts, faces)
    tex = np.zeros((a['T'], a['T'], 4))
    own = owner >= 0
    tex[own] = sphere_material(project_sphere(pos[own]))
    return a, tex, owner


def sample_surface(verts, faces, count, rng):
    """(face [count], bary [count,3]): area-weighted random points"""
    a, b, c = (verts[faces[:, k]] for k in range(3))
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    face = rng.choice(len(faces), size=count, p=area / area.sum())
    r = rng.random((count, 2))
    r1 = np.sqrt(r[:, 0])
    return face, np.stack([1 - r1, r1 * (1 - r[:, 1]), r1 * r[:, 1]], 1)


def round_trip_sphere(verts, faces, size, count, seed=0):
    """(texture mean error, vertex-interpolation mean error) of the analytic material at random surface points"""
    a, tex, _ = bake_sphere(verts, faces, size)
    face, bary = sample_surface(verts, faces, count, np.random.default_rng(seed))
    x = (bary[:, :, None] * verts[faces[face]]).sum(1)
    want = sphere_material(project_sphere(x))
    got = sample(a, tex, face, bary)
    per_vertex = sphere_material(verts)
    interp = (bary[:, :, None] * per_vertex[faces[face]]).sum(1)
    return np.abs(got - want).mean(), np.abs(interp - want).mean()
