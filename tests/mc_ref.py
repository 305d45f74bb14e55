"""numpy marching cubes with exactly the conventions of csrc/nefii_mcubes.hip (the oracle of the mesh tests).

The triangle table is parsed from nefii_amd/csrc/mc_tables.h, the one copy the kernels compile.  Inside: v < level.
Vertices: one per crossing grid edge, numbered by (owner grid point's linear index, axis x < y < z), at
origin + (p0 + t (p1 - p0)) * spacing with t = (level - v0) / (v1 - v0), all in float32.  Faces: by cell linear index, then
table order."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'nefii_amd', 'csrc', 'mc_tables.h')


def load_table():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = re.search(r'nefii_mc_tri\s*\[256\]\s*\[16\]\s*=\s*\{(.*?)\};', src, re.S).group(1)
    tri = np.array([int(v) for v in re.findall(r'-?\d+', body)], dtype=np.int64).reshape(256, 16)
    body = re.search(r'nefii_mc_ntri\s*\[256\]\s*=\s*\{(.*?)\};', src, re.S).group(1)
    ntri = np.array([int(v) for v in re.findall(r'\d+', body)], dtype=np.int64)
    assert ntri.shape == (256,) and ((tri >= 0).sum(1) == 3 * ntri).all()
    return tri, ntri


TRI, NTRI = load_table()


def edge_offsets():
    """edge e -> (corner offset (ox, oy, oz) of its lower end, axis)"""
    out = []
    for e in range(12):
        a, j = e >> 2, e & 3
        others = [x for x in range(3) if x != a]
        off = [0, 0, 0]
        off[others[0]], off[others[1]] = j & 1, j >> 1
        out.append((tuple(off), a))
    return out


EDGE = edge_offsets()


def marching_cubes(vol, level=0.0, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0)):
    """-> (verts [V,3] float32, faces [F,3] int64)"""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    nx, ny, nz = vol.shape
    lev = np.float32(level)
    inside = vol < lev
    cross = np.zeros(vol.shape + (3,), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(-1)
    vid = np.cumsum(flat) - 1
    sel = np.nonzero(flat)[0]
    p, a = sel // 3, sel % 3
    ix, iy, iz = p // (ny * nz), (p // nz) % ny, p % nz
    strides = np.array([ny * nz, nz, 1])
    v0 = vol.reshape(-1)[p]
    v1 = vol.reshape(-1)[p + strides[a]]
    t = (lev - v0) / (v1 - v0)
    idx = np.stack([ix, iy, iz], 1).astype(np.float32)
    idx[np.arange(len(p)), a] += t
    verts = (np.asarray(origin, np.float32)[None] + idx * np.asarray(spacing, np.float32)[None]).astype(np.float32)

    cube = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        ox, oy, oz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        cube |= inside[ox:nx - 1 + ox, oy:ny - 1 + oy, oz:nz - 1 + oz].astype(np.int64) << c
    cube = cube.reshape(-1)
    cells = np.nonzero(NTRI[cube] > 0)[0]
    cx, cy, cz = cells // ((ny - 1) * (nz - 1)), (cells // (nz - 1)) % (ny - 1), cells % (nz - 1)
    rows = TRI[cube[cells]]                                         # [C, 16]
    ids = np.full(rows.shape, -1, dtype=np.int64)
    for e, ((ox, oy, oz), a) in enumerate(EDGE):
        m = rows == e
        if not m.any():
            continue
        q = ((cx + ox) * ny + (cy + oy)) * nz + (cz + oz)
        ids[m] = vid[(q * 3 + a)[:, None].repeat(16, 1)[m]]
    faces = ids[rows >= 0].reshape(-1, 3)
    return verts, faces


# ---- mesh checks --------------------------------------------------------------------------------
def edge_use(faces):
    """-> (undirected edge counts, directed edge counts) as dicts keyed by vertex pairs"""
    f = np.asarray(faces, dtype=np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    und = np.sort(d, 1)
    _, cu = np.unique(und, axis=0, return_counts=True)
    _, cd = np.unique(d, axis=0, return_counts=True)
    return cu, cd


def is_closed_oriented(faces):
    """every edge in exactly two triangles, used once in each direction"""
    if len(faces) == 0:
        return True
    cu, cd = edge_use(faces)
    return bool((cu == 2).all() and (cd == 1).all())


def euler(verts, faces):
    f = np.asarray(faces, dtype=np.int64)
    used = np.unique(f)
    und = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0), 1), axis=0)
    return len(used) - len(und) + len(f)


def area_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()
    vol = (a * np.cross(b, c)).sum() / 6.0
    return area, vol
