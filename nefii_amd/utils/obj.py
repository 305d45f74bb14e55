"""Wavefront OBJ + MTL for textured meshes (what Blender, three.js and Unreal import; the PLY of utils/ply.py carries
the per-vertex properties).

write_obj(path, verts, faces, normals, corner_uv, mtl_name) writes
    mtllib <mtl_name>, v x y z per vertex, vn x y z per vertex, vt u v per face corner (3 F of them, corner 3 f + k),
    usemtl <material>, f a/t/a b/t/b c/t/c per face
write_mtl(path, specular, map_kd, map_pr, norm, ao=None) writes one material: Kd 1 1 1, map_Kd, Ks, map_Pr, norm and, with
    ao, map_Ka: the ambient-occlusion map.
read_obj(path) -> dict(verts, normals, uv, faces, face_uv, face_normals, mtllib, usemtl) reads what write_obj writes;
read_mtl(path) -> {key: value string} of the first material.

Every array is formatted by one % operation over the whole of it: no Python loop per face.  float32 inputs are written with 9
significant digits and float64 texture coordinates with 17, so that reading gives back the same bits.
"""
import numpy as np

MATERIAL = 'baked'


def _np(t):
    if hasattr(t, 'detach'):
        t = t.detach().cpu().numpy()
    return np.asarray(t)


def _rows(fmt, a):
    """fmt applied to every row of a [N, k], as one string"""
    return (fmt * a.shape[0]) % tuple(a.reshape(-1).tolist())


def write_obj(path, verts, faces, normals, corner_uv, mtl_name, material=MATERIAL):
    """verts, normals [V,3], faces [F,3] (0-based), corner_uv [F,3,2] (OBJ convention: v up), mtl_name: the material file's
    name as the OBJ refers to it.  ValueError for shapes that do not match and indices out of range."""
    v = _np(verts).astype(np.float32).reshape(-1, 3)
    n = _np(normals).astype(np.float32).reshape(-1, 3)
    f = _np(faces).astype(np.int64).reshape(-1, 3)
    uv = _np(corner_uv).astype(np.float64)
    if n.shape != v.shape:
        raise ValueError('one normal per vertex is needed: %d vertices, %d normals' % (v.shape[0], n.shape[0]))
    if uv.shape != (f.shape[0], 3, 2):
        raise ValueError('corner_uv must be [F, 3, 2] = %s, got %s' % ((f.shape[0], 3, 2), uv.shape))
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError('face indices out of range')
    t = 3 * np.arange(f.shape[0], dtype=np.int64)[:, None] + np.arange(3, dtype=np.int64)[None, :]
    fi = np.stack([f + 1, t + 1, f + 1], 2)                                 # [F, 3 corners, (v, vt, vn)], 1-based
    with open(path, 'w') as fh:
        fh.write('# nefii_amd textured mesh: %d vertices, %d faces\nmtllib %s\n' % (v.shape[0], f.shape[0], mtl_name))
        fh.write(_rows('v %.9g %.9g %.9g\n', v.astype(np.float64)))
        fh.write(_rows('vn %.9g %.9g %.9g\n', n.astype(np.float64)))
        fh.write(_rows('vt %.17g %.17g\n', uv.reshape(-1, 2)))
        fh.write('usemtl %s\n' % material)
        fh.write(_rows('f %d/%d/%d %d/%d/%d %d/%d/%d\n', fi.reshape(-1, 9)))


def write_mtl(path, specular, map_kd, map_pr, norm, material=MATERIAL, ao=None):
    """One material: white Kd under the albedo map, the global specular reflection as Ks, the roughness map (map_Pr, the PBR
    extension of the format) and the normal map (norm), which is in OBJECT space.  ao: the file name of an ambient-occlusion
    map, written as map_Ka (the slot importers read occlusion from); without it the file is what it was."""
    s = [float(x) for x in _np(specular).reshape(-1)]
    if len(s) != 3:
        raise ValueError('specular must hold 3 values, got %d' % len(s))
    with open(path, 'w') as fh:
        fh.write('# nefii_amd baked materials\n# the normal map (norm) is in OBJECT space, not tangent space\n')
        fh.write('newmtl %s\nKd 1 1 1\nmap_Kd %s\nKs %.9g %.9g %.9g\nmap_Pr %s\nnorm %s\n' % (
            material, map_kd, s[0], s[1], s[2], map_pr, norm))
        if ao is not None:
            fh.write('# map_Ka holds baked AMBIENT OCCLUSION (linear, 1 = open), not an ambient colour\nmap_Ka %s\n' % ao)


def _table(lines, cols, dtype):
    if not lines:
        return np.zeros((0, cols), dtype=dtype)
    return np.array(' '.join(lines).split(), dtype=dtype).reshape(-1, cols)


def read_obj(path):
    with open(path) as fh:
        rows = [ln.split(None, 1) for ln in fh.read().splitlines() if ln and not ln.startswith('#')]
    by = {}
    for r in rows:
        by.setdefault(r[0], []).append(r[1] if len(r) > 1 else '')
    f = _table([ln.replace('/', ' ') for ln in by.get('f', [])], 9, np.int64).reshape(-1, 3, 3) - 1
    return {'verts': _table(by.get('v', []), 3, np.float64).astype(np.float32),
            'normals': _table(by.get('vn', []), 3, np.float64).astype(np.float32),
            'uv': _table(by.get('vt', []), 2, np.float64),
            'faces': f[:, :, 0], 'face_uv': f[:, :, 1], 'face_normals': f[:, :, 2],
            'mtllib': (by.get('mtllib') or [None])[0], 'usemtl': (by.get('usemtl') or [None])[0]}


def read_mtl(path):
    out = {}
    with open(path) as fh:
        for ln in fh.read().splitlines():
            if ln and not ln.startswith('#'):
                k, _, val = ln.partition(' ')
                out.setdefault(k, val)
    return out
