"""Binary little-endian PLY for extracted meshes (the reference's surface_<epoch>.ply, written there by trimesh).

write_ply(path, verts, faces, normals=None, vertex_props=None, comments=()) writes
    x y z [nx ny nz] [red green blue (uchar) <float props in the given order>]  per vertex
    list uchar int vertex_indices                                                per face
read_ply(path) -> dict(vertex={name: np.ndarray}, faces [F,3] int64, comments [str]) reads what write_ply writes.
"""
import numpy as np

_NP = {'float': '<f4', 'uchar': 'u1', 'int': '<i4'}


def _np(t):
    if t is None:
        return None
    if hasattr(t, 'detach'):
        t = t.detach().cpu().numpy()
    return np.asarray(t)


def write_ply(path, verts, faces, normals=None, vertex_props=None, comments=()):
    """vertex_props: ordered {name: [V] or [V,1] array}; uint8 arrays become uchar properties, everything else float."""
    v = _np(verts).astype(np.float32).reshape(-1, 3)
    f = _np(faces).astype(np.int64).reshape(-1, 3)
    n = v.shape[0]
    if f.size and (f.min() < 0 or f.max() >= n):
        raise ValueError('face indices out of range')
    cols = [('x', 'float', v[:, 0]), ('y', 'float', v[:, 1]), ('z', 'float', v[:, 2])]
    if normals is not None:
        nr = _np(normals).astype(np.float32).reshape(-1, 3)
        cols += [('nx', 'float', nr[:, 0]), ('ny', 'float', nr[:, 1]), ('nz', 'float', nr[:, 2])]
    for name, a in (vertex_props or {}).items():
        a = _np(a).reshape(n)
        cols.append((name, 'uchar' if a.dtype == np.uint8 else 'float', a))
    dt = np.dtype([(name, _NP[ty]) for name, ty, _ in cols])
    rec = np.empty(n, dtype=dt)
    for name, _, a in cols:
        rec[name] = a
    frec = np.empty(f.shape[0], dtype=np.dtype([('n', 'u1'), ('i', '<i4', (3,))]))
    frec['n'] = 3
    frec['i'] = f.astype(np.int32)
    head = ['ply', 'format binary_little_endian 1.0']
    head += ['comment ' + str(c).replace('\n', ' ') for c in comments]
    head += ['element vertex %d' % n] + ['property %s %s' % (ty, name) for name, ty, _ in cols]
    head += ['element face %d' % f.shape[0], 'property list uchar int vertex_indices', 'end_header']
    with open(path, 'wb') as fh:
        fh.write(('\n'.join(head) + '\n').encode('ascii'))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())


def read_ply(path):
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    lines = data[:end].decode('ascii').splitlines()
    if lines[0] != 'ply' or lines[1] != 'format binary_little_endian 1.0':
        raise ValueError('not a binary little-endian PLY')
    comments, props, counts, elem = [], {}, {}, None
    for ln in lines[2:]:
        w = ln.split()
        if w[0] == 'comment':
            comments.append(ln[len('comment '):])
        elif w[0] == 'element':
            elem = w[1]
            counts[elem] = int(w[2])
            props[elem] = []
        elif w[0] == 'property':
            if w[1] == 'list':
                if (w[2], w[3]) != ('uchar', 'int'):
                    raise ValueError('face lists must be uchar / int')
                props[elem].append(('list', w[4]))
            else:
                props[elem].append((w[1], w[2]))
    vdt = np.dtype([(name, _NP[ty]) for ty, name in props['vertex']])
    nv = counts['vertex']
    vert = np.frombuffer(data, dtype=vdt, count=nv, offset=end)
    off = end + nv * vdt.itemsize
    nf = counts.get('face', 0)
    frec = np.frombuffer(data, dtype=np.dtype([('n', 'u1'), ('i', '<i4', (3,))]), count=nf, offset=off)
    if nf and not (frec['n'] == 3).all():
        raise ValueError('only triangles are read')
    return {'vertex': {name: np.array(vert[name]) for _, name in props['vertex']},
            'faces': frec['i'].astype(np.int64).reshape(-1, 3), 'comments': comments}
