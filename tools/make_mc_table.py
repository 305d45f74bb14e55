"""Generate nefii_amd/csrc/mc_tables.h: the marching-cubes triangle table of csrc/nefii_mcubes.hip.

    python tools/make_mc_table.py            # rewrites the header
    python tools/make_mc_table.py --check    # exit 1 when the committed header differs

The table is derived, not transcribed.  For each of the 256 inside/outside patterns of a cell's corners:
  - every cube face cuts its crossing edges the same way from both cells that share it: each INSIDE corner of the face
    gets a segment between its two face edges.  On an ambiguous face (two diagonal inside corners) the inside corners are
    thus kept apart; the face's own four corners decide, so no crack can open between two cells;
  - the segments form closed loops on the cube's surface (every crossing edge lies on two faces);
  - each loop is wound so that its normal points from the inside corners to the outside ones (towards increasing values)
    and triangulated without a diagonal between two vertices that share a cube face: such a diagonal could be cut by the
    neighbouring cell too, and the mesh edge would then belong to four triangles.
"""
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'nefii_amd', 'csrc', 'mc_tables.h')


def corner_pos(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def edge_corners(e):
    """edge e = axis * 4 + j; j holds the offsets along the two other axes (lower axis in bit 0)"""
    a, j = e >> 2, e & 3
    others = [x for x in range(3) if x != a]
    off = [0, 0, 0]
    off[others[0]], off[others[1]] = j & 1, j >> 1
    c0 = off[0] | off[1] << 1 | off[2] << 2
    return c0, c0 | 1 << a


EDGES = [edge_corners(e) for e in range(12)]


def faces():
    """(corners in cyclic order, edges between consecutive corners) of the six cube faces"""
    out = []
    for f, s in itertools.product(range(3), range(2)):
        u, v = [x for x in range(3) if x != f]
        cyc = []
        for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
            cyc.append((s << f) | (du << u) | (dv << v))
        edges = []
        for i in range(4):
            a, b = cyc[i], cyc[(i + 1) % 4]
            edges.append(next(e for e, (c0, c1) in enumerate(EDGES) if {c0, c1} == {a, b}))
        out.append((cyc, edges))
    return out


FACES = faces()


def share_face(e0, e1):
    return any(e0 in fe and e1 in fe for _, fe in FACES)


def loops(mask):
    inside = [(mask >> c) & 1 for c in range(8)]
    nbr = {}

    def seg(ea, eb):
        nbr.setdefault(ea, []).append(eb)
        nbr.setdefault(eb, []).append(ea)
    for cyc, fe in FACES:
        cross = [e for e in fe if inside[EDGES[e][0]] != inside[EDGES[e][1]]]
        if len(cross) == 2:
            seg(*cross)
        elif len(cross) == 4:                    # ambiguous: each inside corner cut off between its two face edges
            for i in range(4):
                if inside[cyc[i]]:
                    seg(fe[i - 1], fe[i])
    for e, ns in nbr.items():
        assert len(ns) == 2, (mask, e, ns)
    seen, out = set(), []
    for e0 in sorted(nbr):
        if e0 in seen:
            continue
        cyc, prev, cur = [e0], None, e0
        seen.add(e0)
        while True:
            nxt = nbr[cur][0] if nbr[cur][0] != prev else nbr[cur][1]
            if nxt == e0:
                break
            cyc.append(nxt)
            seen.add(nxt)
            prev, cur = cur, nxt
        out.append(orient(cyc, inside))
    return out


def orient(cyc, inside):
    mid = [(corner_pos(EDGES[e][0]) + corner_pos(EDGES[e][1])) / 2 for e in cyc]
    c = sum(mid) / len(mid)
    area = sum(np.cross(mid[i] - c, mid[(i + 1) % len(mid)] - c) for i in range(len(mid)))
    d = np.zeros(3)
    for e in cyc:
        c0, c1 = EDGES[e]
        d += (corner_pos(c1) - corner_pos(c0)) * (1.0 if inside[c0] else -1.0)     # inside -> outside
    assert abs(area @ d) > 1e-9
    return cyc if area @ d > 0 else cyc[::-1]


def triangulate(cyc):
    """triangles of the polygon cyc with no diagonal between two vertices on a common cube face; fans first"""
    k = len(cyc)
    if k == 3:
        return [tuple(cyc)]
    for s in range(k):
        fan = [cyc[(s + i) % k] for i in range(k)]
        if all(not share_face(fan[0], fan[i]) for i in range(2, k - 1)):
            return [(fan[0], fan[i], fan[i + 1]) for i in range(1, k - 1)]

    def rec(poly):
        if len(poly) == 3:
            return [tuple(poly)]
        n = len(poly)
        for i in range(n):
            for j in range(i + 2, n if i else n - 1):
                if share_face(poly[i], poly[j]):
                    continue
                a, b = poly[i:j + 1], poly[j:] + poly[:i + 1]
                ta, tb = rec(a), rec(b)
                if ta is not None and tb is not None:
                    return ta + tb
        return None
    t = rec(cyc)
    assert t is not None, cyc
    return t


def table():
    rows = []
    for mask in range(256):
        tris = [t for cyc in loops(mask) for t in triangulate(cyc)]
        assert len(tris) <= 5, (mask, len(tris))
        rows.append([e for t in tris for e in t] + [-1] * (16 - 3 * len(tris)))
    return rows


def render(rows):
    lines = ['/* mc_tables.h - the marching-cubes triangle table of nefii_mcubes.hip (generated by tools/make_mc_table.py;',
             ' * edit that script, not this file).  tests/mc_ref.py parses the table from here.',
             ' *',
             ' * corner c of a cell at grid point (i, j, k): offsets (c & 1, c >> 1 & 1, c >> 2 & 1) along (x, y, z);',
             ' * bit c of the case index is set when that corner is inside (v < level).',
             ' * edge e = axis * 4 + j runs from the corner with offset 0 along `axis` to the one with offset 1; j holds the',
             ' * offsets along the two other axes, the lower axis in bit 0.  The edge is owned by its lower grid point.',
             ' * Row `case`: up to 5 triangles as edge triples, -1 after the last; triangles wound so that their normals',
             ' * point towards increasing values.  Ambiguous faces keep their inside corners apart, in every cell alike. */',
             '#ifndef NEFII_MC_TABLES_H',
             '#define NEFII_MC_TABLES_H',
             '',
             '#ifndef NEFII_MC_STORAGE',
             '#define NEFII_MC_STORAGE static const',
             '#endif',
             '',
             'NEFII_MC_STORAGE signed char nefii_mc_tri[256][16] = {']
    lines += ['    {%s},' % ', '.join('%d' % v for v in r) for r in rows]
    lines[-1] = lines[-1].rstrip(',')
    lines += ['};', '', 'NEFII_MC_STORAGE unsigned char nefii_mc_ntri[256] = {']
    counts = [sum(1 for v in r if v >= 0) // 3 for r in rows]
    for i in range(0, 256, 32):
        lines.append('    ' + ', '.join(str(c) for c in counts[i:i + 32]) + (',' if i + 32 < 256 else ''))
    lines += ['};', '', '#endif', '']
    return '\n'.join(lines)


if __name__ == '__main__':
    text = render(table())
    if '--check' in sys.argv:
        sys.exit(0 if os.path.exists(OUT) and open(OUT).read() == text else 1)
    with open(OUT, 'w') as f:
        f.write(text)
    print('wrote', OUT)
