"""NumPy restatement of the brick classification of sparse mesh export (include/nefii_amd.h: nefii_mcubes_classify_bricks;
DESIGN.md 6f "Sparse export"), operation for operation, so that the kernel can be held against it bit for bit; and the
helpers the sparse-export tests share."""
import numpy as np


def unpack_cells(cells):
    """(lo, hi) float32 [G,G,G] of the interval-grid words: fp16 lo in the low half, fp16 hi in the high half"""
    w = np.ascontiguousarray(cells).view(np.uint32)
    lo = (w & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32)
    hi = (w >> 16).astype(np.uint16).view(np.float16).astype(np.float32)
    return lo, hi


def pack_cells(lo, hi):
    """int32 words of lo rounded DOWN and hi rounded UP to fp16 (non-finite values pass as they are)"""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        l16, h16 = lo.astype(np.float16), hi.astype(np.float16)
        l16 = np.where(l16.astype(np.float32) > lo, np.nextafter(l16, np.float16(-np.inf)), l16).astype(np.float16)
        h16 = np.where(h16.astype(np.float32) < hi, np.nextafter(h16, np.float16(np.inf)), h16).astype(np.float16)
    return (l16.view(np.uint16).astype(np.uint32) | (h16.view(np.uint16).astype(np.uint32) << 16)).view(np.int32)


def brick_counts(shape, brick):
    return tuple((n - 2) // brick + 1 for n in shape)


def classify_bricks(cells, radius, shape, p0, steps, level, brick=8):
    """uint8 [bx,by,bz]: 0 only where the intervals of every cell the brick's widened box overlaps exclude the level"""
    G = cells.shape[0]
    lo, hi = unpack_cells(cells)
    bad = ~np.isfinite(lo) | ~np.isfinite(hi)
    R = np.float32(radius)
    inv_h = np.float32(G / (2.0 * float(R)))
    level = np.float32(level)
    p0 = np.asarray(p0, np.float64)
    s = np.asarray(steps, np.float64)
    nb = brick_counts(shape, brick)
    out = np.ones(nb, np.uint8)
    for i in range(nb[0]):
        for j in range(nb[1]):
            for k in range(nb[2]):
                first = [i * brick, j * brick, k * brick]
                last = [min(first[a] + brick, shape[a] - 1) for a in range(3)]
                pts = []
                for c in range(8):
                    di = float(last[0] if c & 1 else first[0])
                    dj = float(last[1] if c & 2 else first[1])
                    dk = float(last[2] if c & 4 else first[2])
                    pts.append((((p0 + di * s[0]) + dj * s[1]) + dk * s[2]).astype(np.float32))
                pts = np.stack(pts)
                blo, bhi = pts.min(0), pts.max(0)
                m = np.abs(pts).max()
                u = np.nextafter(m, np.float32(np.inf)) - m
                blo, bhi = (blo - u).astype(np.float32), (bhi + u).astype(np.float32)
                if not (np.all(blo >= -R) and np.all(bhi <= R)):
                    continue
                c0 = np.clip(((blo + R) * inv_h).astype(np.int64), 0, G - 1)
                c1 = np.clip(((bhi + R) * inv_h).astype(np.int64), 0, G - 1)
                sl = tuple(slice(int(c0[a]), int(c1[a]) + 1) for a in range(3))
                if bad[sl].any():
                    continue
                if lo[sl].min() > level or hi[sl].max() < level:
                    out[i, j, k] = 0
    return out


def crossing_bricks(vol, level, brick):
    """uint8 [bx,by,bz]: the bricks that hold a cell whose 8 corners are not all on one side (inside: v < level)"""
    ins = np.asarray(vol) < np.float32(level)
    nx, ny, nz = ins.shape
    n_in = np.zeros((nx - 1, ny - 1, nz - 1), np.int32)
    for c in range(8):
        n_in += ins[(c & 1):nx - 1 + (c & 1), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1), (c >> 2):nz - 1 + (c >> 2)]
    cross = (n_in > 0) & (n_in < 8)
    nb = brick_counts(ins.shape, brick)
    pad = np.zeros(tuple(b * brick for b in nb), bool)
    pad[:nx - 1, :ny - 1, :nz - 1] = cross
    return pad.reshape(nb[0], brick, nb[1], brick, nb[2], brick).any(axis=(1, 3, 5)).astype(np.uint8)


def rotation(axis, angle):
    """[3,3] float64 rotation about `axis` by `angle` (Rodrigues)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
