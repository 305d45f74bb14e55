"""The ambient-occlusion bake restated in numpy (include/nefii_amd.h states the arithmetic): the uniforms and the
origin lift in fp32, operation for operation as csrc/nefii_texbake.hip has them - the same bits; the directions in fp64 from
those fp32 uniforms, with the frame of csrc/mc_sampling.h's to_world; the accumulate step with its fp32 distance test and its
fp64 bent normal."""
import numpy as np

F32 = np.float32
TINY = 1e-6                                        # mc_sampling.h
MAX_RAYS = 1024


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def brev32(s):
    s = np.asarray(s, dtype=np.uint32)
    out = np.zeros_like(s)
    for b in range(32):
        out |= ((s >> np.uint32(b)) & np.uint32(1)) << np.uint32(31 - b)
    return out


def uniforms(texel, K, seed=0):
    """[K, m, 2] float32: (u0, u1) of sample s of the texels with global indices texel [m]"""
    with np.errstate(over='ignore'):
        g = (np.asarray(texel, dtype=np.int64) & 0xffffffff).astype(np.uint32)
        h0 = lowbias32(g ^ lowbias32(np.uint32(seed)))
        h1 = lowbias32(h0 + np.uint32(0x9e3779b9))
    r0 = (h0 >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
    r1 = (h1 >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
    s = np.arange(K, dtype=np.uint32)
    strat = (s.astype(F32) + F32(0.5)) / F32(K)
    u0 = r0[None, :] + strat[:, None]
    u0 = np.where(u0 >= F32(1), u0 - F32(1), u0)
    u0 = np.minimum(u0, F32(1) - F32(2.0 ** -24))
    u1 = r1[None, :] + (brev32(s).astype(F32) * F32(2.0 ** -32))[:, None]
    u1 = np.where(u1 >= F32(1), u1 - F32(1), u1)
    assert u0.dtype == F32 and u1.dtype == F32
    return np.stack([u0, u1], 2)


def _to_world(l, n):
    """to_world of mc_sampling.h in fp64: l, n [..., 3]; the branch is taken on the fp32 normal"""
    up = np.where((n[..., :1].astype(F32) > F32(0.9)), np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]))
    t = np.cross(up, n)
    t = t / (np.sqrt((t * t).sum(-1, keepdims=True)) + TINY)
    s = np.cross(t, n)
    return l[..., 0:1] * t + l[..., 1:2] * s + l[..., 2:3] * n


def directions(u, normal):
    """[K, m, 3] float64 from the uniforms u [K, m, 2] (float32, as the kernel has them) and the unit normals [m, 3] (float32)"""
    u0, u1 = u[..., 0].astype(np.float64), u[..., 1].astype(np.float64)
    n = np.asarray(normal, dtype=F32).astype(np.float64)[None]
    phi = 2.0 * np.pi * u1
    r, lz = np.sqrt(u0), np.sqrt(1.0 - u0)
    flip = np.asarray(normal, dtype=F32)[None, :, 0:1] < F32(-0.9)
    l = np.stack([r * np.cos(phi), r * np.sin(phi), lz], -1)
    l = np.where(flip, l * np.array([1.0, 1.0, -1.0]), l)
    w = _to_world(l, np.broadcast_to(np.where(flip, -n, n), l.shape))
    return w / np.sqrt((w * w).sum(-1, keepdims=True))


def origins(pos, normal, sdf, gnorm, bias=0.0):
    """[m, 3] float32, the kernel's bits: fl(x + fl(t n)), t = fl(bias - fl(sdf / gnorm))"""
    pos, normal = np.asarray(pos, dtype=F32), np.asarray(normal, dtype=F32)
    t = F32(bias) - np.asarray(sdf, dtype=F32) / np.asarray(gnorm, dtype=F32)
    return pos + t[:, None] * normal


def accumulate(hit, hit_pts, orig, dirs, normal, distance=0.0):
    """(ao [m] float32, bent [m, 3] float64, occluded [K, m] bool)"""
    hit = np.asarray(hit) != 0
    K = hit.shape[0]
    d = np.asarray(hit_pts, dtype=F32) - np.asarray(orig, dtype=F32)[None]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == F32
    dist = F32(distance)
    with np.errstate(invalid='ignore'):               # the point of a miss may hold anything
        occluded = hit & (True if dist <= 0 else d2 <= dist * dist)
    ao = (K - occluded.sum(0)).astype(F32) / F32(K)
    b = np.zeros((hit.shape[1], 3))
    for s in range(K):                               # in order of s
        b += np.where(occluded[s][:, None], 0.0, np.asarray(dirs[s], dtype=F32).astype(np.float64))
    length = np.sqrt((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
    none = occluded.all(0) | ~(length > 0)
    bent = np.where(none[:, None], np.asarray(normal, dtype=F32).astype(np.float64), b / np.where(none, 1.0, length)[:, None])
    return ao, bent, occluded


def unit_normals(m, rng):
    """[m, 3] float32 random unit normals; the first ones cover every branch of the frame: (1, 0, 0), (0.95, ..), (-1, 0, 0),
    (-0.95, ..) and both sides of the 0.9 thresholds"""
    n = rng.normal(size=(m, 3))
    fixed = [[1, 0, 0], [0.95, 0.2, -0.24], [-1, 0, 0], [-0.95, -0.2, 0.24], [0.899, 0.3, 0.32], [-0.899, 0.3, 0.32],
             [0, 1, 0], [0, 0, -1]]
    k = min(m, len(fixed))
    n[:k] = fixed[:k]
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
