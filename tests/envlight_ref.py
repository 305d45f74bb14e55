"""fp64 numpy oracle of the lat-long map light (csrc/nefii_envlight.hip): both axis mappings, the CDF
build, continuous sampling, the pdf, nearest-texel radiance, and the exact integral of L(w) f_r(w) cos over the sphere
with nefii_mc_shade's BRDF (supersampled sub-texels: L is piecewise constant, the BRDF is smooth inside a texel)."""
import numpy as np

TINY = 1e-6
COORDS = ('mitsuba', 'blender')


def direction(u, v, coord):
    """unit direction of map coordinates (u, v) in [0, 1]^2, [..., 3]"""
    phi = np.pi * np.asarray(v, np.float64)
    u = np.asarray(u, np.float64)
    if coord == 'mitsuba':
        th = 2. * np.pi * u - 0.5 * np.pi
        return np.stack([np.cos(th) * np.sin(phi), np.cos(phi), np.sin(th) * np.sin(phi)], -1)
    th = np.pi - 2. * np.pi * u
    return np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], -1)


def texel_centres(H, W, coord):
    v, u = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing='ij')
    return direction(u, v, coord)


def map_coords(d, coord):
    """(u, v, sin phi) of directions d [..., 3] (normalised first, norm clamped at 1e-8)"""
    d = np.asarray(d, np.float64)
    d = d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-8)
    if coord == 'mitsuba':
        x, up, side = d[..., 0], d[..., 1], d[..., 2]
    else:
        x, side, up = d[..., 0], d[..., 1], d[..., 2]
    phi = np.arccos(np.clip(up, -1., 1.))
    th = np.arctan2(side, x)
    if coord == 'mitsuba':
        u = (th + 0.5 * np.pi) / (2. * np.pi)
        u = u - np.floor(u)
    else:
        u = (np.pi - th) / (2. * np.pi)
    rho = np.sqrt(x * x + side * side)
    return u, phi / np.pi, np.where(rho > 0, rho / np.maximum(np.sqrt(rho * rho + up * up), 1e-300), 0.)


def texel_of(d, H, W, coord):
    """(i, j, sin phi) of directions d"""
    u, v, s = map_coords(d, coord)
    i = np.clip(np.floor(v * H), 0, H - 1).astype(np.int64)
    j = np.clip(np.floor(u * W), 0, W - 1).astype(np.int64)
    return i, j, s


def edge_distance(d, H, W, coord):
    """angular distance (rad, lower bound) of d from the nearest texel edge"""
    u, v, s = map_coords(d, coord)
    dv = np.abs(v * H - np.round(v * H)) / H * np.pi
    du = np.abs(u * W - np.round(u * W)) / W * 2. * np.pi * s
    return np.minimum(dv, du)


def distribution(envmap):
    """f(i, j) = max(mean rgb, 0) * sin(pi (i + 0.5) / H), fp64 [H, W]"""
    m = np.asarray(envmap, np.float64).mean(-1)
    H = m.shape[0]
    return np.maximum(m, 0.) * np.sin(np.pi * (np.arange(H) + 0.5) / H)[:, None]


def _cdf(x):
    tot = x.sum()
    n = x.shape[-1]
    if not tot > 0:
        c = (np.arange(n) + 1.) / n
    else:
        c = np.cumsum(x) / tot
    c[-1] = 1.
    return c


def build(envmap):
    """(M [H], C [H, W]) in fp64: the marginal and the conditional CDFs, each ending in exactly 1 (uniform for a zero
    row / an all-zero map).  np.float32 of them is what the kernel stores (to rounding of the sums' order)."""
    f = distribution(envmap)
    C = np.stack([_cdf(row) for row in f])
    M = _cdf(f.sum(1))
    return M, C


def texel_prob(M, C, i, j):
    M = np.asarray(M, np.float64)
    C = np.asarray(C, np.float64)
    Mp = np.where(i > 0, M[np.maximum(i - 1, 0)], 0.)
    Cp = np.where(j > 0, C[i, np.maximum(j - 1, 0)], 0.)
    return (M[i] - Mp) * (C[i, j] - Cp)


def solid_angle_pdf(P, H, W, sin_phi):
    return np.where(sin_phi > 0, P * H * W / (2. * np.pi ** 2 * np.where(sin_phi > 0, sin_phi, 1.)), 0.)


def pdf(M, C, coord, d):
    """solid-angle pdf of the map sampler along d [..., 3] on the table (M, C) - fp64, or the stored fp32 floats"""
    H, W = np.shape(C)
    i, j, s = texel_of(d, H, W, coord)
    return solid_angle_pdf(texel_prob(M, C, i, j), H, W, s)


def radiance(envmap, coord, d):
    H, W = envmap.shape[:2]
    i, j, _ = texel_of(d, H, W, coord)
    return envmap[i, j]


def _search(cdf, x):
    """first k with cdf[k] > x (last if none), and the continuous offset in it (clamped to [0, 1 - 2^-24])"""
    cdf = np.asarray(cdf, np.float64)
    k = np.minimum(np.searchsorted(cdf, x, side='right'), cdf.shape[-1] - 1)
    return k


def sample(M, C, coord, u_row, u_col):
    """continuous inversion (PBRT SampleContinuous) -> (i, j, d [n, 3], own pdf [n]); M, C as stored"""
    M = np.asarray(M, np.float64)
    C = np.asarray(C, np.float64)
    H, W = C.shape
    u_row = np.asarray(u_row, np.float64)
    u_col = np.asarray(u_col, np.float64)
    dmax = 1. - 2. ** -24
    i = _search(M, u_row)
    Mp = np.where(i > 0, M[np.maximum(i - 1, 0)], 0.)
    w = M[i] - Mp
    dv = np.clip(np.where(w > 0, (u_row - Mp) / np.where(w > 0, w, 1.), 0.), 0., dmax)
    Ci = C[i]
    j = np.array([min(np.searchsorted(Ci[k], u_col[k], side='right'), W - 1) for k in range(len(i))], np.int64)
    Cp = np.where(j > 0, Ci[np.arange(len(i)), np.maximum(j - 1, 0)], 0.)
    w = Ci[np.arange(len(i)), j] - Cp
    du = np.clip(np.where(w > 0, (u_col - Cp) / np.where(w > 0, w, 1.), 0.), 0., dmax)
    v = (i + dv) / H
    u = (j + du) / W
    d = direction(u, v, coord)
    return i, j, d, solid_angle_pdf(texel_prob(M, C, i, j), H, W, np.sin(np.pi * v))


# ---- nefii_mc_shade's BRDF and the exact integral --------------------------------------------------------------------
def brdf_cos(n, v, wi, rough, albedo, spec):
    """(specular, diffuse) f_r * cos of nefii_mc_shade (GGX D, Schlick 2^(-(5.55473 vh + 6.8316) vh), Smith-Schlick G,
    Lambert, the kernel's clamps) for directions wi [..., 3]; each [..., 3]"""
    h = wi + v
    h = h / (np.linalg.norm(h, axis=-1, keepdims=True) + TINY)
    nh = np.maximum(h @ n, 0.)
    vh = np.maximum(h @ v, 0.)
    P = 2. ** (-(5.55473 * vh + 6.8316) * vh)
    d1 = max(float(v @ n), 0.)
    d2 = np.maximum(wi @ n, 0.)
    den = 4. * d1 * d2 + TINY
    a4 = rough ** 4
    root = nh * nh + (1. - nh * nh) / a4
    D = 1. / (np.pi * a4 * root * root)
    k = (rough + 1.) ** 2 / 8.
    G = (d1 / (d1 * (1. - k) + k + TINY)) * (d2 / (d2 * (1. - k) + k + TINY))
    F = spec[None, :] + (1. - spec[None, :]) * P[:, None]
    cosn = np.maximum(wi @ n, 0.)
    s = F * (D * G / den * cosn)[:, None]
    dif = np.broadcast_to(albedo[None, :] / np.pi, s.shape) * cosn[:, None]
    return s, dif


def integral(envmap, coord, n, v, rough, albedo, spec, sub=8, fine=None, fine_angle=0.5):
    """(specular, diffuse) of integral L(w) f_r(w) cos dw over the sphere: every texel split into sub x sub cells
    (midpoint rule in (u, v), dw = 2 pi^2 sin(phi) du dv); texels within fine_angle of the mirror direction into
    fine x fine cells"""
    envmap = np.asarray(envmap, np.float64)
    H, W = envmap.shape[:2]
    n = np.asarray(n, np.float64)
    v = np.asarray(v, np.float64)
    albedo = np.asarray(albedo, np.float64)
    spec = np.asarray(spec, np.float64)
    refl = 2. * (n @ v) * n - v
    centres = texel_centres(H, W, coord).reshape(-1, 3)
    near = np.arccos(np.clip(centres @ refl, -1., 1.)) < fine_angle
    s_acc = np.zeros(3)
    d_acc = np.zeros(3)
    L = envmap.reshape(-1, 3)
    for mask, k in ((~near, sub), (near, fine or sub)):
        idx = np.nonzero(mask)[0]
        if idx.size == 0:
            continue
        off = (np.arange(k) + 0.5) / k
        ov, ou = np.meshgrid(off, off, indexing='ij')
        ov, ou = ov.reshape(-1), ou.reshape(-1)
        for c0 in range(0, idx.size, max(1, 400000 // (k * k))):
            t = idx[c0:c0 + max(1, 400000 // (k * k))]
            ti, tj = t // W, t % W
            vv = (ti[:, None] + ov[None, :]) / H
            uu = (tj[:, None] + ou[None, :]) / W
            d = direction(uu, vv, coord).reshape(-1, 3)
            dw = (2. * np.pi ** 2 / (H * W * k * k)) * np.sin(np.pi * vv).reshape(-1)
            s, dif = brdf_cos(n, v, d, rough, albedo, spec)
            Lt = np.repeat(L[t], k * k, axis=0)
            s_acc += (Lt * s * dw[:, None]).sum(0)
            d_acc += (Lt * dif * dw[:, None]).sum(0)
    return s_acc, d_acc
