"""The irradiance bake restated in numpy (include/nefii_amd.h states the arithmetic): the uniforms of both
techniques in fp32, operation for operation as csrc/nefii_texbake.hip has them - the same bits; the inversion of the stored
fp32 CDFs (the sampled texel exactly, the continuous offsets in fp64); the directions and the balance-heuristic weights in fp64;
the accumulate step in fp64 in the kernel's order; and exact_irradiance, the integral the estimator estimates, by sub-sampling
every texel of the map.  The cosine rows are tests/texbake_ao_ref.py's, the map's coordinates tests/envlight_ref.py's."""
import numpy as np

import envlight_ref as env
import texbake_ao_ref as ao

F32 = np.float32
COORDS = env.COORDS
DV_MAX = 1.0 - 2.0 ** -24


def uniforms(texel, K_cos, K_map, seed=0):
    """[K_cos + K_map, m, 2] float32, the kernel's bits: rows s < K_cos are texbake_ao_ref.uniforms(texel, K_cos, seed); the
    others the same sequence over K_map on the offsets r2, r3 of h2 = lowbias32(h1 + 0x9e3779b9), h3 = lowbias32(h2 + ..)"""
    rows = []
    if K_cos:
        rows.append(ao.uniforms(texel, K_cos, seed))
    if K_map:
        with np.errstate(over='ignore'):
            g = (np.asarray(texel, dtype=np.int64) & 0xffffffff).astype(np.uint32)
            h0 = ao.lowbias32(g ^ ao.lowbias32(np.uint32(seed)))
            h1 = ao.lowbias32(h0 + np.uint32(0x9e3779b9))
            h2 = ao.lowbias32(h1 + np.uint32(0x9e3779b9))
            h3 = ao.lowbias32(h2 + np.uint32(0x9e3779b9))
        r2 = (h2 >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
        r3 = (h3 >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
        s = np.arange(K_map, dtype=np.uint32)
        u0 = r2[None, :] + ((s.astype(F32) + F32(0.5)) / F32(K_map))[:, None]
        u0 = np.where(u0 >= F32(1), u0 - F32(1), u0)
        u0 = np.minimum(u0, F32(1) - F32(2.0 ** -24))
        u1 = r3[None, :] + (ao.brev32(s).astype(F32) * F32(2.0 ** -32))[:, None]
        u1 = np.where(u1 >= F32(1), u1 - F32(1), u1)
        assert u0.dtype == F32 and u1.dtype == F32
        rows.append(np.stack([u0, u1], 2))
    return np.concatenate(rows, 0)


def stored_table(envmap):
    """(M [H], C [H, W]) float32: envlight_ref.build rounded as the kernel stores it (the GPU tests read the kernel's own
    table instead: its sums run in another order)"""
    M, C = env.build(envmap)
    return M.astype(F32), C.astype(F32)


def _invert(cdf, x):
    """(k, offset): the first k with cdf[k] > x (the last if none) of the stored fp32 cdf [..., n] per x [...] (fp32) - exact -
    and the continuous offset inside it in fp64, clamped to [0, 1 - 2^-24]"""
    n = cdf.shape[-1]
    k = np.minimum((cdf <= x[..., None]).sum(-1), n - 1)            # a CDF is sorted: the count of entries <= x
    c = cdf.astype(np.float64)
    hi = np.take_along_axis(c, k[..., None], -1)[..., 0]
    lo = np.where(k > 0, np.take_along_axis(c, np.maximum(k - 1, 0)[..., None], -1)[..., 0], 0.0)
    w = hi - lo
    d = np.where(w > 0, (x.astype(np.float64) - lo) / np.where(w > 0, w, 1.0), 0.0)
    return k, np.clip(d, 0.0, DV_MAX)


def sample_map(u, M32, C32):
    """(i, j, v, uu) of the map rows' uniforms u [..., 2] float32: the row by the marginal, the column by that row's
    conditional, v = (i + dv) / H, uu = (j + du) / W in fp64"""
    H, W = C32.shape
    i, dv = _invert(np.broadcast_to(M32, u.shape[:-1] + (H,)), u[..., 0])
    j, du = _invert(C32[i], u[..., 1])
    return i, j, (i + dv) / H, (j + du) / W


def directions(u, normal, K_cos, M32, C32, coord, R=None):
    """(dirs [K, m, 3] float64, (i, j, v) of the map rows): rows s < K_cos texbake_ao_ref.directions, the others R
    direction(uu, v) of the inverted CDFs; R [3, 3] world-from-light as the kernel has its floats (None: the identity)"""
    rows, picked = [], None
    if K_cos:
        rows.append(ao.directions(u[:K_cos], normal))
    if u.shape[0] > K_cos:
        i, j, v, uu = sample_map(u[K_cos:], M32, C32)
        d = env.direction(uu, v, coord)
        if R is not None:
            d = d @ np.asarray(R, dtype=F32).astype(np.float64).T
        rows.append(d)
        picked = (i, j, v)
    return np.concatenate(rows, 0), picked


def weights(dirs, normal, envmap, M32, C32, coord, K_cos, K_map, picked, R=None):
    """(weight [K, m, 3], c [K, m], sin phi [K, m], i, j [K, m]) in fp64 along the directions dirs [K, m, 3] (the test hands in
    the kernel's own fp32 directions, so that both look up the same point of the map): c = max(n . w, 0), p_map from the stored
    floats - at the texel under R^T w for the cosine rows, at the sampled texel `picked` for the map rows - and weight = L c /
    (K_cos c / pi + K_map p_map), 0 where c = 0 or the denominator is 0"""
    dirs = np.asarray(dirs, dtype=np.float64)
    n = np.asarray(normal, dtype=F32).astype(np.float64)[None]
    H, W = C32.shape
    c = np.maximum((dirs * n).sum(-1), 0.0)
    local = dirs if R is None else dirs @ np.asarray(R, dtype=F32).astype(np.float64)         # R^T w, row vectors
    i, j, sin_phi = env.texel_of(local, H, W, coord)
    if picked is not None:
        i, j, sin_phi = i.copy(), j.copy(), sin_phi.copy()
        i[K_cos:], j[K_cos:], sin_phi[K_cos:] = picked[0], picked[1], np.sin(np.pi * picked[2])
    p = env.solid_angle_pdf(env.texel_prob(M32, C32, i, j), H, W, sin_phi)
    den = K_cos * c / np.pi + K_map * p
    g = np.where((c > 0) & (den > 0), c / np.where(den > 0, den, 1.0), 0.0)
    return np.asarray(envmap, dtype=np.float64)[i, j] * g[..., None], c, sin_phi, i, j


def cos_f32(dirs, normal):
    """n . w as the kernel's fp32 has it: (n.x w.x + n.y w.y) + n.z w.z, every operation rounded - the same bits"""
    d, n = np.asarray(dirs, dtype=F32), np.asarray(normal, dtype=F32)[None]
    c = (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]
    assert c.dtype == F32
    return c


def accumulate(hit, weight, K_cos, K_map):
    """(irradiance [m, 3], noise [m]) float64, unrounded, in the kernel's order: the rows with a non-zero weight and hit == 0
    summed in order of s; per technique S, Q of the luminance y = ((w0 + w1) + w2) / 3, var = sum over the techniques with n >= 2
    of (Q - S S / n) n / (n - 1), noise = sqrt(max(var, 0))"""
    w = np.asarray(weight, dtype=F32).astype(np.float64)
    K, m = w.shape[:2]
    assert K == K_cos + K_map
    counted = (np.asarray(hit) == 0) & (w != 0).any(-1)
    E, var = np.zeros((m, 3)), np.zeros(m)
    start = 0
    for n_t in (K_cos, K_map):
        S, Q = np.zeros(m), np.zeros(m)
        for s in range(start, start + n_t):
            E += np.where(counted[s][:, None], w[s], 0.0)
            y = np.where(counted[s], ((w[s, :, 0] + w[s, :, 1]) + w[s, :, 2]) / 3.0, 0.0)
            S += y
            Q += y * y
        start += n_t
        if n_t >= 2:
            var += (Q - S * S / n_t) * (n_t / (n_t - 1))
    return E, np.sqrt(np.maximum(var, 0.0))


def estimate(envmap, normal, texel, K_cos, K_map, coord, seed=0, R=None):
    """[m, 3] float64: the reference estimator without occluders - the sum of the weights of every row"""
    M32, C32 = stored_table(envmap)
    u = uniforms(texel, K_cos, K_map, seed)
    d, picked = directions(u, normal, K_cos, M32, C32, coord, R)
    return weights(d, normal, envmap, M32, C32, coord, K_cos, K_map, picked, R)[0].sum(0)


def exact_irradiance(envmap, normals, R=None, coord='mitsuba', sub=32):
    """[m, 3] float64: the integral of L(R^T w) max(n . w, 0) dw over the sphere at the unit normals [m, 3] - every texel with
    light in it split into sub x sub cells (midpoint rule in (u, v), dw = 2 pi^2 sin(pi v) du dv); L is constant inside a texel
    and the cosine smooth, so the rule's error falls with 1 / sub^2"""
    assert sub >= 32
    envmap = np.asarray(envmap, dtype=np.float64)
    H, W = envmap.shape[:2]
    n = np.asarray(normals, dtype=np.float64)
    off = (np.arange(sub) + 0.5) / sub
    ov, ou = (a.reshape(-1) for a in np.meshgrid(off, off, indexing='ij'))
    E = np.zeros((n.shape[0], 3))
    for i, j in zip(*np.nonzero(envmap.any(-1))):
        v, u = (i + ov) / H, (j + ou) / W
        d = env.direction(u, v, coord)
        if R is not None:
            d = d @ np.asarray(R, dtype=np.float64).T
        dw = (2.0 * np.pi ** 2 / (H * W * sub * sub)) * np.sin(np.pi * v)
        E += (np.maximum(n @ d.T, 0.0) @ dw)[:, None] * envmap[i, j][None]
    return E


def sun_map(H, W, i, j, value=1000.0):
    """[H, W, 3] float32: one texel at `value`, the rest 0"""
    m = np.zeros((H, W, 3), dtype=F32)
    m[i, j] = value
    return m


def sun_direction(H, W, i, j, coord, R=None):
    """the centre of texel (i, j), rotated out"""
    d = env.direction((j + 0.5) / W, (i + 0.5) / H, coord)
    return d if R is None else np.asarray(R, dtype=np.float64) @ d


def relative_error(est, exact):
    """per point: |luminance of est - luminance of exact| / luminance of exact"""
    a, b = np.asarray(est, dtype=np.float64).mean(-1), np.asarray(exact, dtype=np.float64).mean(-1)
    return np.abs(a - b) / b


BOWL_AXIS = np.array([0.0, 0.55, 0.835]) / np.linalg.norm([0.0, 0.55, 0.835])      # the fitted bowl opens along it


def nearest_texel(H, W, d, coord):
    """(i, j) of the texel whose centre is nearest to the direction d"""
    k = int(np.argmax(env.texel_centres(H, W, coord).reshape(-1, 3) @ np.asarray(d, dtype=np.float64)))
    return k // W, k % W


def rotation_between(a, b):
    """the rotation [3, 3] float32 about a x b that carries the unit vector a to b (Rodrigues)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    v, c = np.cross(a, b), float(a @ b)
    vx = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return (np.eye(3) + vx + vx @ vx / (1.0 + c)).astype(F32)


SUN_SHAPE = (16, 32)
SUN_AUTHORED = (5, 11)                              # the rotated sun's texel before the rotation carries it to -BOWL_AXIS


def sun_cases(coord='mitsuba'):
    """the two suns below the bowl that the CPU run and the GPU bakes share -> [(name, map, R, unit direction of the sun)]: the
    texel nearest -BOWL_AXIS lit, and the texel SUN_AUTHORED lit under the rotation that carries its centre to -BOWL_AXIS"""
    H, W = SUN_SHAPE
    i, j = nearest_texel(H, W, -BOWL_AXIS, coord)
    R = rotation_between(sun_direction(H, W, *SUN_AUTHORED, coord), -BOWL_AXIS)
    return [('plain', sun_map(H, W, i, j), None, sun_direction(H, W, i, j, coord)),
            ('rotated', sun_map(H, W, *SUN_AUTHORED), R, sun_direction(H, W, *SUN_AUTHORED, coord, R))]


def sun_deviation(envmap, R, s, K_cos, K_map, seed, coord='mitsuba', count=400):
    """the mean relative error of the reference estimator (no occluders) against exact_irradiance over the normals with n . s >
    0.3 of `count` random ones"""
    rng = np.random.default_rng(100 + seed)
    n = ao.unit_normals(count, rng)
    texel = rng.integers(0, 2 ** 26, size=count).astype(np.int64)
    lit = n.astype(np.float64) @ s > 0.3
    exact = exact_irradiance(envmap, n[lit], R, coord)
    return relative_error(estimate(envmap, n[lit], texel[lit], K_cos, K_map, coord, seed, R), exact).mean()


# The statistical bound of the GPU bakes under a sun map (tests/test_gpu_texture_irradiance.py): three times the worst
# sun_deviation of the 16 + 16 mix over seeds 0 .. 3 and both sun_cases - the reference's own run, measured by
# tests/test_texture_irradiance_cpu.py::test_sun_map_the_mix_beats_cosine_sampling, which recomputes it.
SUN_MIX_WORST = 0.014456                            # the rotated sun at seed 3; the others 0.0120 .. 0.0140
SUN_MIX_BOUND = 3.0 * SUN_MIX_WORST
