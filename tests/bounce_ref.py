"""numpy oracle of the recomputed bounce under a map light (nefii_envlight_bounce_sample), on top of
tests/envlight_ref.py: one-sample MIS with the balance heuristic over the renderer's three techniques (cosine, GGX, the
map's continuous inversion), the mixture density along the direction drawn and the weight f_r cos L / mix with
nefii_mc_shade's BRDF.  Parameterised by dtype: float64 is the reference, float32 measures how well the arithmetic is
conditioned at the same inputs (tests/sg64.py's rule).  The map's table (M, C) is always the one handed in - the stored
fp32 CDFs when a kernel is judged; its searches run in fp64 in either dtype (envlight_ref)."""
import numpy as np

import envlight_ref as er

TINY = 1e-6


# ---- shared inputs of the bounce tests ---------------------------------------------------------------------------------
def lognormal_map(H, W, seed, sigma=1.5):
    g = np.random.Generator(np.random.Philox(seed))
    return np.exp(g.normal(size=(H, W, 3)) * sigma).astype(np.float32)


def bright_texel_map():
    """the 32 x 64 map of test_mean_matches_the_exact_integral_on_a_bright_texel_map (tests/test_gpu_envlight.py)"""
    env = lognormal_map(32, 64, 9, 0.6)
    env[10, 20] *= 400.
    env[25, 50] *= 50.
    return env


SPEC, ALBEDO = np.array([0.3, 0.3, 0.3]), np.array([0.6, 0.4, 0.25])      # of that test


def cases(n_cases, seed):
    """(normal, view, roughness) of tests/test_gpu_envlight.py's estimator tests"""
    g = np.random.Generator(np.random.Philox(seed))
    out = []
    for c in range(n_cases):
        nrm = g.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        t = g.normal(size=3)
        t -= (t @ nrm) * nrm
        t /= np.linalg.norm(t)
        cv = g.uniform(0.25, 1.0)
        v = cv * nrm + np.sqrt(1 - cv * cv) * t
        out.append((nrm, v, (0.089, 0.3, 1.0)[c % 3]))
    return out


def integral_cases():
    """the 32 (coord, k, normal, view, roughness) of the bright-texel integral test: cases(16, .) per axis convention"""
    return [(coord, k) + c for coord in er.COORDS for k, c in enumerate(cases(16, 2 + (coord == 'blender')))]


def philox_uniforms(n, seed):
    """[n, 3] uniforms in [0, 1), Philox-seeded and rounded through float32 (what a kernel would be handed)"""
    return np.random.Generator(np.random.Philox(seed)).random((n, 3), dtype=np.float32)


# ---- the BRDF techniques -------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(-1)


def to_world(local, n):
    dt = n.dtype
    up = np.where((n[:, 0:1] > 0.9), np.array([0., 1., 0.], dt), np.array([1., 0., 0.], dt))
    t = np.cross(up, n)
    t = t / (np.linalg.norm(t, axis=-1, keepdims=True) + dt.type(TINY))
    s = np.cross(t, n)
    return local[:, 0:1] * t + local[:, 1:2] * s + local[:, 2:3] * n


def _polar(theta, phi):
    return np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], -1)


def sample_cos(n, r1, r2):
    dt = n.dtype.type
    theta = np.arccos(np.sqrt(dt(1) - r1))
    return to_world(_polar(theta, dt(2 * np.pi) * r2), n)


def sample_ggx(n, v, rough, r1, r2):
    dt = n.dtype.type
    theta = np.arctan(rough * rough * np.sqrt(r1 / (dt(1) - r1)))
    h = to_world(_polar(theta, dt(2 * np.pi) * r2), n)
    return dt(2) * _dot(v, h)[:, None] * h - v


def pdf_cos(wo, n):
    dt = n.dtype.type
    return np.maximum(_dot(wo, n), dt(TINY)) / dt(np.pi)


def pdf_ggx(wo, n, v, rough):
    dt = n.dtype.type
    h = wo + v
    with np.errstate(invalid='ignore', divide='ignore'):
        h = h / np.linalg.norm(h, axis=-1, keepdims=True)
    h = np.where(np.isnan(h), n, h)
    c = np.maximum(_dot(h, n), dt(TINY))
    r4 = (rough * rough) * (rough * rough)
    root = c * c + (dt(1) - c * c) / r4
    pdf_h = c / (dt(np.pi) * r4 * root * root)
    return pdf_h / (dt(4) * np.maximum(_dot(h, v), dt(TINY)))


def brdf_cos(n, v, wo, rough, albedo, spec):
    """(specular, diffuse) f_r * cos per row - envlight_ref.brdf_cos with a normal, view, roughness and albedo of its own
    in every row, in the rows' dtype"""
    dt = n.dtype.type
    h = wo + v
    h = h / (np.linalg.norm(h, axis=-1, keepdims=True) + dt(TINY))
    nh = np.maximum(_dot(n, h), dt(0))
    vh = np.maximum(_dot(v, h), dt(0))
    P = np.exp2(-(dt(5.55473) * vh + dt(6.8316)) * vh)
    d1 = np.maximum(_dot(v, n), dt(0))
    d2 = np.maximum(_dot(wo, n), dt(0))
    den = dt(4) * d1 * d2 + dt(TINY)
    a4 = (rough * rough) * (rough * rough)
    root = nh * nh + (dt(1) - nh * nh) / a4
    D = dt(1) / (dt(np.pi) * a4 * root * root)
    k = (rough + dt(1)) * (rough + dt(1)) / dt(8)
    G = (d1 / (d1 * (dt(1) - k) + k + dt(TINY))) * (d2 / (d2 * (dt(1) - k) + k + dt(TINY)))
    F = spec[None, :] + (dt(1) - spec[None, :]) * P[:, None]
    s = F * (D * G / den * d2)[:, None]
    d = albedo / dt(np.pi) * d2[:, None]
    return s, d


# ---- the estimator ---------------------------------------------------------------------------------------------------
def _rows(x, m, dtype, cols=None):
    """x broadcast to [m] (cols None; [m, 1] and scalars welcome) or [m, cols]"""
    x = np.asarray(x, dtype)
    if cols is None and x.ndim:
        x = x.reshape(-1)
    return np.ascontiguousarray(np.broadcast_to(x, (m,) if cols is None else (m, cols)))


def _sin_phi(wo, coord):
    """sin of the polar angle of wo in wo's dtype, as texel_of has it: rho / |(rho, up)| of the normalised direction"""
    dt = wo.dtype.type
    d = wo / np.maximum(np.linalg.norm(wo, axis=-1, keepdims=True), dt(1e-8))
    up = d[:, 1] if coord == 'mitsuba' else d[:, 2]
    side = d[:, 2] if coord == 'mitsuba' else d[:, 1]
    rho = np.sqrt(d[:, 0] * d[:, 0] + side * side)
    r = np.sqrt(rho * rho + up * up)
    return np.where(rho > 0, rho / np.where(r > 0, r, dt(1)), dt(0))


def weight_at(wo, envmap, M, C, coord, n, v, rough, albedo, spec, dtype=np.float64, drawn=None):
    """(mix [m], weight [m, 3]) of the estimator for GIVEN directions wo [m, 3]: mix = (pdf_cos + pdf_ggx + p_map) / 3,
    weight = max(s L / mix, 0) + max(d L / mix, 0) with (s, d) = brdf_cos.  The texel (radiance and P(i, j)) is the one
    under wo; drawn = (mask [m], i [m], j [m]) names the texel that was drawn for the rows of mask (technique 2).
    n, v, albedo: [3] or [m, 3]; rough: scalar or [m]; spec [3]."""
    wo = np.asarray(wo, dtype)
    m = wo.shape[0]
    H, W = envmap.shape[:2]
    n, v, albedo = (_rows(x, m, dtype, 3) for x in (n, v, albedo))
    rough = _rows(rough, m, dtype)
    spec = np.asarray(spec, dtype).reshape(3)
    i, j, _ = er.texel_of(wo, H, W, coord)
    if drawn is not None:
        mask, di, dj = drawn
        i, j = np.where(mask, di, i), np.where(mask, dj, j)
    P = np.asarray(er.texel_prob(M, C, i, j), dtype)
    s_phi = _sin_phi(wo, coord)
    two_pi2 = np.dtype(dtype).type(2 * np.pi ** 2)
    p_map = np.where(s_phi > 0, P * np.dtype(dtype).type(H) * np.dtype(dtype).type(W) /
                     (two_pi2 * np.where(s_phi > 0, s_phi, 1)), 0).astype(dtype)
    mix = (pdf_cos(wo, n) + pdf_ggx(wo, n, v, rough) + p_map) / np.dtype(dtype).type(3)
    L = np.asarray(envmap, dtype)[i, j]
    s, d = brdf_cos(n, v, wo, rough, albedo, spec)
    weight = np.maximum(s * L / mix[:, None], 0) + np.maximum(d * L / mix[:, None], 0)
    return mix, weight


def technique(u0):
    """k = min((int)(3.f * u0), 2) in fp32"""
    return np.minimum((np.float32(3.) * np.asarray(u0, np.float32)).astype(np.int64), 2)


def sample(envmap, M, C, coord, n, v, rough, albedo, spec, uniforms, dtype=np.float64):
    """The estimator itself for uniforms [m, 3] -> (k [m], wo [m, 3], mix [m], weight [m, 3])"""
    k, wo, mix, weight, _ = sample_texels(envmap, M, C, coord, n, v, rough, albedo, spec, uniforms, dtype)
    return k, wo, mix, weight


def sample_texels(envmap, M, C, coord, n, v, rough, albedo, spec, uniforms, dtype=np.float64):
    """sample() and the drawn = (mask, i, j) it handed to weight_at"""
    u = np.asarray(uniforms, np.float32)
    m = u.shape[0]
    k = technique(u[:, 0])
    nn, vv = (_rows(x, m, dtype, 3) for x in (n, v))
    rr = _rows(rough, m, dtype)
    u1, u2 = u[:, 1].astype(dtype), u[:, 2].astype(dtype)
    wo = np.zeros((m, 3), dtype)
    s0, s1, s2 = k == 0, k == 1, k == 2
    wo[s0] = sample_cos(nn[s0], u1[s0], u2[s0])
    wo[s1] = sample_ggx(nn[s1], vv[s1], rr[s1], u1[s1], u2[s1])
    di, dj = np.zeros(m, np.int64), np.zeros(m, np.int64)
    if s2.any():
        i, j, d, _ = er.sample(M, C, coord, u[s2, 1], u[s2, 2])
        wo[s2] = d.astype(dtype)
        di[s2], dj[s2] = i, j
    drawn = (s2, di, dj)
    mix, weight = weight_at(wo, envmap, M, C, coord, nn, vv, rr, albedo, spec, dtype, drawn)
    return k, wo, mix, weight, drawn


def estimate(envmap, coord, n, v, rough, albedo, spec, draws, seed):
    """mean, standard error and standard deviation per channel of the fp64 oracle estimator over `draws` Philox-seeded
    uniforms, and the largest weight relative to the mean, on the fp32 table a build would store"""
    M, C = [x.astype(np.float32) for x in er.build(envmap)]
    _, _, _, w = sample(envmap, M, C, coord, n, v, rough, albedo, spec, philox_uniforms(draws, seed))
    mean, std = w.mean(0), w.std(0, ddof=1)
    return mean, std / np.sqrt(draws), std, (w.max(0) / np.maximum(mean, 1e-300)).max()
