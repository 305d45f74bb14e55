"""numpy oracle of the per-pixel moments and of the variance-guided a-trous level, written from the
definitions and not from the kernels, and the "shadow scene" its tests share.

moments.  Row p R + r of diffuse, albedo, specular [P R, 3] and hit [P R] is ray r of pixel p.  For a pixel whose rays all hit,
with abar the mean albedo per channel and a = max(abar, ALBEDO_FLOOR):

    signal 0 = (mean_r diffuse_r / a, v),  signal 1 = (mean_r specular_r, v),  v = sum_r (e_r - ebar)^2 / (R (R - 1))

with e_r = Y(diffuse_r / a) and Y(specular_r), Y the Rec. 709 luminance: the variance of the MEAN of the luminance.  All in
double.  ebar is the mean of the e_r, formed as e_0 + mean(e_r - e_0), so that equal samples have ebar = e_r and a variance of
exactly 0.  A NaN or inf sample - albedo included - makes the lanes it enters non-finite; a pixel with a ray that missed is
four zeros in both signals.

level_var.  denoise_ref.level on signals C_s[p] = (r, g, b, v), every use of v being max(v, 0):

    vbar_s(p) = sum g_ij v_s(q) / sum g_ij over the 3 x 3 pixels at UNIT offsets that are in the image, valid and finite,
                g = [1 2 1] x [1 2 1] / 16
    w_l,s = exp(-|Y_s(p) - Y_s(q)| / (sigma_l sqrt(vbar_s(p)) + 1e-12))
    w = h_i h_j valid(q) finite(q) w_n w_x w_l,s
    out_s(p).rgb = sum w c_s(q) / sum w,  out_s(p).v = sum w^2 v_s(q) / (sum w)^2;  in_s(p), four lanes, where sum w = 0;
    in(p), bitwise, at an invalid p

finite(q) = 0 where any of the four lanes of any signal at q is NaN or inf.  w_l = 1 for equal luminances, for a centre that
is not finite or that has no pixel in vbar, and for sigma_l = inf (inf * sqrt(0) is not formed).  sigma_l is the same at
every level of cascade_var."""
import numpy as np

import denoise_ref as dr

ALBEDO_FLOOR = float(np.float32(1e-3))              # NEFII_ALBEDO_FLOOR, an fp32 number
G3 = np.array([1., 2., 1.]) / 4.
START = dict(levels=5, sigma_n=32., sigma_x=0.1, sigma_l=4.)


def luminance64(c):
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def variance_of_mean(e):
    """e [P, R] -> sum_r (e_r - ebar)^2 / (R (R - 1)), two passes in double"""
    R = e.shape[1]
    with np.errstate(all='ignore'):
        ebar = e[:, :1] + (e - e[:, :1]).mean(1, keepdims=True)
        return ((e - ebar) ** 2).sum(1) / (R * (R - 1.))


def moments(diffuse, albedo, specular, hit, R):
    """[P R, 3] x 3 and hit [P R] -> signals [2, P, 4] float64"""
    d, a, s = (np.asarray(x, np.float64).reshape(-1, R, 3) for x in (diffuse, albedo, specular))
    all_hit = np.asarray(hit).reshape(-1, R).astype(bool).all(1)
    with np.errstate(all='ignore'):
        abar = a.mean(1)
        floor = np.where(abar < ALBEDO_FLOOR, ALBEDO_FLOOR, abar)               # a NaN mean stays NaN
        poison = 0. * abar.sum(-1)                                             # NaN where an albedo is NaN or inf
        out = np.zeros((2, d.shape[0], 4))
        out[0, :, :3] = d.mean(1) / floor + poison[:, None]
        out[0, :, 3] = variance_of_mean(luminance64(d / floor[:, None, :])) + poison
        out[1, :, :3] = s.mean(1)
        out[1, :, 3] = variance_of_mean(luminance64(s))
    out[:, ~all_hit] = 0.
    return out


def level_var(g0, g1, c4, step, sigma_n, sigma_x, sigma_l, dtype=np.float64):
    """g0, g1 [H, W, 4], c4 [S, H, W, 4] -> the filtered signals [S, H, W, 4] in `dtype`"""
    dtype = np.dtype(dtype).type
    g0, g1, c4 = np.asarray(g0).astype(dtype), np.asarray(g1).astype(dtype), np.asarray(c4).astype(dtype)
    S, H, W, _ = c4.shape
    stop_off = bool(np.isinf(sigma_l))
    sigma_n, sigma_x, sigma_l = dtype(sigma_n), dtype(sigma_x), dtype(sigma_l)
    tiny = dtype(1e-12)
    n_p, x_p, valid = g0[..., :3], g1[..., :3], g0[..., 3] > 0.5
    finite = np.isfinite(c4).all(axis=(0, 3))
    clean = np.where(finite[None, :, :, None], c4, dtype(0))        # a tap that is not finite has weight 0: keep 0 * NaN out
    lum = dr.luminance(clean, dtype)                                # [S, H, W]
    var = np.maximum(clean[..., 3], dtype(0))
    ys, xs = np.arange(H), np.arange(W)
    with np.errstate(all='ignore'):
        # the prefiltered variance, from unit offsets whatever the step
        vsum, gsum = np.zeros((S, H, W), dtype), np.zeros((H, W), dtype)
        for j in range(-1, 2):
            qy = ys + j
            in_y = (qy >= 0) & (qy < H)
            qy = np.clip(qy, 0, H - 1)
            for i in range(-1, 2):
                qx = xs + i
                in_x = (qx >= 0) & (qx < W)
                qx = np.clip(qx, 0, W - 1)
                take = lambda a: a[..., qy[:, None], qx[None, :]]
                ok = in_y[:, None] & in_x[None, :] & take(valid) & take(finite)
                g = dtype(G3[j + 1] * G3[i + 1])
                vsum += np.where(ok, g * take(var), dtype(0)).astype(dtype)
                gsum += np.where(ok, g, dtype(0)).astype(dtype)
        stop_on = finite & (gsum > 0) & (not stop_off)
        scale = np.where(stop_on, sigma_l * np.sqrt(vsum / gsum) + tiny, dtype(1)).astype(dtype)      # [S, H, W]

        acc = np.zeros_like(c4)
        wsum = np.zeros((S, H, W), dtype)
        for j in range(-2, 3):
            qy = ys + j * step
            in_y = (qy >= 0) & (qy < H)
            qy = np.clip(qy, 0, H - 1)
            for i in range(-2, 3):
                qx = xs + i * step
                in_x = (qx >= 0) & (qx < W)
                qx = np.clip(qx, 0, W - 1)
                take = lambda a: a[qy[:, None], qx[None, :]]
                ok = in_y[:, None] & in_x[None, :] & take(valid) & take(finite)
                n_q, x_q = take(n_p), take(x_p)
                d = n_p[..., 0] * n_q[..., 0] + n_p[..., 1] * n_q[..., 1] + n_p[..., 2] * n_q[..., 2]
                w_n = np.power(np.maximum(d, dtype(0)), sigma_n)
                dx = x_q - x_p
                dist = np.sqrt(dx[..., 0] * dx[..., 0] + dx[..., 1] * dx[..., 1] + dx[..., 2] * dx[..., 2])
                off = np.abs(n_p[..., 0] * dx[..., 0] + n_p[..., 1] * dx[..., 1] + n_p[..., 2] * dx[..., 2])
                w_x = np.exp(-off / (sigma_x * dist + tiny))
                geo = dtype(dr.H5[j + 2] * dr.H5[i + 2]) * w_n * w_x
                for s in range(S):
                    diff = np.abs(lum[s] - take(lum[s]))
                    w_l = np.exp(-diff / scale[s])
                    w_l = np.where((diff == 0) | ~stop_on, dtype(1), w_l)
                    w = np.where(ok, geo * w_l, dtype(0)).astype(dtype)
                    acc[s, ..., :3] += w[..., None] * take(clean[s, ..., :3])
                    acc[s, ..., 3] += w * w * take(var[s])
                    wsum[s] += w
        out = np.concatenate([acc[..., :3] / wsum[..., None], (acc[..., 3] / (wsum * wsum))[..., None]], -1)
        out = np.where((wsum > 0)[..., None], out, c4)
    return np.where(valid[None, :, :, None], out, c4)


def cascade_var(g0, g1, c4, levels, sigma_n, sigma_x, sigma_l, dtype=np.float64):
    """levels l = 0 .. levels-1 with step 2^l and the same sigma_l, each on the output of the one before"""
    for l in range(levels):
        c4 = level_var(g0, g1, c4, 1 << l, sigma_n, sigma_x, sigma_l, dtype)
    return c4


def shadow_scene(H, W, R, seed=0):
    """denoise_ref.scene with a hard shadow that geometry does not explain - the diffuse light times 0.25 where
    u + 0.5 v > 0.2, across the coplanar pixels of the plane - and heteroscedastic noise: R samples per pixel, Gamma(k, 1 / k)
    per sample and channel with the shape k falling from 25 at u = -1 to 0.45 at u = 1 (relative deviation 0.2 .. 1.5)
    -> g0, g1 [H, W, 4], clean [2, H, W, 3], signals4 [2, H, W, 4] = (mean over the rays, variance of the mean of Y), float32"""
    g0, g1, clean, _ = dr.scene(H, W, seed)
    v, u = np.meshgrid((np.arange(H) + 0.5) / H * 2. - 1., (np.arange(W) + 0.5) / W * 2. - 1., indexing='ij')
    clean = clean.astype(np.float64)
    clean[0] = np.where((u + 0.5 * v > 0.2)[..., None], 0.25 * clean[0], clean[0])
    rng = np.random.Generator(np.random.Philox(seed + 100))
    k = np.interp(u, [-1., 1.], [25., 0.45])
    samples = clean[:, None] * rng.gamma(k[..., None], 1. / k[..., None], size=(2, R, H, W, 3))
    var = luminance64(samples).var(axis=1, ddof=1) / R
    signals4 = np.concatenate([samples.mean(1), var[..., None]], -1)
    return g0, g1, clean.astype(np.float32), signals4.astype(np.float32)
