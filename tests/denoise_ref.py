"""numpy oracle of the guided a-trous filter, written from the definition and not from the kernel, and the
synthetic scene the denoiser's tests share.

One level with step s on an H x W frame.  Guides G0[p] = (n, valid), G1[p] = (x, 0); signals C[s][p] = (r, g, b).  For a
valid centre p the taps are q = p + s (i, j), i, j in -2 .. 2, inside the image, h = [1 4 6 4 1] / 16:

    w_s(p,q) = h_i h_j valid(q) finite(q) w_n w_x w_c,s
    w_n   = max(0, n_p . n_q)^sigma_n
    w_x   = exp(-|n_p . (x_q - x_p)| / (sigma_x |x_q - x_p| + 1e-12))
    w_c,s = exp(-|Y_s(p) - Y_s(q)| / ((|Y_s(p)| + |Y_s(q)| + 1e-12) sigma_c_level)),  Y = 0.2126 r + 0.7152 g + 0.0722 b
    out_s(p) = sum_q w_s c_s(q) / sum_q w_s;  in_s(p) where that sum is 0;  in(p), bitwise, at an invalid p

finite(q) = 0 where any channel of any signal at q is NaN or inf.  Two cases the formula leaves open: equal luminances have
w_c = 1 whatever the denominator (sigma_c = 0 would give 0 / 0), and a centre that is not finite has no luminance, so its
w_c is 1 for every tap: it becomes the guided average of its finite neighbours.

`level` runs in the dtype it is given: float64 is the reference, float32 measures the conditioning (tests/sg64.py)."""
import numpy as np

H5 = np.array([1., 4., 6., 4., 1.]) / 16.
START = dict(levels=5, sigma_n=32., sigma_x=0.1, sigma_c=1.)          # the issue's starting parameters


def luminance(c, dtype):
    return dtype(0.2126) * c[..., 0] + dtype(0.7152) * c[..., 1] + dtype(0.0722) * c[..., 2]


def level(g0, g1, c, step, sigma_n, sigma_x, sigma_c_level, dtype=np.float64):
    """g0, g1 [H, W, 4], c [S, H, W, 3] -> the filtered signals [S, H, W, 3] in `dtype`"""
    dtype = np.dtype(dtype).type
    g0, g1, c = np.asarray(g0).astype(dtype), np.asarray(g1).astype(dtype), np.asarray(c).astype(dtype)
    S, H, W, _ = c.shape
    sigma_n, sigma_x, sigma_c_level = dtype(sigma_n), dtype(sigma_x), dtype(sigma_c_level)
    tiny = dtype(1e-12)
    n_p, x_p, valid = g0[..., :3], g1[..., :3], g0[..., 3] > 0.5
    finite = np.isfinite(c).all(axis=(0, 3))
    clean = np.where(finite[None, :, :, None], c, dtype(0))         # a tap that is not finite has weight 0: keep 0 * NaN out
    lum = luminance(clean, dtype)                                   # [S, H, W]
    acc = np.zeros_like(c)
    wsum = np.zeros((S, H, W), dtype)
    ys, xs = np.arange(H), np.arange(W)
    with np.errstate(all='ignore'):
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
                geo = dtype(H5[j + 2] * H5[i + 2]) * w_n * w_x
                for s in range(S):
                    y_q = lum[s][qy[:, None], qx[None, :]]
                    diff = np.abs(lum[s] - y_q)
                    w_c = np.exp(-diff / ((np.abs(lum[s]) + np.abs(y_q) + tiny) * sigma_c_level))
                    w_c = np.where((diff == 0) | ~finite, dtype(1), w_c)
                    w = np.where(ok, geo * w_c, dtype(0)).astype(dtype)
                    acc[s] += w[..., None] * clean[s][qy[:, None], qx[None, :]]
                    wsum[s] += w
        out = np.where((wsum > 0)[..., None], acc / wsum[..., None], c)
    return np.where(valid[None, :, :, None], out, c)


def cascade(g0, g1, c, levels, sigma_n, sigma_x, sigma_c, dtype=np.float64):
    """levels l = 0 .. levels-1 with step 2^l and sigma_c 2^-l, each on the output of the one before"""
    for l in range(levels):
        c = level(g0, g1, c, 1 << l, sigma_n, sigma_x, sigma_c * 2. ** -l, dtype)
    return c


def cascaded_kernel_1d(levels):
    """the 1-D kernel of `levels` B3-spline levels with the colour and geometry terms off: the convolution of h dilated by
    1, 2, 4, ..."""
    k = np.array([1.])
    for l in range(levels):
        h = np.zeros(4 * (1 << l) + 1)
        h[::1 << l] = H5
        k = np.convolve(k, h)
    return k


def flat_guides(H, W):
    """a coplanar, all-valid frame: the plane z = 0 seen from above"""
    g0 = np.zeros((H, W, 4), np.float32)
    g0[..., 2] = 1.
    g0[..., 3] = 1.
    g1 = np.zeros((H, W, 4), np.float32)
    g1[..., 1], g1[..., 0] = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    return g0, g1


def scene(H, W, seed=0, n_signals=2):
    """An orthographic view down -z of a sphere (radius 0.45 about the origin) on a tilted plane, pixel centres on
    [-1, 1]^2 -> g0, g1 [H, W, 4] float32, clean and noisy signals [S, H, W, 3] float32.  Signal 0 is a Lambert term under one
    directional light plus an ambient term, signal 1 a smooth glossy lobe; the noise is multiplicative, Gamma(4, 1/4) per
    pixel and channel (mean 1, relative standard deviation 0.5) from a seeded generator.  The top H // 12 rows are
    background (valid = 0), and where the frame has more than 64 pixels a few scattered pixels are invalid too."""
    rng = np.random.Generator(np.random.Philox(seed))
    v, u = np.meshgrid((np.arange(H) + 0.5) / H * 2. - 1., (np.arange(W) + 0.5) / W * 2. - 1., indexing='ij')
    r2 = u * u + v * v
    on_sphere = r2 < 0.45 ** 2
    z_sphere = np.sqrt(np.maximum(0.45 ** 2 - r2, 0.))
    z = np.where(on_sphere, z_sphere, -0.6 + 0.3 * u + 0.2 * v)
    plane_n = np.array([-0.3, -0.2, 1.]) / np.linalg.norm([-0.3, -0.2, 1.])
    nrm = np.where(on_sphere[..., None], np.stack([u, v, z_sphere], -1) / 0.45, plane_n)
    valid = np.ones((H, W), bool)
    valid[:H // 12] = False
    if H * W > 64:
        k = rng.choice(H * W, size=max(3, H * W // 400), replace=False)
        valid.reshape(-1)[k] = False
    light = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
    half = (light + np.array([0., 0., 1.])) / np.linalg.norm(light + np.array([0., 0., 1.]))
    lambert = np.maximum(nrm @ light, 0.)[..., None] * np.array([1.0, 0.8, 0.6]) + np.array([0.10, 0.12, 0.15])
    glossy = (np.maximum(nrm @ half, 0.) ** 20)[..., None] * np.array([0.9, 0.9, 1.0]) + 0.05
    clean = np.stack([lambert, glossy])[:n_signals]
    noisy = clean * rng.gamma(4., 0.25, size=clean.shape)
    g0 = np.concatenate([nrm, valid[..., None].astype(np.float64)], -1).astype(np.float32)
    g1 = np.concatenate([np.stack([u, v, z], -1), np.zeros((H, W, 1))], -1).astype(np.float32)
    return g0, g1, clean.astype(np.float32), noisy.astype(np.float32)


def rel_rmse(x, ref, valid):
    """relative RMSE over the valid pixels, in double"""
    x, ref = np.asarray(x, np.float64)[..., valid, :], np.asarray(ref, np.float64)[..., valid, :]
    return float(np.sqrt(((x - ref) ** 2).mean() / (ref ** 2).mean()))
