"""numpy fp64 restatement of the adaptive-sampling kernels (nefii_amd/csrc/nefii_adaptive.hip) and the synthetic
scene its premise was checked on.  A frame is rendered in rounds of R rays per pixel:

  moments   rgb [P R, 3] -> (ebar, M2) per pixel: ebar = Y(mean colour), M2 = sum_r (Y(rgb_r) - ebar)^2, two passes
  merge     sum[p] += R row;  stat[p] = (n, mean, M2) by the pairwise rule, in the kernel's order of operations (bit for bit)
  score     s = sqrt(M2 / (n - 1)) / (|mean| + eps), 0 where n < 2 or fl32(s) is not finite; dilate: 3 x 3 maximum
  rounds    k_p(lambda) = min(K, max(1, ceil(fl32(lambda s_p)))), a NaN product gives 1;  T = sum k_p
  allocate  the largest finite fp32 lambda >= 0 with T(lambda) <= N, by bisection on its bit pattern
  finalise  out = fl32(sum / n), all()-columns 1 where sum == n, rays = n, variance = M2 / (n (n - 1))"""
import struct

import numpy as np

FLT_MAX_BITS = 0x7F7FFFFF


def luminance64(c):
    c = np.asarray(c, np.float64)
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def moments(rgb, R):
    """rgb [P R, 3] (any float type, read as given) -> [P, 2] float64 = (ebar, M2), not yet rounded to fp32"""
    x = np.asarray(rgb, np.float64).reshape(-1, R, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        ebar = luminance64(x.sum(1) / float(R))
        dev = luminance64(x) - ebar[:, None]
        return np.stack([ebar, (dev * dev).sum(1)], 1)


def merge(rows, pixel, R, sum_, stat):
    """in place on sum_ [P, C] and stat [P, 3] float64; rows [m, C + 2], read as given (the kernel's are float32); pixel [m] or
    None"""
    rows = np.asarray(rows).astype(np.float64)
    C = sum_.shape[1]
    p = np.arange(rows.shape[0]) if pixel is None else np.asarray(pixel, np.int64)
    rays = np.float64(R)
    with np.errstate(invalid='ignore', over='ignore'):
        sum_[p] = sum_[p] + rays * rows[:, :C]
        n, mean, m2 = stat[p, 0], stat[p, 1], stat[p, 2]
        ebar, m2_b = rows[:, C], rows[:, C + 1]
        delta = ebar - mean
        n_new = n + rays
        stat[p, 0] = n_new
        stat[p, 1] = mean + (delta * rays) / n_new
        stat[p, 2] = (m2 + m2_b) + (delta * delta) * ((n * rays) / n_new)


def score(stat, H, W, eps, dilate):
    """-> [H W] float64: the score before its one rounding (np.float32(score(...)) is what the kernel stores)"""
    stat = np.asarray(stat, np.float64)
    n, mean, m2 = stat[:, 0], stat[:, 1], stat[:, 2]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        s = np.sqrt(m2 / (n - 1.)) / (np.abs(mean) + eps)
        keep = (n >= 2.) & np.isfinite(s.astype(np.float32))
    s = np.where(keep, s, 0.).reshape(H, W)
    if dilate:
        pad = np.zeros((H + 2, W + 2))              # scores are >= 0: a zero border is "not in the image"
        pad[1:-1, 1:-1] = s
        s = np.max([pad[1 + j:1 + j + H, 1 + i:1 + i + W] for j in (-1, 0, 1) for i in (-1, 0, 1)], axis=0)
    return s.reshape(-1)


def lambda_of(bits):
    return np.float32(struct.unpack('<f', struct.pack('<I', int(bits)))[0])


def bits_of(lam):
    return struct.unpack('<I', struct.pack('<f', float(lam)))[0]


def rounds(score32, lam, K):
    """k [P] int64 for fp32 scores and an fp32 lambda"""
    with np.errstate(invalid='ignore', over='ignore'):
        x = np.float32(lam) * np.asarray(score32, np.float32)
        assert x.dtype == np.float32
        up = np.ceil(np.where(x > 1., np.minimum(x, np.float32(K)), np.float32(1.)))
    return np.where(x > 1., np.where(x >= np.float32(K), K, up), 1).astype(np.int64)


def allocate(score32, N, K):
    """-> (k, lambda fp32, T): lambda the largest finite fp32 >= 0 with T(lambda) <= N; N >= P"""
    score32 = np.asarray(score32, np.float32)
    assert N >= score32.size
    lo, hi = 0, FLT_MAX_BITS + 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if rounds(score32, lambda_of(mid), K).sum() <= N:
            lo = mid
        else:
            hi = mid
    k = rounds(score32, lambda_of(lo), K)
    return k, lambda_of(lo), int(k.sum())


def finalise(sum_, stat, mask_columns=()):
    """-> out [P, C] float32, rays [P] int32, variance [P] float32"""
    n, m2 = stat[:, 0], stat[:, 2]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        out = (sum_ / n[:, None]).astype(np.float32)
        for c in mask_columns:
            out[:, c] = (sum_[:, c] == n).astype(np.float32)
        var = np.where(n >= 2., m2 / (n * (n - 1.)), 0.).astype(np.float32)
    return out, n.astype(np.int32), var


# ---- the synthetic scene of the premise ----------------------------------------------------------------------------------
def scene(H=48, W=64):
    """-> clean luminance [H, W], the Gamma shape k [H, W], background [H, W] (every sample is exactly the clean value)"""
    v, u = np.meshgrid((np.arange(H) + 0.5) / H * 2. - 1., (np.arange(W) + 0.5) / W * 2. - 1., indexing='ij')
    clean = 0.2 + 0.8 * (0.5 + 0.5 * np.sin(3. * u + 2. * v))
    clean = np.where(u + 0.5 * v > 0.2, 0.25 * clean, clean)
    return clean, np.interp(u, [-1., 1.], [25., 0.45]), u * u + v * v > 0.81


def draw(rng, clean, k, background, R):
    """R samples per pixel [R, H, W]: clean x Gamma(k, 1 / k), exactly clean on the background"""
    g = rng.gamma(k, 1. / k, size=(R,) + clean.shape)
    return np.where(background, clean, clean * g)


def grey_rows(samples):
    """samples [R, m] of m pixels -> a round's packed rows [m, 3] float32 = (mean, ebar, M2): the samples as grey rays"""
    R, m = samples.shape
    rgb = np.repeat(samples.T.reshape(m * R, 1), 3, axis=1).astype(np.float32)
    mom = moments(rgb, R)
    mean = rgb.astype(np.float64).reshape(m, R, 3)[:, :, 0].sum(1) / R
    return np.concatenate([mean[:, None], mom], 1).astype(np.float32)


def simulate(seed, pilot=4, budget=16, max_rounds=16, eps=0.01, dilate=True, H=48, W=64):
    """The premise's experiment -> dict: ratio (adaptive / uniform relative MSE), N, T, k, lam, rays, est, uniform, clean.  Draw
    order: the uniform frame's `budget` samples, the pilot, then one full (pilot, H, W) draw per round masked to the active
    pixels."""
    clean, shape, background = scene(H, W)
    rng = np.random.Generator(np.random.Philox(seed))
    uniform = draw(rng, clean, shape, background, budget).mean(0)
    P = H * W
    sum_, stat = np.zeros((P, 1)), np.zeros((P, 3))
    merge(grey_rows(draw(rng, clean, shape, background, pilot).reshape(pilot, P)), None, pilot, sum_, stat)
    s32 = score(stat, H, W, eps, dilate).astype(np.float32)
    N = budget * P // pilot
    k, lam, T = allocate(s32, N, max_rounds)
    for j in range(2, max_rounds + 1):
        active = np.nonzero(k >= j)[0]
        if active.size == 0:
            break
        samples = draw(rng, clean, shape, background, pilot).reshape(pilot, P)[:, active]
        merge(grey_rows(samples), active, pilot, sum_, stat)
    out, rays, var = finalise(sum_, stat)
    est = out[:, 0].astype(np.float64).reshape(H, W)
    rel = lambda x: np.mean(((x - clean) / (clean + eps)) ** 2)
    return dict(ratio=rel(est) / rel(uniform), N=N, T=T, k=k, lam=lam, rays=rays, est=est, uniform=uniform, clean=clean,
                score=s32, variance=var)
