"""fp64 numpy oracle of the image metrics: SSIM's level statistics, the pooled pyramid, MS-SSIM and the squared
error, from fp32 inputs [H, W, C] - the definition of include/nefii_amd.h's nefii_image_metrics written out with slices.  No
conv2d, no avg_pool2d: tests/test_image_metrics_cpu.py pins it against nefii_amd/scripts/evaluate.py's torch calls."""
import numpy as np

WIN, SIGMA = 11, 1.5
MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
LEVELS = len(MS_WEIGHTS)


def window():
    k = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-k * k / (2 * SIGMA * SIGMA))
    return g / g.sum()


def filter_valid(a, g):
    """separable 'valid' filtering of [h, w, C]: along h, then along w; the taps are added in their order"""
    h, w = a.shape[:2]
    t = np.zeros((h - WIN + 1, w) + a.shape[2:])
    for k in range(WIN):
        t += g[k] * a[k:k + h - WIN + 1]
    out = np.zeros((h - WIN + 1, w - WIN + 1) + a.shape[2:])
    for k in range(WIN):
        out += g[k] * t[:, k:k + w - WIN + 1]
    return out


def level_means(x, y, data_range=1.0):
    """x, y [h, w, C] float64 -> (mean ssim [C], mean cs [C]) over the (h - 10) x (w - 10) valid positions"""
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    g = window()
    mu1, mu2 = filter_valid(x, g), filter_valid(y, g)
    s11 = filter_valid(x * x, g) - mu1 * mu1
    s22 = filter_valid(y * y, g) - mu2 * mu2
    s12 = filter_valid(x * y, g) - mu1 * mu2
    cs = (2 * s12 + C2) / (s11 + s22 + C2)
    ssim = (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs
    return ssim.mean((0, 1)), cs.mean((0, 1))


def pool(a):
    """2 x 2 average with the divisor 4; an odd side is padded with one zero row / column in front"""
    h, w = a.shape[:2]
    p = np.zeros((h + h % 2, w + w % 2) + a.shape[2:])
    p[h % 2:, w % 2:] = a
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) * 0.25


def pyramid(x, levels=LEVELS):
    out = [np.asarray(x, np.float64)]
    for _ in range(levels - 1):
        out.append(pool(out[-1]))
    return out


def stats(x, y, levels, data_range=1.0):
    """[levels, C, 2] = (mean ssim, mean cs) per level and channel"""
    assert x.dtype == np.float32 and y.dtype == np.float32 and x.shape == y.shape and x.ndim == 3
    return np.stack([np.stack(level_means(a, b, data_range), -1) for a, b in zip(pyramid(x, levels), pyramid(y, levels))])


def ssim(x, y, data_range=1.0):
    return float(stats(x, y, 1, data_range)[0, :, 0].mean())


def ms_ssim_from_stats(st):
    vals = np.maximum(np.concatenate([st[:-1, :, 1], st[-1:, :, 0]]), 0.)
    return float(np.prod(vals ** np.array(MS_WEIGHTS)[:, None], axis=0).mean())


def ms_ssim(x, y, data_range=1.0):
    if min(x.shape[:2]) <= (WIN - 1) * 2 ** 4:
        raise ValueError('MS-SSIM over five scales needs images larger than 160 pixels on their smaller side')
    return ms_ssim_from_stats(stats(x, y, LEVELS, data_range))


def squared_error(x, y):
    """[C]: sum over the pixels of (x - y)^2 in double"""
    d = x.astype(np.float64) - y.astype(np.float64)
    return (d * d).sum((0, 1))


# ---- the test images -------------------------------------------------------------------------------------------------
def random_pair(H, W, C, seed):
    g = np.random.Generator(np.random.Philox(seed))
    return g.uniform(0., 1., (H, W, C)).astype(np.float32), g.uniform(0., 1., (H, W, C)).astype(np.float32)


def noisy_pair(H, W, C, seed, sigma=0.05):
    """a smooth image and a noisy copy of it: the case the metrics are for"""
    g = np.random.Generator(np.random.Philox(seed))
    yy, xx = np.mgrid[0:H, 0:W]
    a = 0.5 + 0.4 * np.sin(xx / 9.0 + np.arange(C)[:, None, None]) * np.cos(yy / 5.0)
    a = a.transpose(1, 2, 0)
    return a.astype(np.float32), np.clip(a + g.normal(0, sigma, a.shape), 0, 1).astype(np.float32)


def checker_pair(H, W, C, cell=3):
    """y = 1 - x on a checker: anti-correlated, cs < 0 at every level the checker survives"""
    yy, xx = np.mgrid[0:H, 0:W]
    a = (((yy // cell) + (xx // cell)) % 2).astype(np.float32) * np.float32(0.8) + np.float32(0.1)
    x = np.repeat(a[..., None], C, -1)
    return x, (np.float32(1.) - x).astype(np.float32)
