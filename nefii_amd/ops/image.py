"""Whole-frame kernels: the a-trous denoiser and the PSNR / SSIM / MS-SSIM statistics."""
import ctypes
import math

import torch

from ._call import _ptr, call, check_tensor, nbytes, need_gpu


# ---- the a-trous denoiser of Monte-Carlo frames -----------------------------------------------------
DENOISE_MAX_SIDE = 16384


def _atrous_level(symbol, sigma_3_name, guides0, guides1, src, dst, height, width, step, sigma_n, sigma_x, sigma_3):
    """the checks and the call of the two level entry points; sigma_3_name names the third sigma in the messages"""
    height, width, step = int(height), int(width), int(step)
    if not (1 <= height <= DENOISE_MAX_SIDE and 1 <= width <= DENOISE_MAX_SIDE):
        raise ValueError('height and width must lie in 1 .. %d, got %d x %d' % (DENOISE_MAX_SIDE, height, width))
    if step < 1:
        raise ValueError('step must be at least 1, got %d' % step)
    for name, v in (('sigma_n', sigma_n), ('sigma_x', sigma_x), (sigma_3_name, sigma_3)):
        if not float(v) >= 0.:
            raise ValueError('%s must not be negative or NaN, got %r' % (name, v))
    if math.isinf(float(sigma_n)):
        raise ValueError('sigma_n must be finite')
    if not torch.is_tensor(src) or src.dim() != 3 or src.shape[0] not in (1, 2):
        raise ValueError('src must be [S, H*W, 4] with S = 1 or 2, got %s'
                         % (tuple(src.shape) if torch.is_tensor(src) else type(src).__name__,))
    n = height * width
    for name, t, shape in (('guides0', guides0, (n, 4)), ('guides1', guides1, (n, 4)), ('src', src, (src.shape[0], n, 4)),
                           ('dst', dst, (src.shape[0], n, 4))):
        check_tensor(name, t, torch.float32, shape)
    if dst.data_ptr() == src.data_ptr():
        raise ValueError('dst must not be src: a level reads its taps from the whole input')
    need_gpu(guides0, guides1, src, dst)
    call(symbol, _ptr(guides0), _ptr(guides1), _ptr(src), _ptr(dst), src.shape[0], height, width, step, float(sigma_n),
         float(sigma_x), float(sigma_3))
    return dst


def denoise_atrous(guides0, guides1, src, dst, height, width, step, sigma_n, sigma_x, sigma_c_level):
    """One level of the guided a-trous filter (nefii_denoise_atrous) on a height x width frame: guides0
    [H*W, 4] = (normal, valid), guides1 [H*W, 4] = (position, 0), src [S, H*W, 4] = (rgb, carried), S = 1 or 2, all
    contiguous float32 on the GPU -> dst [S, H*W, 4], another tensor of src's shape, which is returned.  step >= 1; the sigmas
    are >= 0, sigma_c_level may be inf (no colour term).  No gradient."""
    return _atrous_level('nefii_denoise_atrous', 'sigma_c_level', guides0, guides1, src, dst, height, width, step, sigma_n,
                         sigma_x, sigma_c_level)


# ---- per-pixel variance from the rays and the level it guides ---------------------------------------------
MOMENTS_MAX_RAYS = 4096


def pixel_moments(diffuse, albedo, specular, hit, rays):
    """The denoiser's signals with their variance (nefii_pixel_moments): diffuse, albedo, specular [P*rays, 3]
    contiguous float32 and hit [P*rays] bool or uint8 on the GPU, row p * rays + r ray r of pixel p, rays in 2 .. 4096 ->
    [2, P, 4] float32 = (diffuse / max(mean albedo, 1e-3), variance of its mean luminance) and (specular, variance), four
    zeros where a ray of the pixel missed.  fp64 sums, bitwise reproducible.  No gradient."""
    rays = int(rays)
    if not 2 <= rays <= MOMENTS_MAX_RAYS:
        raise ValueError('rays must lie in 2 .. %d (a variance needs two samples), got %d' % (MOMENTS_MAX_RAYS, rays))
    if not torch.is_tensor(diffuse) or diffuse.dim() != 2 or diffuse.shape[0] < rays or diffuse.shape[0] % rays:
        raise ValueError('diffuse must be [P * %d, 3] with P >= 1, got %s'
                         % (rays, tuple(diffuse.shape) if torch.is_tensor(diffuse) else type(diffuse).__name__))
    n = diffuse.shape[0]
    for name, t in (('diffuse', diffuse), ('albedo', albedo), ('specular', specular)):
        check_tensor(name, t, torch.float32, (n, 3))
    if torch.is_tensor(hit) and hit.dtype == torch.bool:
        check_tensor('hit', hit, torch.bool, (n,))
        hit = hit.view(torch.uint8)
    else:
        check_tensor('hit', hit, torch.uint8, (n,))
    need_gpu(diffuse, albedo, specular, hit)
    signals = torch.empty(2, n // rays, 4, dtype=torch.float32, device=diffuse.device)
    call('nefii_pixel_moments', _ptr(diffuse), _ptr(albedo), _ptr(specular), _ptr(hit), n // rays, rays, _ptr(signals))
    return signals


def denoise_atrous_variance(guides0, guides1, src, dst, height, width, step, sigma_n, sigma_x, sigma_l):
    """One level of the variance-guided a-trous filter (nefii_denoise_atrous_variance): denoise_atrous's
    buffers with src [S, H*W, 4] = (rgb, variance of the luminance's mean) -> dst, the filtered colour and the variance left,
    which is returned.  sigma_l scales the local standard deviation in the luminance stop and is the same at every level;
    inf switches the stop off.  No gradient."""
    return _atrous_level('nefii_denoise_atrous_variance', 'sigma_l', guides0, guides1, src, dst, height, width, step, sigma_n,
                         sigma_x, sigma_l)


# ---- PSNR / SSIM / MS-SSIM statistics of image pairs --------------------------------------------------
METRICS_MAX_SIDE, METRICS_MAX_BATCH, METRICS_WINDOW, METRICS_LEVELS = 16384, 65535, 11, 5
_metrics_workspaces = {}            # (device, B, H, W, C, levels) -> uint8 tensor
_metrics_window = []


def metrics_window():
    """the 11-tap Gaussian of scripts/evaluate.py:gaussian_window, formed there in double on the host, as a ctypes array"""
    if not _metrics_window:
        from ..scripts.evaluate import gaussian_window
        _metrics_window.append((ctypes.c_double * METRICS_WINDOW)(*gaussian_window().tolist()))
    return _metrics_window[0]


def image_metrics(x, y, levels, data_range=1.0):
    """The SSIM statistics and squared error of image pairs (nefii_image_metrics): x, y [B, H, W, C] contiguous
    float32 on the GPU, C in 1 .. 4; levels = 1 (SSIM) or 5 (MS-SSIM, sides above 160) -> (stats [B, levels, C, 2] float64 =
    the means of (ssim, cs) per level, sq_err [B, C] float64 = sum (x - y)^2 over the pixels), both on the GPU.  All arithmetic
    is fp64.  ValueError for a wrong dtype, layout or shape, RuntimeError for tensors that are not on the GPU.  No gradient."""
    check_tensor('x', x, torch.float32, (None, None, None, None))
    check_tensor('y', y, torch.float32, tuple(x.shape))
    B, H, W, C = x.shape
    levels = int(levels)
    if levels not in (1, METRICS_LEVELS):
        raise ValueError('levels must be 1 or %d, got %d' % (METRICS_LEVELS, levels))
    if not 1 <= C <= 4:
        raise ValueError('1 .. 4 channels, got %d' % C)
    if not 1 <= B <= METRICS_MAX_BATCH:
        raise ValueError('1 .. %d images per call, got %d' % (METRICS_MAX_BATCH, B))
    if min(H, W) < METRICS_WINDOW or max(H, W) > METRICS_MAX_SIDE:
        raise ValueError('height and width must lie in %d .. %d, got %d x %d' % (METRICS_WINDOW, METRICS_MAX_SIDE, H, W))
    if levels == METRICS_LEVELS and min(H, W) <= (METRICS_WINDOW - 1) * 2 ** 4:
        raise ValueError('MS-SSIM over five scales needs images larger than 160 pixels on their smaller side')
    data_range = float(data_range)
    if not (data_range > 0. and math.isfinite(data_range)):
        raise ValueError('data_range must be positive and finite, got %r' % data_range)
    need_gpu(x, y)
    if x.device != y.device:
        raise RuntimeError('x is on %s, y on %s' % (x.device, y.device))
    key = (x.device, B, H, W, C, levels)
    ws = _metrics_workspaces.get(key)
    if ws is None:
        n = nbytes('nefii_image_metrics_workspace_bytes', B, H, W, C, levels)
        if len(_metrics_workspaces) >= 8:               # a split has one shape; a few more for the callers that mix them
            _metrics_workspaces.clear()
        ws = _metrics_workspaces[key] = torch.empty(n // 8, dtype=torch.float64, device=x.device)
    stats = torch.empty(B, levels, C, 2, dtype=torch.float64, device=x.device)
    sq_err = torch.empty(B, C, dtype=torch.float64, device=x.device)
    call('nefii_image_metrics', _ptr(x), _ptr(y), B, H, W, C, levels, metrics_window(), (0.01 * data_range) ** 2,
         (0.03 * data_range) ** 2, _ptr(ws), _ptr(stats), _ptr(sq_err))
    return stats, sq_err
