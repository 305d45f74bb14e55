"""Whole-frame kernels: the a-trous denoiser and the PSNR / SSIM / MS-SSIM statistics."""
import ctypes
import math
import struct

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


# ---- adaptive sampling of Monte-Carlo frames ---------------------------------------------------------------
ADAPTIVE_MAX_COLUMNS, ADAPTIVE_MAX_ROUNDS, ADAPTIVE_MAX_PIXELS = 64, 65536, 2 ** 31 - 1
LAMBDA_BITS_END = 0x7F800000         # the bit pattern of +inf: one past FLT_MAX's


def _rounds(name, v, top):
    v = int(v)
    if not 1 <= v <= top:
        raise ValueError('%s must lie in 1 .. %d, got %d' % (name, top, v))
    return v


def ray_luminance_moments(rgb, rays):
    """A round's noise estimate per pixel (nefii_ray_luminance_moments): rgb [P*rays, 3] contiguous float32 on the
    GPU, row p * rays + r ray r of pixel p, rays in 1 .. 4096 -> [P, 2] float32 = (Rec. 709 luminance of the mean colour, sum
    of the squared deviations of the rays' luminances from it).  Two fp64 passes, bitwise reproducible.  No gradient."""
    rays = _rounds('rays', rays, MOMENTS_MAX_RAYS)
    if not torch.is_tensor(rgb) or rgb.dim() != 2 or rgb.shape[0] < rays or rgb.shape[0] % rays:
        raise ValueError('rgb must be [P * %d, 3] with P >= 1, got %s'
                         % (rays, tuple(rgb.shape) if torch.is_tensor(rgb) else type(rgb).__name__))
    check_tensor('rgb', rgb, torch.float32, (rgb.shape[0], 3))
    need_gpu(rgb)
    out = torch.empty(rgb.shape[0] // rays, 2, dtype=torch.float32, device=rgb.device)
    call('nefii_ray_luminance_moments', _ptr(rgb), rgb.shape[0] // rays, rays, _ptr(out))
    return out


def _check_state(sum_, stat):
    """sum [P, C] and stat [P, 3] float64 of one frame -> (P, C)"""
    check_tensor('sum', sum_, torch.float64, (None, None))
    P, C = sum_.shape
    if not (1 <= P <= ADAPTIVE_MAX_PIXELS and 1 <= C <= ADAPTIVE_MAX_COLUMNS):
        raise ValueError('sum must be [P, C] with P >= 1 and C in 1 .. %d, got %s' % (ADAPTIVE_MAX_COLUMNS, tuple(sum_.shape)))
    check_tensor('stat', stat, torch.float64, (P, 3))
    return P, C


def adaptive_merge(rows, pixel, rays, sum_, stat):
    """Adds one round to a frame's running state (nefii_adaptive_merge): rows [m, C + 2] contiguous float32 =
    the round's C packed means over `rays` rays and its (ebar, M2) of ray_luminance_moments; pixel [m] int32, strictly
    increasing in [0, P), or None for rows of all P pixels; sum_ [P, C] and stat [P, 3] = (n, mean, M2) float64, updated in
    place: sum_ += rays * row, stat by the pairwise rule.  Any split of the rows into calls gives the same bits."""
    rays = _rounds('rays', rays, MOMENTS_MAX_RAYS)
    P, C = _check_state(sum_, stat)
    check_tensor('rows', rows, torch.float32, (None, C + 2))
    m = rows.shape[0]
    if not 1 <= m <= P:
        raise ValueError('rows must hold 1 .. %d rows, got %d' % (P, m))
    if pixel is None:
        if m != P:
            raise ValueError('pixel is None: rows must hold all %d pixels, got %d' % (P, m))
    else:
        check_tensor('pixel', pixel, torch.int32, (m,))
        if int(pixel[0]) < 0 or int(pixel[-1]) >= P or (m > 1 and not bool((pixel[1:] > pixel[:-1]).all())):
            raise ValueError('pixel must be strictly increasing within [0, %d)' % P)
    need_gpu(rows, sum_, stat, *(() if pixel is None else (pixel,)))
    call('nefii_adaptive_merge', _ptr(rows), _ptr(pixel), m, P, C, rays, _ptr(sum_), _ptr(stat))


def adaptive_score(stat, height, width, eps, dilate=True):
    """The allocation's per-pixel score (nefii_adaptive_score): stat [H*W, 3] float64 = (n, mean, M2) ->
    [H*W] float32, the relative standard deviation sqrt(M2 / (n - 1)) / (|mean| + eps), 0 where n < 2 or it is not finite;
    with dilate the maximum over the 3 x 3 pixels around each pixel that lie in the image."""
    height, width = int(height), int(width)
    if not (1 <= height <= DENOISE_MAX_SIDE and 1 <= width <= DENOISE_MAX_SIDE):
        raise ValueError('height and width must lie in 1 .. %d, got %d x %d' % (DENOISE_MAX_SIDE, height, width))
    eps = float(eps)
    if not (eps > 0. and math.isfinite(eps)):
        raise ValueError('eps must be positive and finite, got %r' % eps)
    check_tensor('stat', stat, torch.float64, (height * width, 3))
    need_gpu(stat)
    score = torch.empty(height * width, dtype=torch.float32, device=stat.device)
    call('nefii_adaptive_score', _ptr(stat), height, width, eps, int(bool(dilate)), _ptr(score))
    return score


def _lambda_of(bits):
    return struct.unpack('<f', struct.pack('<I', bits))[0]


def adaptive_allocate(score, budget_rounds, max_rounds):
    """Rounds per pixel under a budget (nefii_adaptive_count / nefii_adaptive_targets): score [P] contiguous
    float32 on the GPU, budget_rounds = N >= P, max_rounds = K -> (k [P] int32, lambda, T): k_p = min(K, max(1,
    ceil(fl32(lambda * score_p)))) for the largest finite lambda >= 0 whose total T = sum k_p is at most N, found by bisection
    on lambda's bit pattern: at most 31 counts, each read back by the host."""
    K = _rounds('max_rounds', max_rounds, ADAPTIVE_MAX_ROUNDS)
    check_tensor('score', score, torch.float32, (None,))
    P = score.shape[0]
    N = int(budget_rounds)
    if not 1 <= P <= ADAPTIVE_MAX_PIXELS:
        raise ValueError('score must hold 1 .. 2^31 - 1 pixels, got %d' % P)
    if N < P:
        raise ValueError('budget_rounds must cover one round per pixel: %d < %d' % (N, P))
    need_gpu(score)
    totals = torch.zeros(32, dtype=torch.int64, device=score.device)

    def count(bits, slot):
        call('nefii_adaptive_count', _ptr(score), P, _lambda_of(bits), K, totals.data_ptr() + 8 * slot)
        return int(totals[slot])
    lo, hi, T, slot = 0, LAMBDA_BITS_END, P, 0          # T(0) = P <= N; hi is never evaluated
    while hi - lo > 1:
        mid = (lo + hi) // 2
        t = count(mid, slot)
        slot += 1
        if t <= N:
            lo, T = mid, t
        else:
            hi = mid
    lam = _lambda_of(lo)
    k = torch.empty(P, dtype=torch.int32, device=score.device)
    call('nefii_adaptive_targets', _ptr(score), P, lam, K, _ptr(k))
    return k, lam, T


def adaptive_finalise(sum_, stat, mask_columns=()):
    """The merged frame (nefii_adaptive_finalise): sum_ [P, C], stat [P, 3] float64 of adaptive_merge ->
    (out [P, C] float32 = sum / n - in the columns listed in mask_columns 1 where sum == n else 0: mean_pixel's all() over every
    ray of every round -, rays [P] int32 = n, variance [P] float32 = M2 / (n (n - 1)), the variance of the mean luminance)."""
    P, C = _check_state(sum_, stat)
    word = 0
    for c in mask_columns:
        if not 0 <= int(c) < C:
            raise ValueError('mask column %d is outside 0 .. %d' % (int(c), C - 1))
        word |= 1 << int(c)
    need_gpu(sum_, stat)
    out = torch.empty(P, C, dtype=torch.float32, device=sum_.device)
    rays = torch.empty(P, dtype=torch.int32, device=sum_.device)
    variance = torch.empty(P, dtype=torch.float32, device=sum_.device)
    call('nefii_adaptive_finalise', _ptr(sum_), _ptr(stat), P, C, word, _ptr(out), _ptr(rays), _ptr(variance))
    return out, rays, variance


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
