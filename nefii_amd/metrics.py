"""PSNR, MSE, SSIM and MS-SSIM of frames that sit in GPU memory: the numbers of scripts/evaluate.py's
calculate_psnr / calculate_mse / calculate_ssim / calculate_ms_ssim, from one ops.image_metrics call per batch.

Inputs are float32 device tensors [H, W, C] or [B, H, W, C], C in 1 .. 4.  The kernels leave per-level, per-channel means
and per-channel sums of squared differences in fp64; the reductions that remain - the relu, the weighted product over the
scales, the means over channels and pixels - are done here on the host in double, as evaluate does them.  Every function
returns a Python float for [H, W, C] input and a list of floats, one per image, for [B, H, W, C]."""
import math

import torch

from . import ops
from .scripts.evaluate import MS_WEIGHTS


def _batched(x, y):
    if not torch.is_tensor(x) or not torch.is_tensor(y):
        raise ValueError('x and y must be tensors')
    if x.dim() not in (3, 4) or tuple(x.shape) != tuple(y.shape):
        raise ValueError('x and y must be [H, W, C] or [B, H, W, C] of one shape, got %s and %s'
                         % (tuple(x.shape), tuple(y.shape)))
    single = x.dim() == 3
    return (x[None], y[None], single) if single else (x, y, single)


def _give(values, single):
    values = [float(v) for v in values]
    return values[0] if single else values


def _ssim_of(stats):
    """stats [B, levels, C, 2] on the host -> [B]: the mean over channels of level 0's mean ssim"""
    return stats[:, 0, :, 0].mean(-1)


def _ms_ssim_of(stats):
    """stats [B, 5, C, 2] on the host -> [B]: calculate_ms_ssim's relu, weighted product over the scales and channel mean"""
    vals = torch.cat([stats[:, :-1, :, 1], stats[:, -1:, :, 0]], dim=1).relu()         # cs of scales 0 .. 3, ssim of scale 4
    w = torch.tensor(MS_WEIGHTS, dtype=vals.dtype).view(1, -1, 1)
    return torch.prod(vals ** w, dim=1).mean(-1)


def _mse_of(sq_err, pixels):
    """sq_err [B, C] on the host -> [B]: the mean over all pixels and channels"""
    return sq_err.sum(-1) / (pixels * sq_err.shape[1])


def _psnr_of(mse):
    return [float('inf') if m == 0 else 20 * math.log10(1.0 / math.sqrt(m)) for m in mse.tolist()]


def _run(x, y, levels, data_range):
    x, y, single = _batched(x, y)
    if levels == ops.METRICS_LEVELS and x.dim() == 4 and min(x.shape[1:3]) <= (ops.METRICS_WINDOW - 1) * 2 ** 4:
        raise ValueError('MS-SSIM over five scales needs images larger than 160 pixels on their smaller side')
    stats, sq_err = ops.image_metrics(x, y, levels, data_range)
    return stats.cpu(), sq_err.cpu(), x.shape[1] * x.shape[2], single


def ssim(x, y, data_range=1.0):
    stats, _, _, single = _run(x, y, 1, data_range)
    return _give(_ssim_of(stats), single)


def ms_ssim(x, y, data_range=1.0):
    """ValueError unless the smaller side exceeds 160 (evaluate's rule)"""
    stats, _, _, single = _run(x, y, ops.METRICS_LEVELS, data_range)
    return _give(_ms_ssim_of(stats), single)


def ssim_and_ms_ssim(x, y, data_range=1.0):
    """(ssim, ms_ssim) from one five-level call: level 0 is shared"""
    stats, _, _, single = _run(x, y, ops.METRICS_LEVELS, data_range)
    return _give(_ssim_of(stats), single), _give(_ms_ssim_of(stats), single)


def mse(x, y):
    _, sq_err, pixels, single = _run(x, y, 1, 1.0)
    return _give(_mse_of(sq_err, pixels), single)


def psnr(x, y):
    """for images in [0, 1], as calculate_psnr; inf for identical images"""
    _, sq_err, pixels, single = _run(x, y, 1, 1.0)
    return _give(_psnr_of(_mse_of(sq_err, pixels)), single)


def all_metrics(x, y, data_range=1.0):
    """{'psnr', 'mse', 'ssim', 'ms_ssim'} from ONE call; ms_ssim is nan where the smaller side does not exceed 160"""
    xb, yb, single = _batched(x, y)
    five = xb.dim() == 4 and min(xb.shape[1:3]) > (ops.METRICS_WINDOW - 1) * 2 ** 4
    stats, sq_err, pixels, _ = _run(xb, yb, ops.METRICS_LEVELS if five else 1, data_range)
    m = _mse_of(sq_err, pixels)
    return {'psnr': _give(_psnr_of(m), single), 'mse': _give(m, single), 'ssim': _give(_ssim_of(stats), single),
            'ms_ssim': _give(_ms_ssim_of(stats) if five else [float('nan')] * xb.shape[0], single)}
