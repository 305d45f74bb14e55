"""Denoising of Monte-Carlo frames with a feature-guided a-trous wavelet filter (Dammertz et al. 2010).

The renderer hands out, per pixel and free of noise, the normal, the world position, the albedo and the all-rays-hit mask,
and keeps diffuse and specular light apart.  The filter (csrc/nefii_denoise.hip, one launch per level) smooths the
demodulated diffuse light E = diffuse / max(albedo, 1e-3) and the specular light over 5 x 5 taps at steps 1, 2, 4, ...,
stopped by normal, tangent-plane and luminance differences; the texture comes back with the albedo afterwards.

    den = Denoiser(out['normal_values'], out['points'], out['network_object_mask'], img_res)
    clean = den.filter(signals)                         # [S, H, W, 3], S = 1 or 2
    out = denoise_outputs(out, img_res)                 # the frame-level step on a merged render_frame dict

With per-pixel variances from the rays (IDRNetwork.pixel_moments = True adds out['denoise_signals']) the
luminance stop is scaled by the local standard deviation and the variance is filtered along (the same file's variance-guided
level):

    clean4 = den.filter_variance(signals4)              # [S, H, W, 4] = (rgb, variance left)
    out = denoise_outputs(out, img_res, variance=True)

Evaluation only: nothing here carries a gradient."""
import torch

from . import ops

DEFAULTS = dict(levels=5, sigma_n=32., sigma_x=0.1, sigma_c=1.)
VARIANCE_DEFAULTS = dict(levels=5, sigma_n=32., sigma_x=0.1, sigma_l=4.)
MAX_LEVELS = 8
ALBEDO_FLOOR = 1e-3                 # NEFII_ALBEDO_FLOOR of include/nefii_amd.h


def check_levels(levels):
    if int(levels) != levels or not 1 <= int(levels) <= MAX_LEVELS:
        raise ValueError('denoise levels must be an integer in 1 .. %d, got %r' % (MAX_LEVELS, levels))
    return int(levels)


class Denoiser:
    """The guides of one view, packed once: every filter call on this view (the angles of a light turntable) reuses them."""

    def __init__(self, normal, points, valid, img_res):
        H, W = int(img_res[0]), int(img_res[1])
        n = H * W
        normal, points, valid = normal.detach().reshape(-1, 3), points.detach().reshape(-1, 3), valid.detach().reshape(-1)
        if normal.shape[0] != n or points.shape[0] != n or valid.shape[0] != n:
            raise ValueError('one view per call: normal / points [H*W, 3] and valid [H*W] for img_res %d x %d, got %d, %d, %d'
                             % (H, W, normal.shape[0], points.shape[0], valid.shape[0]))
        normal = normal.to(torch.float32)
        unit = normal / normal.norm(dim=1, keepdim=True).clamp_min(1e-12)
        self.img_res = (H, W)
        self.valid = valid.bool()
        self.guides0 = torch.cat([unit, self.valid.to(torch.float32)[:, None]], dim=1).contiguous()
        self.guides1 = torch.cat([points.to(torch.float32), torch.zeros_like(unit[:, :1])], dim=1).contiguous()

    def _signal_count(self, name, signals, lanes):
        """S of signals [S, H, W, lanes] (or [S, H*W, lanes]), S = 1 or 2; ValueError for any other shape"""
        H, W = self.img_res
        if signals.dim() not in (3, 4) or signals.shape[0] not in (1, 2) or signals.shape[-1] != lanes \
                or signals[0].numel() != H * W * lanes:
            raise ValueError('%s must be [S, %d, %d, %d] with S = 1 or 2, got %s' % (name, H, W, lanes, tuple(signals.shape)))
        return signals.shape[0]

    def _cascade(self, level, src, levels, sigma_n, sigma_x, sigma_3_of_level):
        """`levels` launches of `level` (ops.denoise_atrous or ops.denoise_atrous_variance) at steps 1, 2, 4, ... between src
        [S, H*W, 4], which is overwritten, and a second buffer -> the one that holds the last level's output"""
        H, W = self.img_res
        dst = torch.empty_like(src)
        for l in range(levels):
            level(self.guides0, self.guides1, src, dst, H, W, 1 << l, sigma_n, sigma_x, sigma_3_of_level(l))
            src, dst = dst, src
        return src

    def filter(self, signals, levels=DEFAULTS['levels'], sigma_n=DEFAULTS['sigma_n'], sigma_x=DEFAULTS['sigma_x'],
               sigma_c=DEFAULTS['sigma_c']):
        """signals [S, H, W, 3] (or [S, H*W, 3]), S = 1 or 2 -> the filtered signals [S, H, W, 3] after `levels` levels"""
        levels = check_levels(levels)
        H, W = self.img_res
        S = self._signal_count('signals', signals, 3)
        src = torch.zeros(S, H * W, 4, device=signals.device, dtype=torch.float32)
        src[:, :, :3] = signals.detach().reshape(S, H * W, 3)
        out = self._cascade(ops.denoise_atrous, src, levels, sigma_n, sigma_x, lambda l: float(sigma_c) * 2. ** -l)
        return out[:, :, :3].reshape(S, H, W, 3)

    def filter_variance(self, signals4, levels=VARIANCE_DEFAULTS['levels'], sigma_n=VARIANCE_DEFAULTS['sigma_n'],
                        sigma_x=VARIANCE_DEFAULTS['sigma_x'], sigma_l=VARIANCE_DEFAULTS['sigma_l']):
        """signals4 [S, H, W, 4] (or [S, H*W, 4]) = (rgb, variance of the luminance's mean: ops.pixel_moments), S = 1 or 2 ->
        the filtered [S, H, W, 4], colour and the variance left, after `levels` variance-guided levels"""
        levels = check_levels(levels)
        H, W = self.img_res
        S = self._signal_count('signals4', signals4, 4)
        src = signals4.detach().to(torch.float32).reshape(S, H * W, 4).clone(memory_format=torch.contiguous_format)
        out = self._cascade(ops.denoise_atrous_variance, src, levels, sigma_n, sigma_x, lambda l: sigma_l)
        return out.reshape(S, H, W, 4)


def denoise_outputs(model_outputs, img_res, denoiser=None, variance=False, **params):
    """The frame-level step on the merged outputs of one view (training/render.render_frame): a NEW dict in which
    sg_diffuse_rgb_values = albedo * filtered(diffuse / max(albedo, 1e-3)), sg_specular_rgb_values = filtered(specular) and
    sg_rgb_values = their sum on the pixels of network_object_mask; the other pixels keep all three bitwise, and every other
    key is the same tensor.  denoiser: this view's Denoiser (built from the outputs when None); params: Denoiser.filter's.
    variance=True: the signals and their variances are model_outputs['denoise_signals'] [H*W, 8] = (diffuse
    light rgb, v, specular rgb, v), which a model with pixel_moments = True renders; params are Denoiser.filter_variance's,
    and the new dict also carries 'denoise_variance' [H*W, 2], the two variances the filter leaves."""
    H, W = int(img_res[0]), int(img_res[1])
    if variance and 'denoise_signals' not in model_outputs:
        raise ValueError("denoise_outputs(variance=True) needs model_outputs['denoise_signals']: render with "
                         'model.pixel_moments = True (ops.pixel_moments on the per-ray buffers) and pass '
                         "extra_keys=(('denoise_signals', 8),) to render_frame")
    diffuse, specular = model_outputs['sg_diffuse_rgb_values'], model_outputs['sg_specular_rgb_values']
    if diffuse.dim() != 2 or diffuse.shape[0] != H * W:
        raise ValueError('one view per call: the outputs hold %s rows, img_res %d x %d needs %d'
                         % (diffuse.shape[0] if diffuse.dim() else '?', H, W, H * W))
    if denoiser is None:
        denoiser = Denoiser(model_outputs['normal_values'], model_outputs['points'], model_outputs['network_object_mask'],
                            img_res)
    elif tuple(denoiser.img_res) != (H, W):
        raise ValueError('the denoiser was built for %d x %d, not %d x %d' % (denoiser.img_res + (H, W)))
    albedo = model_outputs['sg_diffuse_albedo_values'].float()
    left = None
    if variance:
        signals4 = model_outputs['denoise_signals']
        if signals4.dim() != 2 or tuple(signals4.shape) != (H * W, 8):
            raise ValueError("model_outputs['denoise_signals'] must be [%d, 8], got %s" % (H * W, tuple(signals4.shape)))
        clean4 = denoiser.filter_variance(signals4.float().reshape(H * W, 2, 4).transpose(0, 1), **params).reshape(2, H * W, 4)
        clean, left = clean4[:, :, :3], clean4[:, :, 3].t().contiguous()
    else:
        light = diffuse.float() / albedo.clamp_min(ALBEDO_FLOOR)
        clean = denoiser.filter(torch.stack([light, specular.float()]), **params).reshape(2, H * W, 3)
    valid = denoiser.valid[:, None]
    new_diffuse = torch.where(valid, (albedo * clean[0]).to(diffuse.dtype), diffuse)
    new_specular = torch.where(valid, clean[1].to(specular.dtype), specular)
    out = dict(model_outputs)
    out['sg_diffuse_rgb_values'] = new_diffuse
    out['sg_specular_rgb_values'] = new_specular
    out['sg_rgb_values'] = torch.where(valid, new_diffuse + new_specular, model_outputs['sg_rgb_values'])
    if left is not None:
        out['denoise_variance'] = left
    return out
