"""IDRLoss with the reference's constructor and output dict (code/model/loss.py:123-320).

Runs as torch ops on <= num_pixels x 3 floats (SURVEY.md section 8f ranks fusing it with Adam as the first
"next" item), or - frozen geometry, inputs on the GPU - as the fused kernels of ops.IdrLossFn and ops.PatchLossFn.
The patch terms (SSIM of both colours, roughness-smoothness: DESIGN.md 6n) are computed only when their weight is
non-zero; the view-diff term is not built and raises NotImplementedError when weighted."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class IDRLoss(nn.Module):
    MIN_SSIM_R_PATCH = 6        # the 11-tap window needs a patch side of at least 11, and r_patch = 5.5 does not exist
    MAX_FUSED_R_PATCH = 16      # ops.PatchLossFn keeps a patch in static LDS: side <= 32; larger patches run as torch ops

    def __init__(self, idr_rgb_weight, sg_rgb_weight, eikonal_weight, mask_weight, alpha, r_patch=-1,
                 normalsmooth_weight=0., loss_type='L1', env_loss_type='L1', idr_ssim_weight=0., sg_ssim_weight=0.,
                 view_diff_weight=0., roughnesssmooth_weight=0., background_rgb_weight=0., view_diff_full_rgb=True,
                 sample_each_iter=False):
        super().__init__()
        if view_diff_weight:
            raise NotImplementedError('view_diff_weight: the view-diff term needs the reference\'s PixelPairGenerator '
                                      '(depth re-projection between views), which is not built')
        if (idr_ssim_weight or sg_ssim_weight) and 1 <= int(r_patch) < self.MIN_SSIM_R_PATCH:
            raise ValueError('idr_ssim_weight / sg_ssim_weight need r_patch >= %d (or < 1, which switches the patch terms '
                             'off): a patch of side 2 r_patch <= 10 has no position the 11-tap SSIM window fits, and the '
                             'reference stops with an IndexError at its first step' % self.MIN_SSIM_R_PATCH)
        self.idr_ssim_weight = idr_ssim_weight
        self.sg_ssim_weight = sg_ssim_weight
        self.roughnesssmooth_weight = roughnesssmooth_weight
        self.idr_rgb_weight = idr_rgb_weight
        self.sg_rgb_weight = sg_rgb_weight
        self.background_rgb_weight = background_rgb_weight
        self.eikonal_weight = eikonal_weight
        self.mask_weight = mask_weight
        self.alpha = alpha
        if loss_type not in ('L1', 'L2', 'L1_smooth'):
            raise Exception('Unknown loss_type!')
        if env_loss_type not in ('L1', 'L2'):
            raise Exception('Unknown env_loss_type!')
        self.loss_type = loss_type
        self.env_loss_type = env_loss_type
        self.r_patch = int(r_patch)
        self.normalsmooth_weight = normalsmooth_weight
        self.fused = True       # one-launch HIP kernel for value + gradient when the inputs live on the GPU

    @staticmethod
    def _zero(ref):
        return torch.zeros((), device=ref.device, dtype=torch.float32)

    # Masked reductions are written as (sum of masked terms) / max(count, 1): the same values as the reference's
    # boolean-index + mean formulation, without its data-dependent shapes - no host synchronisation per term.
    @staticmethod
    def _masked_mean(per_elem, mask, width):
        cnt = mask.sum()
        return (per_elem * mask.unsqueeze(-1)).sum() / torch.clamp(cnt * width, min=1)

    def _img_err(self, a, b, kind):
        d = a - b
        if kind == 'L1':
            return d.abs()
        if kind == 'L2':
            return d * d
        ad = d.abs()          # SmoothL1, beta = 1
        return torch.where(ad < 1.0, 0.5 * d * d, ad - 0.5)

    def get_rgb_loss(self, idr_rgb_values, sg_rgb_values, rgb_gt, network_object_mask, object_mask):
        mask = (network_object_mask & object_mask).to(rgb_gt.dtype)
        gt = rgb_gt.reshape(-1, 3)
        return (self._masked_mean(self._img_err(idr_rgb_values, gt, self.loss_type), mask, 3),
                self._masked_mean(self._img_err(sg_rgb_values, gt, self.loss_type), mask, 3))

    def get_background_rgb_loss(self, sg_rgb_values, rgb_gt, network_object_mask, object_mask):
        if self.background_rgb_weight <= 0:
            return self._zero(rgb_gt)
        mask = ((~network_object_mask) & (~object_mask)).to(rgb_gt.dtype)
        return self._masked_mean(self._img_err(sg_rgb_values, rgb_gt.reshape(-1, 3), self.env_loss_type), mask, 3)

    def get_eikonal_loss(self, grad_theta, ref):
        if grad_theta is None or grad_theta.shape[0] == 0:
            return self._zero(ref)
        return ((grad_theta.norm(2, dim=1) - 1) ** 2).mean()

    def get_mask_loss(self, sdf_output, network_object_mask, object_mask):
        mask = (~(network_object_mask & object_mask)).to(sdf_output.dtype)
        sdf_pred = (-self.alpha * sdf_output).squeeze(-1)
        bce = F.binary_cross_entropy_with_logits(sdf_pred, object_mask.to(sdf_output.dtype), reduction='none')
        return (1 / self.alpha) * (bce * mask).sum() / float(object_mask.shape[0])

    def get_normalsmooth_loss(self, normal, network_object_mask, object_mask):
        if self.r_patch < 1 or self.normalsmooth_weight == 0.:
            return self._zero(normal)
        k = 4 * self.r_patch * self.r_patch
        mask = (network_object_mask & object_mask).reshape(-1, k).all(dim=-1).to(normal.dtype)
        var = torch.var(normal.view((-1, k, 3)), dim=1)
        return self._masked_mean(var, mask, 3)

    def _patch_terms_on(self):
        return self.r_patch >= 1 and (self.idr_ssim_weight != 0. or self.sg_ssim_weight != 0. or
                                      self.roughnesssmooth_weight != 0.)

    @staticmethod
    def _ssim_window(ref):
        """ssim_loss_fn's 11-tap Gaussian (sigma 1.5): the reference's fp32 taps, then cast"""
        from ..ops import ssim_loss_window
        return ssim_loss_window().to(device=ref.device, dtype=ref.dtype)

    @staticmethod
    def _ssim_term(x, y, eroded, win):
        """x, y [N, 3, P, P], eroded [N, 1, P, P] in {0, 1} -> sum(e (1 - S)) / max(sum e, 1): the reference's
        1 - mean(S[e]) with S padded by ones (the ring of 5 pixels counts in the denominator alone), 0 when nothing is left"""
        col, row = win.view(1, 1, -1, 1).expand(3, 1, -1, 1), win.view(1, 1, 1, -1).expand(3, 1, 1, -1)
        filt = lambda a: F.conv2d(F.conv2d(a, col, groups=3), row, groups=3)
        mu1, mu2 = filt(x), filt(y)
        s11, s22, s12 = filt(x * x) - mu1 * mu1, filt(y * y) - mu2 * mu2, filt(x * y) - mu1 * mu2
        C1, C2 = 0.01 ** 2, 0.03 ** 2
        cs = (2 * s12 + C2) / (s11 + s22 + C2)
        S = ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs).mean(dim=1, keepdim=True)
        return (eroded[:, :, 5:-5, 5:-5] * (1 - S)).sum() / torch.clamp(eroded.sum(), min=1)

    def get_ssim_loss(self, idr_rgb_values, sg_rgb_values, rgb_gt, network_object_mask, object_mask):
        if self.r_patch < 1 or (self.idr_ssim_weight == 0. and self.sg_ssim_weight == 0.):
            return self._zero(rgb_gt), self._zero(rgb_gt)
        P = 2 * self.r_patch
        img = lambda a: a.reshape(-1, P, P, 3).permute(0, 3, 1, 2)
        mask = (network_object_mask & object_mask).to(rgb_gt.dtype).reshape(-1, 1, P, P)
        # erosion by the 11 x 11 window clipped to the patch (max_pool2d pads with -inf: what lies outside never erodes)
        eroded = -F.max_pool2d(-mask, 11, stride=1, padding=5)
        win = self._ssim_window(rgb_gt)
        gt = img(rgb_gt)
        return self._ssim_term(img(idr_rgb_values), gt, eroded, win), self._ssim_term(img(sg_rgb_values), gt, eroded, win)

    def get_roughnesssmooth_loss(self, roughness, normal, network_object_mask, object_mask):
        if self.r_patch < 1 or self.roughnesssmooth_weight == 0.:
            return self._zero(roughness)
        k = 4 * self.r_patch * self.r_patch
        mask = (network_object_mask & object_mask).reshape(-1, k).all(dim=-1).to(roughness.dtype)
        rough_var = torch.var(roughness.reshape(-1, k), dim=1)
        normal_var = torch.var(normal.detach().reshape(-1, k, 3), dim=1).mean(dim=-1)
        return (mask * rough_var * (4 - normal_var)).sum() / torch.clamp(mask.sum(), min=1)

    def _fused(self, model_outputs, ground_truth):
        """All terms and d loss / d (idr_rgb, sg_rgb) in one kernel launch (ops.IdrLossFn); the torch formulation below
        is ~45 launches of a few microseconds each on the step's critical path."""
        from .. import ops
        from .._lib import LossParams
        kinds = {'L1': 0, 'L2': 1, 'L1_smooth': 2}
        p = LossParams(self.idr_rgb_weight, self.sg_rgb_weight, self.mask_weight, self.alpha, self.normalsmooth_weight,
                       self.background_rgb_weight, kinds[self.loss_type], kinds[self.env_loss_type], self.r_patch, 0)
        idr_rgb = model_outputs['idr_rgb_values']
        if self.idr_rgb_weight == 0 and self.idr_ssim_weight == 0:
            idr_rgb = idr_rgb.detach()      # see forward()
        lo = ops.IdrLossFn.apply(idr_rgb, model_outputs['sg_rgb_values'], ground_truth['rgb'],
                                 model_outputs['network_object_mask'], model_outputs['object_mask'],
                                 model_outputs['sdf_output'].detach(), model_outputs['normal_values'].detach(), p)
        zero = self._zero(lo)
        d = lo.detach()
        loss, idr_ssim, sg_ssim = lo[0], zero, zero
        if self._patch_terms_on():          # two more launches (ops.PatchLossFn); nothing new runs with the three weights at 0
            pp = ops.patch_loss_params(self.idr_ssim_weight, self.sg_ssim_weight, self.roughnesssmooth_weight, self.r_patch)
            pl = ops.PatchLossFn.apply(idr_rgb, model_outputs['sg_rgb_values'], model_outputs['sg_roughness_values'],
                                       ground_truth['rgb'], model_outputs['network_object_mask'],
                                       model_outputs['object_mask'], model_outputs['normal_values'].detach(), pp)
            loss = loss + pl[0]
            idr_ssim, sg_ssim = pl.detach()[1], pl.detach()[2]
        return {'loss': loss, 'idr_rgb_loss': d[1], 'sg_rgb_loss': d[2], 'eikonal_loss': zero, 'mask_loss': d[3],
                'normalsmooth_loss': d[4], 'idr_ssim_loss': idr_ssim, 'sg_ssim_loss': sg_ssim, 'view_diff_loss': zero,
                'background_rgb_loss': d[5]}

    def forward(self, model_outputs, ground_truth):
        sg = model_outputs['sg_rgb_values']
        if self.fused and sg.is_cuda and model_outputs['grad_theta'] is None and \
                not model_outputs['sdf_output'].requires_grad and not model_outputs['normal_values'].requires_grad and \
                not (self._patch_terms_on() and self.r_patch > self.MAX_FUSED_R_PATCH):
            return self._fused(model_outputs, ground_truth)
        rgb_gt = ground_truth['rgb']
        net = model_outputs['network_object_mask']
        obj = model_outputs['object_mask']
        idr_rgb = model_outputs['idr_rgb_values']
        if self.idr_rgb_weight == 0 and self.idr_ssim_weight == 0:
            # a zero-weighted term contributes exact zeros to every gradient; detaching it skips the radiance
            # network's backward pass instead of running it on zeros (physg.conf: idr_rgb_weight = 0.0)
            idr_rgb = idr_rgb.detach()
        idr_rgb_loss, sg_rgb_loss = self.get_rgb_loss(idr_rgb, model_outputs['sg_rgb_values'], rgb_gt, net, obj)
        mask_loss = self.get_mask_loss(model_outputs['sdf_output'], net, obj)
        eikonal_loss = self.get_eikonal_loss(model_outputs['grad_theta'], rgb_gt)
        normalsmooth_loss = self.get_normalsmooth_loss(model_outputs['normal_values'], net, obj)
        background_rgb_loss = self.get_background_rgb_loss(model_outputs['sg_rgb_values'], rgb_gt, net, obj)
        zero = self._zero(rgb_gt)
        loss = self.idr_rgb_weight * idr_rgb_loss + self.sg_rgb_weight * sg_rgb_loss + \
            self.eikonal_weight * eikonal_loss + self.mask_weight * mask_loss + \
            self.normalsmooth_weight * normalsmooth_loss + self.background_rgb_weight * background_rgb_loss
        idr_ssim_loss = sg_ssim_loss = zero
        if self._patch_terms_on():
            idr_ssim_loss, sg_ssim_loss = self.get_ssim_loss(idr_rgb, model_outputs['sg_rgb_values'], rgb_gt, net, obj)
            roughnesssmooth_loss = self.get_roughnesssmooth_loss(model_outputs['sg_roughness_values'],
                                                                 model_outputs['normal_values'], net, obj)
            loss = loss + self.idr_ssim_weight * idr_ssim_loss + self.sg_ssim_weight * sg_ssim_loss + \
                self.roughnesssmooth_weight * roughnesssmooth_loss
        return {'loss': loss, 'idr_rgb_loss': idr_rgb_loss, 'sg_rgb_loss': sg_rgb_loss, 'eikonal_loss': eikonal_loss,
                'mask_loss': mask_loss, 'normalsmooth_loss': normalsmooth_loss, 'idr_ssim_loss': idr_ssim_loss,
                'sg_ssim_loss': sg_ssim_loss, 'view_diff_loss': zero, 'background_rgb_loss': background_rgb_loss}
