"""The two fused losses: IDRLoss per ray and its patch terms."""
import ctypes

import torch

from .. import _lib
from ._call import _f32, _ptr, call, nbytes


class IdrLossFn(torch.autograd.Function):
    """IDRLoss value + gradient in one launch (nefii_idr_loss).  Returns losses [6] = (loss, idr_rgb_loss, sg_rgb_loss,
    mask_loss, normalsmooth_loss, background_rgb_loss); only losses[0] is differentiable, wrt idr_rgb and sg_rgb."""

    @staticmethod
    def forward(ctx, idr_rgb, sg_rgb, rgb_gt, net_mask, obj_mask, sdf_output, normals, params):
        n = sg_rgb.shape[0]
        dev = sg_rgb.device
        # the kernel reads n rows of every array: a shorter one would be read past its end
        if tuple(sg_rgb.shape) != (n, 3) or tuple(idr_rgb.shape) != (n, 3) or rgb_gt.numel() != 3 * n or \
                net_mask.numel() != n or obj_mask.numel() != n or sdf_output.numel() != n or \
                (normals is not None and tuple(normals.shape) != (n, 3)):
            raise ValueError('IdrLossFn: every input describes the same n rays')
        if params.r_patch >= 1 and params.normalsmooth_weight != 0. and n % (4 * params.r_patch * params.r_patch):
            raise ValueError('IdrLossFn: %d rays are no whole number of patches of %d (r_patch %d)'
                             % (n, 4 * params.r_patch * params.r_patch, params.r_patch))
        losses = torch.empty(6, device=dev, dtype=torch.float32)
        need_i, need_s = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d_idr = torch.empty(n, 3, device=dev, dtype=torch.float32) if need_i else None
        d_sg = torch.empty(n, 3, device=dev, dtype=torch.float32) if need_s else None
        # converted copies are bound to names: a temporary handed to _ptr() dies before the launch call is made and the
        # next temporary of the same size is given its memory
        idr_c, sg_c, gt_c = _f32(idr_rgb), _f32(sg_rgb), _f32(rgb_gt).reshape(-1, 3)
        net_c, obj_c = net_mask.to(torch.uint8).contiguous(), obj_mask.to(torch.uint8).contiguous()
        sdf_c = _f32(sdf_output).reshape(-1)
        nrm_c = _f32(normals) if normals is not None else None
        call('nefii_idr_loss', ctypes.byref(params), _ptr(idr_c), _ptr(sg_c), _ptr(gt_c), _ptr(net_c), _ptr(obj_c), _ptr(sdf_c),
             _ptr(nrm_c), n, _ptr(losses), _ptr(d_idr), _ptr(d_sg))
        ctx.save_for_backward(d_idr, d_sg)
        return losses

    @staticmethod
    def backward(ctx, g):
        d_idr, d_sg = ctx.saved_tensors
        s = g[0]
        return (d_idr * s if d_idr is not None else None, d_sg * s if d_sg is not None else None,
                None, None, None, None, None, None)


# The 11-tap Gaussian (sigma 1.5) of the reference's ssim_loss_fn (model/loss.py:8-22), which forms it in fp32: exp(-x^2 / 4.5)
# normalised by its fp32 sum.  Written out (taps 0 .. 5; the window is symmetric) because an exp that differs in the last
# bit - numpy's from torch's, one CPU's vector path from another's - moves the SSIM term by 5e-7 of itself.
_SSIM_LOSS_TAPS = [float.fromhex(h) for h in ('0x1.0d9570p-10', '0x1.f1fe02p-8', '0x1.26eb18p-5', '0x1.bff0fep-4',
                                              '0x1.b43c3ep-3', '0x1.106560p-2')]


def ssim_loss_window():
    """[11] float32 on the host"""
    return torch.tensor(_SSIM_LOSS_TAPS + _SSIM_LOSS_TAPS[-2::-1], dtype=torch.float32)


def patch_loss_params(idr_ssim_weight, sg_ssim_weight, roughnesssmooth_weight, r_patch):
    return _lib.PatchLossParams(idr_ssim_weight, sg_ssim_weight, roughnesssmooth_weight, int(r_patch),
                                (ctypes.c_float * _lib.PATCH_WINDOW)(*ssim_loss_window().tolist()), 0)


class PatchLossFn(torch.autograd.Function):
    """The patch terms of IDRLoss, value + gradient in two launches (nefii_idr_patch_loss).  Rays in patches of
    (2 r_patch)^2 consecutive rows.  Returns losses [4] = (idr_ssim_weight idr_ssim_loss + sg_ssim_weight sg_ssim_loss +
    roughnesssmooth_weight roughnesssmooth_loss, idr_ssim_loss, sg_ssim_loss, roughnesssmooth_loss); only losses[0] is
    differentiable, wrt idr_rgb, sg_rgb and roughness.  params: patch_loss_params(...)."""

    @staticmethod
    def forward(ctx, idr_rgb, sg_rgb, roughness, rgb_gt, net_mask, obj_mask, normals, params):
        n = sg_rgb.shape[0]
        dev = sg_rgb.device
        workspace = torch.empty(nbytes('nefii_idr_patch_loss_workspace_bytes', ctypes.byref(params), n) // 8, device=dev,
                                dtype=torch.float64)
        losses = torch.empty(4, device=dev, dtype=torch.float32)
        d_idr, d_sg, d_rough = [torch.empty(t.shape, device=dev, dtype=torch.float32) if need else None
                                for t, need in zip((idr_rgb, sg_rgb, roughness), ctx.needs_input_grad[:3])]
        # converted copies are bound to names (see IdrLossFn)
        idr_c, sg_c, gt_c = _f32(idr_rgb), _f32(sg_rgb), _f32(rgb_gt).reshape(-1, 3)
        net_c, obj_c = net_mask.to(torch.uint8).contiguous(), obj_mask.to(torch.uint8).contiguous()
        rough_c, nrm_c = _f32(roughness).reshape(-1), _f32(normals)
        if idr_c.shape != (n, 3) or gt_c.shape != (n, 3) or nrm_c.shape != (n, 3) or rough_c.shape != (n,) or \
                net_c.numel() != n or obj_c.numel() != n:
            raise ValueError('PatchLossFn: every input describes the same n rays')
        call('nefii_idr_patch_loss', ctypes.byref(params), _ptr(idr_c), _ptr(sg_c), _ptr(gt_c), _ptr(net_c), _ptr(obj_c),
             _ptr(rough_c), _ptr(nrm_c), n, _ptr(workspace), _ptr(losses), _ptr(d_idr), _ptr(d_sg), _ptr(d_rough))
        ctx.save_for_backward(d_idr, d_sg, d_rough)
        return losses

    @staticmethod
    def backward(ctx, g):
        s = g[0]
        return tuple(d * s if d is not None else None for d in ctx.saved_tensors) + (None, None, None, None, None)
