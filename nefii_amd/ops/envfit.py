"""Fitting light SGs to an environment map (envmaps/fit_envmap_with_sg.py)."""
import torch

from .. import _lib
from ._call import _ptr, call, need_gpu
from .shading import MAX_LOBES, check_light


ENVFIT_MAX_LOBES = MAX_LOBES


def _envfit_args(lgt, dirs, target):
    check_light(lgt)
    if dirs.dim() != 2 or dirs.shape[1] != 3 or target.shape != dirs.shape or dirs.shape[0] == 0:
        raise ValueError('dirs and target must both be [n, 3], got %s and %s' % (tuple(dirs.shape), tuple(target.shape)))
    need_gpu(lgt, dirs, target)
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in (lgt, dirs, target)):
        raise RuntimeError('envfit needs contiguous float32 tensors')


def envfit_workspace(n, n_lobes, device):
    """the slab workspace of nefii_envfit_loss_grad / nefii_envfit_adam, reusable across calls of the same shape"""
    nbytes = _lib.lib().nefii_envfit_workspace_bytes(n, n_lobes)
    if nbytes <= 0:
        raise ValueError('bad envfit shape: n=%d, n_lobes=%d' % (n, n_lobes))
    return torch.empty(nbytes // 4, device=device, dtype=torch.float32)


def envfit_loss_grad(lgt, dirs, target, eps=1e-8, want_rgb=False, workspace=None):
    """(loss [], grad [M, 7]) of mean((SG2Envmap(lgt) - target)^2) over directions dirs [n, 3] (target [n, 3]); with
    want_rgb also the fitted map [n, 3]: (loss, grad, rgb).  One fused, deterministic kernel pair."""
    _envfit_args(lgt, dirs, target)
    n, M = dirs.shape[0], lgt.shape[0]
    ws = envfit_workspace(n, M, dirs.device) if workspace is None else workspace
    loss = torch.empty((), device=dirs.device, dtype=torch.float32)
    grad = torch.empty_like(lgt)
    rgb = torch.empty_like(dirs) if want_rgb else None
    call('nefii_envfit_loss_grad', _ptr(lgt), M, _ptr(dirs), _ptr(target), n, eps, _ptr(ws), _ptr(loss), _ptr(grad), _ptr(rgb))
    return (loss, grad, rgb) if want_rgb else (loss, grad)


def envfit_adam(lgt, exp_avg, exp_avg_sq, dirs, target, step0, iters, lr=1e-2, betas=(0.9, 0.999), adam_eps=1e-8,
                eps=1e-8, workspace=None):
    """`iters` fit iterations with torch.optim.Adam's update applied IN PLACE to lgt / exp_avg / exp_avg_sq (updates
    step0 + 1 ... step0 + iters), no host synchronisation; returns the losses [iters] on the device, entry i the loss
    before update step0 + i + 1."""
    _envfit_args(lgt, dirs, target)
    for t in (exp_avg, exp_avg_sq):
        if t.shape != lgt.shape:
            raise ValueError('Adam state must have the shape of lgtSGs')
        _ptr(t)
    if iters < 0 or step0 < 0:
        raise ValueError('iters and step0 must be >= 0')
    n, M = dirs.shape[0], lgt.shape[0]
    ws = envfit_workspace(n, M, dirs.device) if workspace is None else workspace
    losses = torch.empty(iters, device=dirs.device, dtype=torch.float32)
    if iters:
        call('nefii_envfit_adam', _ptr(lgt), _ptr(exp_avg), _ptr(exp_avg_sq), M, _ptr(dirs), _ptr(target), n, eps, lr, betas[0],
             betas[1], adam_eps, step0, iters, _ptr(ws), _ptr(losses))
    return losses
