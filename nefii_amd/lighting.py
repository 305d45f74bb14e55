"""Spherical-Gaussian lights from HDR environment maps (envmaps/fit_envmap_with_sg.py, envmaps/rotate_lightsg.py).

    fitter = SGEnvmapFitter(target, dirs, num_lobes=128)     # target / dirs [H, W, 3] or [n, 3], on the GPU
    losses = fitter.fit(1000)                                # the loss before each update, on the host
    np.save('sg_128.npy', fitter.lgtSGs.cpu().numpy())       # a light for EnvmapMaterialNetwork.load_light

The fit itself runs in libnefii_hip.so (ops.envfit_adam: one fused, deterministic kernel pair per Adam iteration);
resampling and rotation are small host-side / torch helpers.
"""
import numpy as np
import torch

from . import ops

TINY_NUMBER = 1e-8          # the fit script's epsilon of the lobe-axis normalisation


def init_light_sgs(num_lobes, seed=0):
    """the fit script's initial light: randn [M, 7] with the sharpness column x 100 (float32, CPU)"""
    lgt = torch.randn(num_lobes, 7, generator=torch.Generator().manual_seed(seed))
    lgt[:, 3:4] *= 100.
    return lgt


def _area_weights(n_in, n_out):
    """[n_out, n_in] fp64: output pixel i covers [i, i + 1) * n_in / n_out of the input axis; each input pixel counts
    with the length of its overlap, and the weights of a row sum to 1"""
    edges = torch.arange(n_out + 1, dtype=torch.float64) * (n_in / n_out)
    lo, hi = edges[:-1, None], edges[1:, None]
    j = torch.arange(n_in, dtype=torch.float64)[None, :]
    w = (torch.minimum(hi, j + 1) - torch.maximum(lo, j)).clamp_min(0.)
    return w / w.sum(dim=1, keepdim=True)


def resample_area(img, H, W):
    """Resample an [h, w] or [h, w, C] image (torch tensor or numpy array, CPU or GPU) to [H, W(, C)] by pixel coverage,
    one axis after the other: every output pixel is the average of the input pixels under its footprint, each weighted
    by the area it covers.  Downscaling is cv2.INTER_AREA (an integer factor gives exact block means).  Upscaling uses the
    same rule - each output pixel takes the input pixel(s) under it, nearest-neighbour with a coverage-weighted blend at
    the seams - where cv2.INTER_AREA would interpolate bilinearly.  The footprints tile the image, so its mean radiance
    is preserved either way.  Arithmetic in fp64, the result in the input's dtype."""
    as_numpy = isinstance(img, np.ndarray)
    t = torch.from_numpy(img) if as_numpy else img
    if t.dim() not in (2, 3):
        raise ValueError('resample_area takes [h, w] or [h, w, C], got %s' % (tuple(t.shape),))
    h, w = t.shape[0], t.shape[1]
    x = t.to(torch.float64)
    squeeze = x.dim() == 2
    if squeeze:
        x = x[..., None]
    wy = _area_weights(h, H).to(x.device)
    wx = _area_weights(w, W).to(x.device)
    out = torch.einsum('Hh,hwc->Hwc', wy, x)
    out = torch.einsum('Ww,Hwc->HWc', wx, out)
    if squeeze:
        out = out[..., 0]
    out = out.to(t.dtype)
    return out.numpy() if as_numpy else out


def rotate_light_sgs(lgt, angles, seq='yxz', degrees=True):
    """rotate_lightsg.py: lobe axes normalised (|v| + 1e-8) and rotated by R = Rotation.from_euler(seq, angles), lambda
    and mu written as |lambda| and |mu|.  A light evaluated at d after the rotation equals the original at R^T d.
    lgt [M, 7] numpy or torch (the result has the input's type, dtype and device)."""
    from scipy.spatial.transform import Rotation
    R = Rotation.from_euler(seq, angles, degrees=degrees).as_matrix()
    as_numpy = isinstance(lgt, np.ndarray)
    x = np.asarray(lgt) if as_numpy else lgt.detach().cpu().numpy()
    lobes = x[:, :3] / (np.linalg.norm(x[:, :3], axis=-1, keepdims=True) + 1e-8)
    out = np.concatenate((np.matmul(lobes, R.T), np.abs(x[:, 3:4]), np.abs(x[:, 4:])), axis=-1).astype(x.dtype)
    return out if as_numpy else torch.from_numpy(out).to(lgt.device)


class SGEnvmapFitter:
    """Adam on the light SGs of an environment map (fit_envmap_with_sg.py), state kept on the GPU.

    target, dirs: [H, W, 3] or [n, 3] (dirs: unit directions of the target's pixels, training.render.envmap_directions);
    lgt: the initial [M, 7] light (default init_light_sgs(num_lobes, seed)).  Every tensor moves to `device`."""

    def __init__(self, target, dirs, num_lobes=128, lgt=None, seed=0, lr=1e-2, betas=(0.9, 0.999), adam_eps=1e-8,
                 eps=TINY_NUMBER, device='cuda'):
        self.device = torch.device(device)
        self.target = torch.as_tensor(target).reshape(-1, 3).to(self.device, torch.float32).contiguous()
        self.dirs = torch.as_tensor(dirs).reshape(-1, 3).to(self.device, torch.float32).contiguous()
        if self.target.shape != self.dirs.shape:
            raise ValueError('target and dirs must hold the same number of pixels')
        if lgt is None:
            lgt = init_light_sgs(num_lobes, seed)
        self.lr, self.betas, self.adam_eps, self.eps = lr, tuple(betas), adam_eps, eps
        self.lgtSGs = torch.as_tensor(lgt).to(self.device, torch.float32).clone().contiguous()
        self.exp_avg = torch.zeros_like(self.lgtSGs)
        self.exp_avg_sq = torch.zeros_like(self.lgtSGs)
        self.step = 0
        self._ws = ops.envfit_workspace(self.dirs.shape[0], self.lgtSGs.shape[0], self.device)

    @property
    def num_lobes(self):
        return self.lgtSGs.shape[0]

    def fit(self, iters):
        """`iters` Adam iterations in one library call; the losses before each update as a float32 CPU tensor"""
        losses = ops.envfit_adam(self.lgtSGs, self.exp_avg, self.exp_avg_sq, self.dirs, self.target, self.step, iters,
                                 lr=self.lr, betas=self.betas, adam_eps=self.adam_eps, eps=self.eps, workspace=self._ws)
        self.step += iters
        return losses.cpu()

    def loss_grad(self, want_rgb=False):
        """(loss, grad[, rgb]) at the current light"""
        return ops.envfit_loss_grad(self.lgtSGs, self.dirs, self.target, eps=self.eps, want_rgb=want_rgb,
                                    workspace=self._ws)

    def render(self):
        """the current light evaluated on dirs, [n, 3] (the fit's own forward pass)"""
        return self.loss_grad(want_rgb=True)[2]

    def state(self):
        """the light and the Adam state, CPU tensors (load() takes it back)"""
        return {'lgtSGs': self.lgtSGs.cpu(), 'exp_avg': self.exp_avg.cpu(), 'exp_avg_sq': self.exp_avg_sq.cpu(),
                'step': self.step}

    def load(self, state):
        """resume from state() - or from a light alone ({'lgtSGs': ...}: fresh Adam moments, as the fit script does)"""
        lgt = torch.as_tensor(state['lgtSGs']).to(self.device, torch.float32)
        if lgt.shape != self.lgtSGs.shape:
            raise ValueError('light of shape %s, fitter holds %s' % (tuple(lgt.shape), tuple(self.lgtSGs.shape)))
        self.lgtSGs.copy_(lgt)
        for k in ('exp_avg', 'exp_avg_sq'):
            getattr(self, k).copy_(torch.as_tensor(state[k]).to(self.device)) if k in state else getattr(self, k).zero_()
        self.step = int(state.get('step', 0))
