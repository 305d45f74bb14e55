"""Lights from HDR environment maps: spherical-Gaussian fits (envmaps/fit_envmap_with_sg.py, envmaps/rotate_lightsg.py)
and the map itself as an importance-sampled light of the Monte-Carlo renderer (EnvmapLight).

    fitter = SGEnvmapFitter(target, dirs, num_lobes=128)     # target / dirs [H, W, 3] or [n, 3], on the GPU
    losses = fitter.fit(1000)                                # the loss before each update, on the host
    np.save('sg_128.npy', fitter.lgtSGs.cpu().numpy())       # a light for EnvmapMaterialNetwork.load_light

    light = EnvmapLight.from_exr('sky.exr', 'mitsuba')       # the map, sampling table built once on the GPU
    model.set_envmap_light(light)                            # relight a pt_render_indirect_mlp model under it

The fit itself runs in libnefii_hip.so (ops.envfit_adam: one fused, deterministic kernel pair per Adam iteration), and so
do the map light's table build, sampler and lookups (ops.envlight_*), under a rotation too (EnvmapLight.rotated, DESIGN.md
6i); resampling and the rotation of SG lobes are small host-side / torch helpers.
"""
import math

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


def load_envmap(path, H=None, W=None):
    """an HDR map's first three channels (a single-channel map repeated) as float32 numpy [H, W, 3], resampled by
    resample_area when a size is given (either one missing: the file's own size on that axis)"""
    from .utils import exr
    img = exr.imread(path)
    if img.ndim == 2:
        img = np.repeat(img[..., None], 3, axis=-1)
    if img.shape[-1] < 3:
        raise ValueError('%s has %d channels, need 3' % (path, img.shape[-1]))
    img = np.ascontiguousarray(img[..., :3], dtype=np.float32)
    H = img.shape[0] if H is None else int(H)
    W = img.shape[1] if W is None else int(W)
    if img.shape[:2] != (H, W):
        img = resample_area(img, H, W)
    return img


def turntable_rotations(angles_deg, coordinate_type='mitsuba'):
    """the light turntable of scripts/vis_rotate_envlight.py: a yaw about the up axis per angle (degrees) -> float32
    [A, 3, 3] (CPU), R world-from-light as rotate_light_sgs builds it.  'mitsuba' yaws about y
    (from_euler('yxz', [a, 0, 0])), 'blender' about z (from_euler('xyz', [0, 0, a]))."""
    from scipy.spatial.transform import Rotation
    ops._envlight_coord(coordinate_type)
    angles = np.atleast_1d(np.asarray(angles_deg, dtype=np.float64))
    if angles.ndim != 1 or angles.size < 1:
        raise ValueError('angles_deg must hold at least one angle, got shape %s' % (angles.shape,))
    if coordinate_type == 'mitsuba':
        R = [Rotation.from_euler('yxz', [a, 0., 0.], degrees=True).as_matrix() for a in angles]
    else:
        R = [Rotation.from_euler('xyz', [0., 0., a], degrees=True).as_matrix() for a in angles]
    return torch.from_numpy(np.stack(R).astype(np.float32))


def rotate_light_sgs_matrix(lgt, R):
    """rotate_light_sgs' arithmetic for a given matrix, in torch on lgt's device: lobe axes normalised (|v| + 1e-8) and
    mapped to R v, lambda and mu as |lambda| and |mu|.  lgt [M, 7], R [3, 3] -> [M, 7] of lgt's dtype."""
    R = torch.as_tensor(R).to(lgt.device, torch.float64)
    x = lgt.detach().to(torch.float64)
    lobes = x[:, :3] / (x[:, :3].norm(dim=-1, keepdim=True) + 1e-8)
    return torch.cat((lobes @ R.T, x[:, 3:4].abs(), x[:, 4:].abs()), dim=-1).to(lgt.dtype)


def is_identity_rotation(R):
    """True where the nine floats of R [3, 3] are exactly the identity's: such a rotation is skipped, not multiplied"""
    return torch.equal(torch.as_tensor(R).detach().to('cpu', torch.float32), torch.eye(3))


def turned_light_sgs(lgt, R):
    """the SG light lgt [M, 7] under the rotation R of a turntable: rotate_light_sgs_matrix - or, for a rotation that is
    exactly the identity, the light as it is (detached): angle 0 of a turntable is the unrotated render, bit for bit"""
    return lgt.detach() if is_identity_rotation(R) else rotate_light_sgs_matrix(lgt, R)


def _rotations_f32(R):
    """R as a float32 CPU tensor [A, 3, 3] ([3, 3] -> [1, 3, 3])"""
    R = torch.as_tensor(R).detach().to('cpu', torch.float32)
    if R.dim() == 2:
        R = R[None]
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3) or R.shape[0] < 1:
        raise ValueError('rotations must be [3, 3] or [A, 3, 3], got %s' % (tuple(R.shape),))
    return R.contiguous()


def texel_directions(H, W, coordinate_type='mitsuba'):
    """unit directions [H, W, 3] (float32, CPU) of the texel centres of an H x W map light: v = (i + 0.5) / H,
    u = (j + 0.5) / W (training.render.envmap_directions puts row i at pi i / (H - 1) instead)"""
    v = (torch.arange(H, dtype=torch.float64) + 0.5) / H
    u = (torch.arange(W, dtype=torch.float64) + 0.5) / W
    phi, uu = torch.meshgrid(math.pi * v, u, indexing='ij')
    if coordinate_type == 'mitsuba':
        theta = 2. * math.pi * uu - 0.5 * math.pi
        d = torch.stack([torch.cos(theta) * torch.sin(phi), torch.cos(phi), torch.sin(theta) * torch.sin(phi)], dim=-1)
    elif coordinate_type == 'blender':
        theta = math.pi - 2. * math.pi * uu
        d = torch.stack([torch.cos(theta) * torch.sin(phi), torch.sin(theta) * torch.sin(phi), torch.cos(phi)], dim=-1)
    else:
        raise ValueError('coordinate_type is mitsuba or blender, not ' + str(coordinate_type))
    return d.to(torch.float32)


class EnvmapLight:
    """A lat-long HDR map [H, W, 3] as a light: nearest-texel radiance, importance sampling by the
    piecewise-constant distribution of its luminance x sin(phi).  The map lives on the GPU as contiguous float32, the
    sampling table is built once here.  coordinate_type: 'mitsuba' (y up) or 'blender' (z up)."""

    def __init__(self, envmap, coordinate_type='mitsuba', device='cuda'):
        ops._envlight_coord(coordinate_type)
        self.envmap = torch.as_tensor(envmap).to(device=torch.device(device), dtype=torch.float32).contiguous()
        self.coordinate_type = coordinate_type
        self.table = ops.envlight_table(self.envmap)
        self.rotation = None          # rotated(): R [3, 3] float32 on the CPU, world-from-light; None is the identity
        self._rot = None              # the same as [1, 3, 3] on the GPU

    @classmethod
    def from_exr(cls, path, coordinate_type='mitsuba', height=None, width=None, scale=1.0, device='cuda'):
        """the map in an EXR file (first three channels), resampled to height x width by pixel coverage when given,
        times the exposure `scale`"""
        img = load_envmap(path, height, width)
        if scale != 1.0:
            img = img * np.float32(scale)
        return cls(torch.from_numpy(np.ascontiguousarray(img)), coordinate_type, device)

    @classmethod
    def from_sg(cls, lgtSGs, H, W, coordinate_type='mitsuba'):
        """the SG light lgtSGs [M, 7] evaluated at the texel centres (nefii_env_radiance_forward, eps 1e-6 - as the
        Monte-Carlo renderer evaluates it along its sampled directions)"""
        dirs = texel_directions(H, W, coordinate_type).reshape(-1, 3).to(lgtSGs.device)
        with torch.no_grad():
            rgb = ops.EnvRadianceFn.apply(lgtSGs.detach(), dirs, 1e-6)
        return cls(rgb.reshape(H, W, 3), coordinate_type, lgtSGs.device)

    @property
    def shape(self):
        return self.envmap.shape[0], self.envmap.shape[1]

    def rotated(self, R):
        """this light rotated by R [3, 3] (world-from-light, rotate_light_sgs' convention: the new light along d is this
        one along R^T d) -> an EnvmapLight that shares the map and the table (nothing is rebuilt) and carries R (DESIGN.md
        6i).  A rotation that is exactly the identity gives a light on the unrotated code path."""
        R = self._composed(R)
        if R.shape[0] != 1:
            raise ValueError('rotated takes one [3, 3] rotation, got %d' % R.shape[0])
        out = object.__new__(type(self))
        out.envmap, out.coordinate_type, out.table = self.envmap, self.coordinate_type, self.table
        if is_identity_rotation(R[0]):
            out.rotation, out._rot = None, None
        else:
            out.rotation, out._rot = R[0], R.to(self.envmap.device)
        return out

    def _composed(self, R):
        """R [A, 3, 3] (or [3, 3]) on top of this light's own rotation, float32 on the CPU; without one, R's own floats"""
        R = _rotations_f32(R)
        if self.rotation is None:
            return R
        return (R.to(torch.float64) @ self.rotation.to(torch.float64)).to(torch.float32).contiguous()

    def rotations(self, R):
        """_composed(R) on the GPU, as the ops.envlight_*_rot wrappers take it"""
        return self._composed(R).to(self.envmap.device)

    def radiance(self, dirs):
        """radiance along dirs [..., 3] -> [..., 3]"""
        shape = dirs.shape[:-1]
        return ops._envlight_radiance(self.envmap, self.coordinate_type, dirs.reshape(-1, 3), self._rot).reshape(*shape, 3)

    def pdf(self, dirs):
        """the sampler's solid-angle density along dirs [..., 3] -> [...]"""
        H, W = self.shape
        shape = dirs.shape[:-1]
        return ops._envlight_pdf(self.table, H, W, self.coordinate_type, dirs.reshape(-1, 3), self._rot).reshape(shape)

    def sample(self, rough, normal, view, uniforms):
        """the three MIS directions of every point (cosine, GGX, map) -> wi [3,n,3], own_pdf [3,n], pdf_table [3,n,3],
        light [3,n,3]; uniforms [n, 7] as path_tracing_render.draw_uniforms draws them (columns 4, 5: the map)"""
        return tuple(t[0] for t in ops._envlight_mis(self.envmap, self.table, self.coordinate_type, rough, normal, view,
                                                     uniforms, self._rot))

    def sample_rotations(self, R, rough, normal, view, uniforms):
        """sample() under each of the rotations R [A, 3, 3] of this light, one launch -> wi [A,3,n,3], own_pdf [A,3,n],
        pdf_table [A,3,n,3], light [A,3,n,3]; slice a is rotated(R[a]).sample(...), rows 0-1 (cosine, GGX) are the same
        in every slice"""
        return ops.envlight_mis_sample_rot(self.envmap, self.table, self.coordinate_type, self.rotations(R), rough,
                                           normal, view, uniforms)

    def bounce_sample(self, specular, rough, albedo, normal, view, uniforms):
        """one recomputed bounce at m secondary hits -> wo [m,3], weight [m,3]: one direction per hit by
        one-sample MIS over cosine / GGX / map, and the radiance the hit sends along `view` if that direction is
        unoccluded; uniforms [m, 3] as path_tracing_render.draw_bounce_uniforms draws them"""
        return ops._envlight_bounce(self.envmap, self.table, self.coordinate_type, specular, rough, albedo, normal, view,
                                    uniforms, rot=self._rot)

    def bounce_sample_rotations(self, R, rot_index, specular, rough, albedo, normal, view, uniforms):
        """bounce_sample() with hit p under rotation R[rot_index[p]] of this light (rot_index int32 [m] on the GPU):
        the hits of every angle of a turntable chunk in one launch"""
        return ops.envlight_bounce_sample_rot(self.envmap, self.table, self.coordinate_type, self.rotations(R), rot_index,
                                              specular, rough, albedo, normal, view, uniforms)

    def radiance_rotations(self, R, dirs, rot_index=None):
        """radiance along dirs [n, 3] with direction p under rotation R[rot_index[p]] of this light (None: R[0])"""
        return ops.envlight_radiance_rot(self.envmap, self.coordinate_type, self.rotations(R), dirs, rot_index)
