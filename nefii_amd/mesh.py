"""Mesh export of a trained SDF and the materials on it (utils/plots.py:127-241, get_surface_trace /
get_surface_high_res_mesh, without skimage or trimesh).

    verts, faces = marching_cubes(volume, level)                  # skimage-like primitive on CUDA tensors
    vol = sdf_grid(model.implicit_network, 512, bound)            # the SDF on linspace(-bound, bound, 512)^3
    mesh = extract_mesh(model, resolution=512)                    # vertices, normals, per-vertex materials

The grid is evaluated by the tracer's evaluator and meshed by csrc/nefii_mcubes.hip; normals and materials come from the
fused evaluators the renderer uses.  Vertices stay in the model's normalised object space.
"""
import math
import os
from dataclasses import dataclass, field
from typing import Optional

import torch

from . import ops


def marching_cubes(volume, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """(verts [V,3] float32, faces [F,3] int64) of the level set of volume [nx, ny, nz] (a CUDA tensor), like
    skimage.measure.marching_cubes: vertex = origin + index * spacing, faces wound so that their normals point towards
    increasing values (outward for an SDF).  Welded vertices, deterministic order (include/nefii_amd.h, ABI 17).  A
    volume with no crossing gives [0, 3] tensors.  ValueError for CPU tensors, non-finite values and volumes of 2^31
    points or more."""
    if not torch.is_tensor(volume) or not volume.is_cuda:
        raise ValueError('marching_cubes needs a CUDA tensor (the hot path has no CPU fallback)')
    if volume.dim() != 3 or min(volume.shape) < 2:
        raise ValueError('volume must be [nx, ny, nz] with every dim >= 2, got %s' % (tuple(volume.shape),))
    if volume.numel() > ops.MCUBES_MAX_POINTS:
        raise ValueError('volume of %d points: marching_cubes needs fewer than 2^31' % volume.numel())
    if not math.isfinite(float(level)):
        raise ValueError('level must be finite')
    vol = volume.detach().to(torch.float32).contiguous()
    if not bool(torch.isfinite(vol).all()):
        raise ValueError('volume holds non-finite values')
    verts, faces = ops.marching_cubes(vol, level, origin, spacing)
    return verts, faces.long()


def _tracer_precision(model):
    rt = getattr(model, 'ray_tracer', None)
    return getattr(rt, 'precision', None) or os.environ.get('NEFII_TRACER_PRECISION', 'f16x3w')


def grid_axis(resolution, bound, device):
    """the grid points along one axis: linspace(-bound, bound, resolution) (plots.get_grid_uniform)"""
    return torch.linspace(-bound, bound, resolution, device=device, dtype=torch.float32)


def sdf_grid(implicit_network, resolution, bound, chunk=2 ** 24, precision=None):
    """vol [r, r, r] float32: the SDF at linspace(-bound, bound, r)^3, x slowest (vol[i, j, k] at (x_i, y_j, z_k)).  The
    tracer's evaluator for this net: ops.sdf_eval on the split-precision packing (precision 'f16x3*', the default), else
    implicit_network(x).  Evaluated in chunks of `chunk` points, under no_grad (frozen geometry, as when rendering)."""
    if resolution < 2:
        raise ValueError('resolution must be >= 2')
    if resolution ** 3 > ops.MCUBES_MAX_POINTS:
        raise ValueError('resolution %d: the grid needs fewer than 2^31 points' % resolution)
    precision = precision or os.environ.get('NEFII_TRACER_PRECISION', 'f16x3w')
    dev = next(implicit_network.parameters()).device
    ax = grid_axis(resolution, float(bound), dev)
    n = resolution ** 3
    out = torch.empty(n, device=dev, dtype=torch.float32)
    with torch.no_grad():
        split = precision.startswith('f16x3')
        pm = implicit_network.packed(f16x3=True) if split else None
        for s in range(0, n, chunk):
            idx = torch.arange(s, min(n, s + chunk), device=dev, dtype=torch.int64)
            x = torch.stack([ax[idx // (resolution * resolution)], ax[(idx // resolution) % resolution],
                             ax[idx % resolution]], 1)
            out[s:s + idx.shape[0]] = ops.sdf_eval(pm, x) if split else implicit_network(x)[:, 0]
    return out.view(resolution, resolution, resolution)


@dataclass
class Mesh:
    verts: torch.Tensor                          # [V,3] float32, normalised object space
    faces: torch.Tensor                          # [F,3] int64
    normals: Optional[torch.Tensor] = None       # [V,3] normalised SDF gradient
    diffuse_albedo: Optional[torch.Tensor] = None        # [V,3]
    roughness: Optional[torch.Tensor] = None             # [V,1]
    specular_reflection: Optional[torch.Tensor] = None   # [V,3], specular_inv_remap of the reflectance
    meta: dict = field(default_factory=dict)     # resolution, level, bound, timings (s)


def _implicit(model):
    return model.implicit_network if hasattr(model, 'implicit_network') else model


def extract_mesh(model, resolution=512, level=0.0, bound=None, materials=True, chunk=2 ** 24):
    """Mesh of the level set `level` of the SDF of `model` (an IDRNetwork or a bare ImplicitNetwork) on
    linspace(-bound, bound, resolution)^3; bound defaults to model.object_bounding_sphere.  Normals: the normalised SDF
    gradient at the vertices.  With an IDRNetwork and materials=True, also diffuse_albedo / roughness from
    envmap_material_network(verts, feats) and specular_reflection as render.py writes it (global parameters broadcast)."""
    net = _implicit(model)
    if bound is None:
        if not hasattr(model, 'object_bounding_sphere'):
            raise ValueError('a bare ImplicitNetwork needs an explicit bound')
        bound = model.object_bounding_sphere
    bound = float(bound)
    dev = next(net.parameters()).device
    timing = {}
    with torch.no_grad():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        vol = sdf_grid(net, resolution, bound, chunk=chunk, precision=_tracer_precision(model))
        ev[1].record()
        sp = 2.0 * bound / (resolution - 1)
        verts, faces = marching_cubes(vol, level, spacing=(sp, sp, sp), origin=(-bound, -bound, -bound))
        ev[2].record()
        del vol
        mesh = Mesh(verts, faces)
        if verts.shape[0]:
            _, feat, g = net.value_feature_gradient(verts)
            mesh.normals = g / g.norm(dim=1, keepdim=True).clamp_min(1e-12)
            mat_net = getattr(model, 'envmap_material_network', None)
            if materials and mat_net is not None:
                out = mat_net(verts, feat)
                V = verts.shape[0]
                mesh.diffuse_albedo = out['sg_diffuse_albedo'].float().reshape(V, 3).contiguous()
                mesh.roughness = out['sg_roughness'].float().expand(V, 1).contiguous()
                spec = mat_net.specular_inv_remap(out['sg_specular_reflectance']).float()
                mesh.specular_reflection = spec.expand(V, 3).contiguous()
        torch.cuda.synchronize(dev)
    timing['grid_s'] = ev[0].elapsed_time(ev[1]) / 1e3
    timing['mcubes_s'] = ev[1].elapsed_time(ev[2]) / 1e3
    mesh.meta = dict(resolution=int(resolution), level=float(level), bound=bound, **timing)
    return mesh
