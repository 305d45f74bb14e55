"""pt_render_indirect_mlp with the reference's signature (code/model/path_tracing_render.py:1255-1487,
diff_geo=False): 3-sample MIS direct lighting + near-field indirect light from the radiance network at
secondary hits, on HIP kernels.

Per call: nefii_mis_sample (3 directions + 3x3 pdf table per point) -> nefii_trace_rays on the 3N secondary
rays (one batched trace, the reference's speed_first path :1332-1354) -> SDF value/normal + radiance MLP at the
secondary hits (get_visibility_and_indirect_light :2109-2166; visibility = 1 - hit) -> light-SG sum along the
sampled directions -> nefii_mc_shade (GGX + Lambert, power-heuristic weights).  The reference's extra SDF
evaluation of all 3N light points (:2112) has no consumer when diff_geo=False and is not executed.

Of the reference's 12 renderer variants only this one (and its _memsave alias) is selected by a shipped conf.
pt_render_indirect_mlp_envlight is the same renderer under a lat-long map light (render-time relighting)."""
import torch

from .. import ops

TINY_NUMBER = 1e-6


def draw_uniforms(n, device):
    """The 7 uniforms per point in the reference's call order (cos r1 r2 | ggx r1 r2 | mix r0 r1 r2),
    each a separate torch.rand like the reference (:138-139, :73-74, :201, :219-220)."""
    u = [torch.rand(n, 1, device=device) for _ in range(4)]
    u.append(torch.rand(n, 1, 1, device=device).reshape(n, 1))
    u += [torch.rand(n, 1, device=device) for _ in range(2)]
    return torch.cat(u, dim=1)


def _uniforms(model, n, dev):
    """model.uniforms_override (replays a draw) or a fresh draw_uniforms"""
    uniforms = getattr(model, 'uniforms_override', None)
    if uniforms is None:
        return draw_uniforms(n, dev)
    return uniforms.to(dev)


def _secondary(wi, p3, model):
    """Trace the 3n secondary rays wi [3,n,3] from the surface points p3 [n,3] and take the indirect light from the
    radiance network at their hits -> (sec_pts [3n,3], sec_hit [3n], vis [3n], indirect [3n,3])."""
    n = p3.shape[0]
    dev = p3.device
    with torch.no_grad():
        # secondary rays: origin = surface point, one batched trace of the 3N rays
        origins = p3.detach().unsqueeze(0).expand(3, n, 3).reshape(-1, 1, 3)
        # What the trace returns for rays that MISS has no consumer: visibility and the indirect radiance use the hit mask
        # and the hit points, and the secondary-consistency step masks secondary_points with secondary_mask
        # (idr_train.py:819).  So the secondary trace skips what only fills those outputs - the min-SDF search of the
        # rays that leave without a hit and the bracket search's argmin fallback (a quarter of config 3's SDF
        # evaluations): it runs the tracer's eval-mode recurrences, whose hits are bit-identical (object_mask is all
        # ones here).  secondary_points[~secondary_mask] is then unspecified; model.secondary_miss_search = True
        # (NEFII_SECONDARY_MISS_SEARCH=1) restores the reference's values.
        rt = model.ray_tracer
        prev = rt.miss_search
        rt.miss_search = bool(getattr(model, 'secondary_miss_search', False))
        try:
            sec_pts, sec_hit, sec_dist = rt(sdf=model.implicit_network, cam_loc=origins.reshape(-1, 3),
                                            object_mask=torch.ones(3 * n, dtype=torch.bool, device=dev),
                                            ray_directions=wi.reshape(-1, 1, 3))
        finally:
            rt.miss_search = prev
        vis = 1.0 - sec_hit.to(torch.float32)                                    # [3n]
        hidx = torch.nonzero(sec_hit).flatten()
    # indirect radiance at secondary hits (gradient reaches the radiance network: not detached in the reference)
    indirect = torch.zeros(3 * n, 3, device=dev)
    if hidx.numel() > 0:
        with torch.no_grad():
            hp = sec_pts.index_select(0, hidx)
            _, feats, g = model.implicit_network.value_feature_gradient(hp)
            hn = g / (torch.norm(g, dim=-1, keepdim=True) + 1e-6)
            hv = -wi.reshape(-1, 3).index_select(0, hidx)
            hv = hv / (torch.norm(hv, dim=-1, keepdim=True) + 1e-6)
        idr = model.rendering_network(hp, hn, hv, feats)
        indirect = indirect.index_put((hidx,), idr)
    return sec_pts, sec_hit, vis, indirect


def _result(rgb, srgb, drgb, diffuse_albedo, sec_pts, sec_hit, wi, shape):
    return {'sg_rgb': rgb.reshape(shape + [3]), 'sg_specular_rgb': srgb.reshape(shape + [3]),
            'sg_diffuse_rgb': drgb.reshape(shape + [3]), 'sg_diffuse_albedo': diffuse_albedo,
            'secondary_points': sec_pts.reshape([3] + shape + [3]),
            'secondary_mask': sec_hit.reshape([3] + shape + [1]),
            'secondary_dir': wi.reshape([3] + shape + [3])}


def pt_render_indirect_mlp(lgtSGs, specular_reflectance, roughness, diffuse_albedo, normal, viewdirs, points, model,
                           blending_weights=None, diffuse_rgb=None):
    """lgtSGs [M,7]; specular_reflectance [1,3]; roughness [...,1]; diffuse_albedo/normal/viewdirs/points [...,3];
    model: the IDRNetwork.  Returns the reference's dict: sg_rgb, sg_specular_rgb, sg_diffuse_rgb,
    sg_diffuse_albedo, secondary_points [3,...,3], secondary_mask [3,...,1], secondary_dir [3,...,3]."""
    if blending_weights is not None or diffuse_rgb is not None:
        raise NotImplementedError('blending weights / precomputed diffuse (no shipped conf)')
    shape = list(normal.shape[:-1])
    n3 = normal.reshape(-1, 3)
    v3 = viewdirs.reshape(-1, 3)
    p3 = points.reshape(-1, 3)
    a3 = diffuse_albedo.reshape(-1, 3)
    r1 = roughness.reshape(-1, 1)
    n = n3.shape[0]
    with torch.no_grad():
        uniforms = _uniforms(model, n, n3.device)
        wi, own, tab = ops.mis_sample(lgtSGs, r1, n3, v3, uniforms)
    sec_pts, sec_hit, vis, indirect = _secondary(wi, p3, model)
    light = ops.EnvRadianceFn.apply(lgtSGs, wi.reshape(-1, 3), TINY_NUMBER)      # [3n,3]
    rgb, srgb, drgb = ops.McShadeFn.apply(specular_reflectance, r1, a3, n3, v3, wi, own, tab,
                                          light.reshape(3, n, 3), vis.reshape(3, n), indirect.reshape(3, n, 3))
    return _result(rgb, srgb, drgb, diffuse_albedo, sec_pts, sec_hit, wi, shape)


def pt_render_indirect_mlp_envlight(light, specular_reflectance, roughness, diffuse_albedo, normal, viewdirs, points,
                                    model):
    """pt_render_indirect_mlp under a lat-long map light (lighting.EnvmapLight; the reference's
    pt_render_shadow_indirect_mlp_envmap, path_tracing_render.py:1496 on): the third MIS technique samples the map
    (continuous inversion of its CDFs) instead of the SG mixture, and the directions that leave without a secondary hit
    see the map's texel.  Same uniforms (columns 4 and 5 pick the map's row and column), same secondary trace, indirect
    light and shading kernel; the same dict."""
    shape = list(normal.shape[:-1])
    n3 = normal.reshape(-1, 3)
    v3 = viewdirs.reshape(-1, 3)
    p3 = points.reshape(-1, 3)
    a3 = diffuse_albedo.reshape(-1, 3)
    r1 = roughness.reshape(-1, 1)
    n = n3.shape[0]
    with torch.no_grad():
        uniforms = _uniforms(model, n, n3.device)
        wi, own, tab, radiance = light.sample(r1, n3, v3, uniforms)
    sec_pts, sec_hit, vis, indirect = _secondary(wi, p3, model)
    rgb, srgb, drgb = ops.McShadeFn.apply(specular_reflectance, r1, a3, n3, v3, wi, own, tab, radiance,
                                          vis.reshape(3, n), indirect.reshape(3, n, 3))
    return _result(rgb, srgb, drgb, diffuse_albedo, sec_pts, sec_hit, wi, shape)


def pt_render_indirect_mlp_memsave(*args, **kwargs):
    """Same result; the reference's memsave variant only traces the three sample sets one at a time."""
    return pt_render_indirect_mlp(*args, **kwargs)
