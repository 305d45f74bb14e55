"""pt_render_indirect_mlp with the reference's signature (code/model/path_tracing_render.py:1255-1487,
diff_geo=False): 3-sample MIS direct lighting + near-field indirect light from the radiance network at
secondary hits, on HIP kernels.

Per call: nefii_mis_sample (3 directions + 3x3 pdf table per point) -> nefii_trace_rays on the 3N secondary
rays (one batched trace, the reference's speed_first path :1332-1354) -> SDF value/normal + radiance MLP at the
secondary hits (get_visibility_and_indirect_light :2109-2166; visibility = 1 - hit) -> light-SG sum along the
sampled directions -> nefii_mc_shade (GGX + Lambert, power-heuristic weights).  The reference's extra SDF
evaluation of all 3N light points (:2112) has no consumer when diff_geo=False and is not executed.

Of the reference's 12 renderer variants only this one (and its _memsave alias) is selected by a shipped conf.
pt_render_indirect_mlp_envlight is the same renderer under a lat-long map light (render-time relighting);
its indirect='bounce' replaces the radiance network at the secondary hits by one recomputed bounce under that map (6h).
pt_render_turntable renders a chunk under A rotations of the light at once and shares what does not depend on it (6i)."""
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


def draw_bounce_uniforms(n, device):
    """The 3 uniforms (technique | direction r1 r2) of each of the 3n secondary rays of the recomputed bounce (DESIGN.md
    6h) -> [3n, 3]; row k*n + p belongs to secondary ray k of point p, the layout of wi.  Drawn after draw_uniforms, and
    only in bounce mode: every other mode consumes the RNG stream as before."""
    return torch.rand(3 * n, 3, device=device)


def _bounce_uniforms(model, n, dev):
    """model.bounce_uniforms_override (replays a draw) or a fresh draw_bounce_uniforms"""
    uniforms = getattr(model, 'bounce_uniforms_override', None)
    if uniforms is None:
        return draw_bounce_uniforms(n, dev)
    return uniforms.to(dev)


def trace_occluders(origins, dirs, model):
    """One batched trace of the rays origins + t dirs ([k,3] each) against the model's own surface, as the secondary
    rays are traced -> (points [k,3], hit [k] bool).  Also what texture.bake_occlusion traces its hemisphere rays with."""
    k = origins.shape[0]
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
        pts, hit, _ = rt(sdf=model.implicit_network, cam_loc=origins.reshape(-1, 3),
                         object_mask=torch.ones(k, dtype=torch.bool, device=origins.device),
                         ray_directions=dirs.reshape(-1, 1, 3))
    finally:
        rt.miss_search = prev
    return pts, hit


def _trace_occluders(origins, dirs, model):
    """the renderer's own name for trace_occluders"""
    return trace_occluders(origins, dirs, model)


def _secondary_trace(wi, p3, model):
    """Trace the 3n secondary rays wi [3,n,3] from the surface points p3 [n,3]
    -> (sec_pts [3n,3], sec_hit [3n], vis [3n], hidx: the indices of the hits, in the order of nonzero(sec_hit))."""
    n = p3.shape[0]
    with torch.no_grad():
        # secondary rays: origin = surface point, one batched trace of the 3N rays
        origins = p3.detach().unsqueeze(0).expand(3, n, 3).reshape(-1, 1, 3)
        sec_pts, sec_hit = _trace_occluders(origins, wi, model)
        vis = 1.0 - sec_hit.to(torch.float32)                                    # [3n]
        hidx = torch.nonzero(sec_hit).flatten()
    return sec_pts, sec_hit, vis, hidx


def _hit_frame(wi, sec_pts, hidx, model):
    """points, features, unit normals and unit views (-wi) of the secondary hits hidx (call under no_grad)"""
    hp = sec_pts.index_select(0, hidx)
    _, feats, g = model.implicit_network.value_feature_gradient(hp)
    hn = g / (torch.norm(g, dim=-1, keepdim=True) + 1e-6)
    hv = -wi.reshape(-1, 3).index_select(0, hidx)
    hv = hv / (torch.norm(hv, dim=-1, keepdim=True) + 1e-6)
    return hp, feats, hn, hv


def _indirect_mlp(wi, sec_pts, hidx, model):
    """The trained radiance network at the secondary hits -> indirect [3n,3] (zero where nothing was hit)."""
    # indirect radiance at secondary hits (gradient reaches the radiance network: not detached in the reference)
    indirect = torch.zeros(wi.shape[0] * wi.shape[1], 3, device=wi.device)
    if hidx.numel() > 0:
        with torch.no_grad():
            hp, feats, hn, hv = _hit_frame(wi, sec_pts, hidx, model)
        idr = model.rendering_network(hp, hn, hv, feats)
        indirect = indirect.index_put((hidx,), idr)
    return indirect


def _indirect_bounce(light, wi, sec_pts, hidx, bounce_uniforms, model):
    """One recomputed bounce under the map light -> indirect [3n,3]: at every secondary hit the model's own
    material is shaded under the map along ONE importance-sampled direction (light.bounce_sample), and a tertiary shadow
    ray gives its visibility.  Tertiary rays that hit geometry contribute nothing, so the result is linear in the map."""
    indirect = torch.zeros(wi.shape[0] * wi.shape[1], 3, device=wi.device)
    if hidx.numel() > 0:
        with torch.no_grad():
            hp, feats, hn, hv = _hit_frame(wi, sec_pts, hidx, model)
            mat = model.envmap_material_network(hp, feats, hn)
            m = hp.shape[0]
            wo, weight = light.bounce_sample(mat['sg_specular_reflectance'].expand(1, 3),
                                             mat['sg_roughness'].reshape(-1, 1).expand(m, 1), mat['sg_diffuse_albedo'],
                                             hn, hv, bounce_uniforms.index_select(0, hidx))
            _, ter_hit = _trace_occluders(hp.reshape(-1, 1, 3), wo, model)
            indirect = indirect.index_put((hidx,), weight * (1.0 - ter_hit.to(torch.float32)).unsqueeze(-1))
    return indirect


def _secondary(wi, p3, model):
    """Trace the 3n secondary rays wi [3,n,3] from the surface points p3 [n,3] and take the indirect light from the
    radiance network at their hits -> (sec_pts [3n,3], sec_hit [3n], vis [3n], indirect [3n,3])."""
    sec_pts, sec_hit, vis, hidx = _secondary_trace(wi, p3, model)
    return sec_pts, sec_hit, vis, _indirect_mlp(wi, sec_pts, hidx, model)


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


INDIRECT_MODES = ('mlp', 'bounce')


def pt_render_indirect_mlp_envlight(light, specular_reflectance, roughness, diffuse_albedo, normal, viewdirs, points,
                                    model, indirect='mlp'):
    """pt_render_indirect_mlp under a lat-long map light (lighting.EnvmapLight; the reference's
    pt_render_shadow_indirect_mlp_envmap, path_tracing_render.py:1496 on): the third MIS technique samples the map
    (continuous inversion of its CDFs) instead of the SG mixture, and the directions that leave without a secondary hit
    see the map's texel.  Same uniforms (columns 4 and 5 pick the map's row and column), same secondary trace, indirect
    light and shading kernel; the same dict.

    indirect: 'mlp' reads the trained radiance network at the secondary hits - the TRAINING light's interreflections;
    'bounce' recomputes one bounce under the map there (_indirect_bounce; no gradient)."""
    if indirect not in INDIRECT_MODES:
        raise ValueError('indirect is one of %s, not %r' % (', '.join(INDIRECT_MODES), indirect))
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
    if indirect == 'bounce':
        with torch.no_grad():
            bounce_uniforms = _bounce_uniforms(model, n, n3.device)
        sec_pts, sec_hit, vis, hidx = _secondary_trace(wi, p3, model)
        ind = _indirect_bounce(light, wi, sec_pts, hidx, bounce_uniforms, model)
    else:
        sec_pts, sec_hit, vis, ind = _secondary(wi, p3, model)
    rgb, srgb, drgb = ops.McShadeFn.apply(specular_reflectance, r1, a3, n3, v3, wi, own, tab, radiance,
                                          vis.reshape(3, n), ind.reshape(3, n, 3))
    return _result(rgb, srgb, drgb, diffuse_albedo, sec_pts, sec_hit, wi, shape)


def pt_render_turntable(rotations, lgtSGs, specular_reflectance, roughness, diffuse_albedo, normal, viewdirs, points,
                        model):
    """One chunk under each of the A rotations [A, 3, 3] (world-from-light, lighting.turntable_rotations) of the light
    the model renders under - model.envmap_light in its indirect mode, else lgtSGs - as a list of A dicts, each what
    pt_render_indirect_mlp(_envlight) returns under that rotated light for the same uniforms (no gradient).

    One draw of the uniforms serves every angle.  Rows 0 and 1 of the sampler (cosine, GGX) never see the light, so their
    secondary rays are traced once and row 2 of every angle joins them in ONE trace of (2 + A) n rays; the indirect light
    of all those hits comes from one pass.  Per angle only the shading kernel runs."""
    from ..lighting import turned_light_sgs
    light = model.envmap_light
    mode = model.envmap_indirect if light is not None else 'mlp'
    A = rotations.shape[0]
    shape = list(normal.shape[:-1])
    n3 = normal.reshape(-1, 3)
    v3 = viewdirs.reshape(-1, 3)
    p3 = points.reshape(-1, 3)
    a3 = diffuse_albedo.reshape(-1, 3)
    r1 = roughness.reshape(-1, 1)
    n = n3.shape[0]
    dev = n3.device
    with torch.no_grad():
        uniforms = _uniforms(model, n, dev)
        if light is not None:
            wi, own, tab, radiance = light.sample_rotations(rotations, r1, n3, v3, uniforms)
        else:
            # an SG light: its lobes rotated per angle (angle 0: as they are), one (cheap) sampler call each; rows 0-1 are
            # the first call's
            lgts = [turned_light_sgs(lgtSGs, R) for R in rotations]
            per = [ops.mis_sample(lgt, r1, n3, v3, uniforms) for lgt in lgts]
            wi = torch.stack([torch.cat((per[0][0][:2], s[0][2:]), dim=0) for s in per])
            own = torch.stack([torch.cat((per[0][1][:2], s[1][2:]), dim=0) for s in per])
            tab = torch.stack([s[2] for s in per])
        if mode == 'bounce':
            bounce_uniforms = _bounce_uniforms(model, n, dev)
        # the secondary trace: rows 0-1 once, row 2 of every angle
        dirs = torch.cat((wi[0, :2], wi[:, 2]), dim=0)                                  # [2 + A, n, 3]
        origins = p3.unsqueeze(0).expand(2 + A, n, 3).reshape(-1, 1, 3)
        pts, hit = _trace_occluders(origins, dirs, model)
        hidx = torch.nonzero(hit).flatten()
        if mode == 'bounce':
            ind = _turntable_bounce(light, rotations, dirs, pts, hidx, bounce_uniforms, n, model)   # [A, 3n, 3]
        else:
            shared = _indirect_mlp(dirs, pts, hidx, model)                              # [(2 + A) n, 3]
        out = []
        for a in range(A):
            lo = (2 + a) * n
            sec_pts = torch.cat((pts[:2 * n], pts[lo:lo + n]), dim=0)
            sec_hit = torch.cat((hit[:2 * n], hit[lo:lo + n]), dim=0)
            vis = 1.0 - sec_hit.to(torch.float32)
            ind_a = ind[a] if mode == 'bounce' else torch.cat((shared[:2 * n], shared[lo:lo + n]), dim=0)
            if light is not None:
                rad = radiance[a]
            else:
                rad = ops.EnvRadianceFn.apply(lgts[a], wi[a].reshape(-1, 3), TINY_NUMBER).reshape(3, n, 3)
            rgb, srgb, drgb = ops.McShadeFn.apply(specular_reflectance, r1, a3, n3, v3, wi[a], own[a], tab[a], rad,
                                                  vis.reshape(3, n), ind_a.reshape(3, n, 3))
            out.append(_result(rgb, srgb, drgb, diffuse_albedo, sec_pts, sec_hit, wi[a], shape))
    return out


def _turntable_bounce(light, rotations, dirs, pts, hidx, bounce_uniforms, n, model):
    """_indirect_bounce for the turntable's (2 + A) n secondary rays -> indirect [A, 3n, 3].  A hit of rows 0-1 is shared
    by the angles but lit differently under each, so it enters the bounce sampler once per angle; a row-2 hit belongs to
    its own angle.  The hit frames and materials are evaluated once per hit, the bounce of all of them is one
    bounce_sample call (rot_index) and one tertiary trace."""
    A = rotations.shape[0]
    dev = dirs.device
    ind = torch.zeros(A * 3 * n, 3, device=dev)
    h01, h2 = hidx[hidx < 2 * n], hidx[hidx >= 2 * n]
    parts = []                # per group: (hit frame and material, repeats, rotation of each item, its row of [A, 3n])
    if h01.numel() > 0:
        ang = torch.arange(A, device=dev).repeat_interleave(h01.numel())
        parts.append((h01, A, ang, h01.repeat(A), h01.repeat(A)))
    if h2.numel() > 0:
        ang = (h2 - 2 * n) // n
        ray = 2 * n + (h2 - 2 * n) % n
        parts.append((h2, 1, ang, ray, ray))
    if not parts:
        return ind.reshape(A, 3 * n, 3)
    cols = {k: [] for k in ('hp', 'hn', 'hv', 'rough', 'albedo', 'rot', 'uni', 'dst')}
    spec = None
    for h, rep, ang, ray, uni_row in parts:
        hp, feats, hn, hv = _hit_frame(dirs, pts, h, model)
        mat = model.envmap_material_network(hp, feats, hn)
        spec = mat['sg_specular_reflectance'].expand(1, 3)
        rough = mat['sg_roughness'].reshape(-1, 1).expand(hp.shape[0], 1)
        for k, v in (('hp', hp), ('hn', hn), ('hv', hv), ('rough', rough), ('albedo', mat['sg_diffuse_albedo'])):
            cols[k].append(v.repeat(rep, 1))
        cols['rot'].append(ang)
        cols['uni'].append(bounce_uniforms.index_select(0, uni_row))
        cols['dst'].append(ang * (3 * n) + ray)
    c = {k: torch.cat(v, dim=0) for k, v in cols.items()}
    wo, weight = light.bounce_sample_rotations(rotations, c['rot'].to(torch.int32), spec, c['rough'], c['albedo'],
                                               c['hn'], c['hv'], c['uni'])
    _, ter_hit = _trace_occluders(c['hp'].reshape(-1, 1, 3), wo, model)
    ind = ind.index_put((c['dst'],), weight * (1.0 - ter_hit.to(torch.float32)).unsqueeze(-1))
    return ind.reshape(A, 3 * n, 3)


def pt_render_indirect_mlp_memsave(*args, **kwargs):
    """Same result; the reference's memsave variant only traces the three sample sets one at a time."""
    return pt_render_indirect_mlp(*args, **kwargs)
