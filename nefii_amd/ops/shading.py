"""Row assembly, the material head, SG shading and Monte-Carlo shading."""
import torch

from .. import _lib
from ._call import _f32, _ptr, call, check_tensor


class AssembleRowsFn(torch.autograd.Function):
    """Per-ray output buffers in two launches (include/nefii_amd.h: nefii_assemble_rows): output k is a [rows, cols[k]]
    buffer of fills[k] whose rows where[i] take row i of srcs[k] ([n, cols[k]], or [1, cols[k]] / [n, 1] broadcast).
    Backward: one launch gathers the rows of every output gradient that exists."""

    @staticmethod
    def forward(ctx, where, rows, fills, cols, *srcs):
        check_tensor('where', where, torch.int64, (None,))      # the kernels read n 8-byte entries
        n = where.shape[0]
        dev = where.device
        if not 1 <= len(srcs) <= _lib.MAX_ROW_BLOCKS or len(fills) != len(srcs) or len(cols) != len(srcs) or rows < 1:
            raise ValueError('assemble_rows takes 1 to %d sources with one fill and one column count each, and rows >= 1'
                             % _lib.MAX_ROW_BLOCKS)
        for k, src in enumerate(srcs):      # every source before the first launch: n rows or one, cols[k] columns or one
            if not torch.is_tensor(src) or src.dim() != 2 or src.device != dev or cols[k] < 1 or \
                    src.shape[0] not in (n, 1) or src.shape[1] not in (cols[k], 1):
                raise ValueError('assemble_rows: source %d must be [%d or 1, %d or 1] on %s, got %s'
                                 % (k, n, cols[k], dev, tuple(src.shape) if torch.is_tensor(src) else type(src).__name__))
        blocks = (_lib.RowBlock * len(srcs))()
        outs, keep, shapes = [], [], []
        for k, src in enumerate(srcs):
            shapes.append(tuple(src.shape))
            s = _f32(src)
            if s.shape[-1] != cols[k]:          # a column broadcast ([n, 1] -> [n, C]) is materialised; a row broadcast is a stride
                s = s.expand(s.shape[0], cols[k]).contiguous()
            keep.append(s)
            out = torch.empty(rows, cols[k], device=dev, dtype=torch.float32)
            outs.append(out)
            blocks[k] = _lib.RowBlock(_ptr(s), _ptr(out), cols[k], 0 if s.shape[0] == 1 and n != 1 else cols[k], float(fills[k]), 0)
        call('nefii_assemble_rows', blocks, len(srcs), _ptr(where), n, rows)
        ctx.save_for_backward(where)
        ctx.meta = (rows, tuple(cols), shapes)
        ctx.set_materialize_grads(False)        # a buffer the loss does not read sends None back, not zeros
        # a buffer assembled from constants (normals, points of frozen geometry) is a constant: without this every output of
        # the node would require grad because some other does
        ctx.mark_non_differentiable(*[o for k, o in enumerate(outs) if not ctx.needs_input_grad[4 + k]])
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        where, = ctx.saved_tensors
        rows, cols, shapes = ctx.meta
        n = where.shape[0]
        blocks = (_lib.RowBlock * len(grads))()
        res, keep = [], []
        for k, g in enumerate(grads):
            if g is None or not ctx.needs_input_grad[4 + k]:
                blocks[k] = _lib.RowBlock(None, None, cols[k], cols[k], 0.0, 0)
                res.append(None)
                continue
            gc = _f32(g)
            keep.append(gc)
            d = torch.empty(n, cols[k], device=where.device, dtype=torch.float32)
            blocks[k] = _lib.RowBlock(_ptr(gc), _ptr(d), cols[k], cols[k], 0.0, 0)
            res.append(d)
        if any(r is not None for r in res) and n > 0:
            call('nefii_gather_rows', blocks, len(grads), _ptr(where), n, rows)
        for k, r in enumerate(res):             # undo the broadcasts of forward
            if r is not None and tuple(r.shape) != shapes[k]:
                r = r.sum(dim=0, keepdim=True) if shapes[k][0] == 1 and n != 1 else r
                r = r.sum(dim=1, keepdim=True) if shapes[k][-1] == 1 and cols[k] != 1 else r
                res[k] = r.reshape(shapes[k])
        return (None, None, None, None) + tuple(res)


class MaterialHeadGlobalFn(torch.autograd.Function):
    """(roughness [1,1], specular [1,3]) from the GLOBAL roughness / specular parameters of physg.conf's material network
    (nefii_material_head_global): sigmoid, TINNY_ROUGHNESS blend, white-specular expand, warm-up flags and the 0.16 s^2 remap
    in one launch each way."""

    @staticmethod
    def forward(ctx, rough_param, spec_param, fake_rough, fake_spec):
        r_, s_ = _f32(rough_param), _f32(spec_param)
        rough = torch.empty(1, 1, device=r_.device, dtype=torch.float32)
        spec = torch.empty(1, 3, device=r_.device, dtype=torch.float32)
        call('nefii_material_head_global', _ptr(r_), _ptr(s_), s_.numel(), int(bool(fake_rough)), int(bool(fake_spec)),
             _ptr(rough), _ptr(spec))
        ctx.save_for_backward(r_, s_)
        ctx.flags = (int(bool(fake_rough)), int(bool(fake_spec)))
        ctx.shapes = (rough_param.shape, spec_param.shape)
        ctx.set_materialize_grads(False)
        return rough, spec

    @staticmethod
    def backward(ctx, d_rough, d_spec):
        r_, s_ = ctx.saved_tensors
        if d_rough is None and d_spec is None:
            return None, None, None, None
        dr = _f32(d_rough) if d_rough is not None else None
        ds = _f32(d_spec) if d_spec is not None else None
        gr, gs = torch.empty_like(r_), torch.empty_like(s_)
        call('nefii_material_head_global_backward', _ptr(r_), _ptr(s_), s_.numel(), ctx.flags[0], ctx.flags[1], _ptr(dr),
             _ptr(ds), _ptr(gr), _ptr(gs))
        return gr.reshape(ctx.shapes[0]), gs.reshape(ctx.shapes[1]), None, None


def prepare_hits(points, ray_dirs, grad, feat, idx):
    """(points[idx], view = -ray_dirs[idx] / (norm + 1e-6), normals = grad[idx] / (norm + 1e-6), feat[idx] or None) in one
    launch (nefii_prepare_hits); constants of the autograd graph (frozen geometry)."""
    check_tensor('idx', idx, torch.int64, (None,))              # the kernel reads n 8-byte entries
    n = idx.shape[0]
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[0] < 1:
        raise ValueError('prepare_hits: points must be a tensor [rows, 3] with rows >= 1, got %s'
                         % (tuple(points.shape) if torch.is_tensor(points) else type(points).__name__,))
    rows, dev, bad = points.shape[0], points.device, None
    for name, t, c in (('points', points, 3), ('ray_dirs', ray_dirs, 3), ('grad', grad, 3)) + \
            ((('feat', feat, None),) if feat is not None else ()):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] != rows or (c is not None and t.shape[1] != c) or t.device != dev:
            bad = bad or name
    if bad:
        t = {'points': points, 'ray_dirs': ray_dirs, 'grad': grad, 'feat': feat}[bad]
        raise ValueError('prepare_hits: points, ray_dirs and grad are [rows, 3] and feat [rows, F] with the same rows >= 1 '
                         'on one device; %s is %s' % (bad, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    if idx.device != dev:
        raise ValueError('prepare_hits: idx is on %s, the rows on %s' % (idx.device, dev))
    pts = torch.empty(n, 3, device=dev, dtype=torch.float32)
    view = torch.empty(n, 3, device=dev, dtype=torch.float32)
    nrm = torch.empty(n, 3, device=dev, dtype=torch.float32)
    fcols = 0 if feat is None else feat.shape[1]
    fout = None if feat is None else torch.empty(n, fcols, device=dev, dtype=torch.float32)
    if n > 0:
        p_, d_, g_ = _f32(points), _f32(ray_dirs), _f32(grad)
        f_ = None if feat is None else _f32(feat)
        call('nefii_prepare_hits', _ptr(p_), _ptr(d_), _ptr(g_), _ptr(f_), fcols, _ptr(idx), n, p_.shape[0], _ptr(pts),
             _ptr(view), _ptr(nrm), _ptr(fout))
    return pts, view, nrm, fout


def assemble_rows(where, rows, fills, cols, srcs):
    return AssembleRowsFn.apply(where, int(rows), tuple(fills), tuple(cols), *srcs)


# most light lobes any shading or envfit kernel takes (NEFII_MAX_LOBES in include/nefii_amd.h)
MAX_LOBES = 512


def check_light(lgt):
    """lgtSGs must be [M, 7] with 1 <= M <= MAX_LOBES: refused here with a ValueError rather than as a C error code"""
    if lgt.dim() != 2 or lgt.shape[1] != 7 or not 1 <= lgt.shape[0] <= MAX_LOBES:
        raise ValueError('lgtSGs must be [M, 7] with 1 <= M <= %d, got %s' % (MAX_LOBES, tuple(lgt.shape)))


class SGRenderFn(torch.autograd.Function):
    """render_with_sg for one base material; differentiable wrt lgtSGs, specular, roughness, albedo."""

    @staticmethod
    def forward(ctx, lgt, spec, rough, albedo, normal, view):
        check_light(lgt)
        n = normal.shape[0]
        lgt_c, spec_c, rough_c = _f32(lgt), _f32(spec.expand(1, 3)), _f32(rough)
        albedo_c, normal_c, view_c = _f32(albedo), _f32(normal), _f32(view)
        rgb = torch.empty(n, 3, device=normal.device, dtype=torch.float32)
        srgb, drgb = torch.empty_like(rgb), torch.empty_like(rgb)
        call('nefii_sg_render_forward', _ptr(lgt_c), lgt_c.shape[0], _ptr(spec_c), _ptr(rough_c), _ptr(albedo_c),
             _ptr(normal_c), _ptr(view_c), n, _ptr(rgb), _ptr(srgb), _ptr(drgb))
        ctx.save_for_backward(lgt_c, spec_c, rough_c, albedo_c, normal_c, view_c)
        ctx.spec_shape = tuple(spec.shape)
        ctx.set_materialize_grads(False)        # the specular / diffuse parts usually take no part in the loss: NULL, not zeros
        return rgb, srgb, drgb

    @staticmethod
    def backward(ctx, d_rgb, d_s, d_d):
        lgt, spec, rough, albedo, normal, view = ctx.saved_tensors
        n = normal.shape[0]
        if d_rgb is None and d_s is None and d_d is None:
            return None, None, None, None, None, None
        g_alb = torch.empty_like(albedo)
        acc = torch.zeros(4 + lgt.numel(), device=albedo.device, dtype=torch.float32)      # the accumulators: one fill
        g_rough, g_spec, g_lgt = acc[0:1].view(1, 1), acc[1:4].view(1, 3), acc[4:].view_as(lgt)
        if d_rgb is None:
            d_rgb = torch.zeros(n, 3, device=albedo.device, dtype=torch.float32)
        d_rgb, d_s, d_d = _f32(d_rgb), _f32(d_s), _f32(d_d)     # keep converted copies alive across the launch call
        call('nefii_sg_render_backward', _ptr(lgt), lgt.shape[0], _ptr(spec), _ptr(rough), _ptr(albedo), _ptr(normal),
             _ptr(view), n, _ptr(d_rgb), _ptr(d_s), _ptr(d_d), _ptr(g_alb), _ptr(g_rough), _ptr(g_spec), _ptr(g_lgt))
        if ctx.spec_shape[-1] == 1:
            g_spec = g_spec.sum(-1, keepdim=True)
        return g_lgt, g_spec, g_rough, g_alb, None, None


class EnvRadianceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lgt, dirs, eps):
        check_light(lgt)
        lgt_c, dirs_c = _f32(lgt), _f32(dirs)
        n = dirs_c.shape[0]
        rgb = torch.empty(n, 3, device=dirs.device, dtype=torch.float32)
        call('nefii_env_radiance_forward', _ptr(lgt_c), lgt_c.shape[0], _ptr(dirs_c), n, eps, _ptr(rgb))
        ctx.save_for_backward(lgt_c, dirs_c)
        ctx.eps = eps
        return rgb

    @staticmethod
    def backward(ctx, d_rgb):
        lgt, dirs = ctx.saved_tensors
        g = torch.zeros_like(lgt)
        d_rgb = _f32(d_rgb)
        call('nefii_env_radiance_backward', _ptr(lgt), lgt.shape[0], _ptr(dirs), dirs.shape[0], ctx.eps, _ptr(d_rgb), _ptr(g))
        return g, None, None


# ---- Monte-Carlo direct + indirect shading ----------------------------------------------------------
def mis_sample(lgt, rough, normal, view, uniforms):
    """-> wi [3,n,3], own_pdf [3,n], pdf_table [3,n,3]   (no gradient: the reference samples under no_grad)."""
    check_light(lgt)
    n = normal.shape[0]
    dev = normal.device
    wi = torch.empty(3, n, 3, device=dev, dtype=torch.float32)
    own = torch.empty(3, n, device=dev, dtype=torch.float32)
    tab = torch.empty(3, n, 3, device=dev, dtype=torch.float32)
    lgt_c = _f32(lgt)
    rough_c, normal_c, view_c, uni_c = _f32(rough).reshape(-1), _f32(normal), _f32(view), _f32(uniforms)
    call('nefii_mis_sample', _ptr(lgt_c), lgt_c.shape[0], _ptr(rough_c), _ptr(normal_c), _ptr(view_c), _ptr(uni_c), n,
         _ptr(wi), _ptr(own), _ptr(tab))
    return wi, own, tab


class McShadeFn(torch.autograd.Function):
    """Sum over the 3 MIS samples of (direct*vis + (1-vis)*indirect) x (GGX specular + Lambert);
    differentiable wrt light, indirect, albedo, roughness and (if it requires grad) the global specular."""

    @staticmethod
    def forward(ctx, spec, rough, albedo, normal, view, wi, own, tab, light, vis, indirect):
        n = normal.shape[0]
        t = [_f32(spec.expand(1, 3)), _f32(rough).reshape(-1), _f32(albedo), _f32(normal), _f32(view), _f32(wi),
             _f32(own), _f32(tab), _f32(light), _f32(vis), _f32(indirect)]
        rgb = torch.empty(n, 3, device=normal.device, dtype=torch.float32)
        srgb, drgb = torch.empty_like(rgb), torch.empty_like(rgb)
        call('nefii_mc_shade_forward', *[_ptr(x) for x in t], n, _ptr(rgb), _ptr(srgb), _ptr(drgb))
        ctx.save_for_backward(*t)
        ctx.spec_grad = spec.requires_grad
        ctx.spec_shape = tuple(spec.shape)
        ctx.rough_shape = tuple(rough.shape)
        return rgb, srgb, drgb

    @staticmethod
    def backward(ctx, d_rgb, d_s, d_d):
        t = ctx.saved_tensors
        n = t[3].shape[0]
        dev = t[3].device
        g_light = torch.empty(3, n, 3, device=dev, dtype=torch.float32)
        g_ind = torch.empty_like(g_light)
        g_alb = torch.empty(n, 3, device=dev, dtype=torch.float32)
        g_rough = torch.empty(n, device=dev, dtype=torch.float32)
        g_spec = torch.zeros(1, 3, device=dev, dtype=torch.float32) if ctx.spec_grad else None
        d_rgb, d_s, d_d = _f32(d_rgb), _f32(d_s), _f32(d_d)
        call('nefii_mc_shade_backward', *[_ptr(x) for x in t], n, _ptr(d_rgb), _ptr(d_s), _ptr(d_d), _ptr(g_light), _ptr(g_ind),
             _ptr(g_alb), _ptr(g_rough), _ptr(g_spec))
        if g_spec is not None and ctx.spec_shape[-1] == 1:
            g_spec = g_spec.sum(-1, keepdim=True)
        return (g_spec, g_rough.reshape(ctx.rough_shape), g_alb, None, None, None, None, None, g_light, None, g_ind)
