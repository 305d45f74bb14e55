"""The lat-long environment map light (include/nefii_amd.h ABI 18) and its rotations."""
import torch

from .. import _lib
from ._call import _f32, _ptr, call, check_tensor, need_gpu


ENVLIGHT_COORDS = {'mitsuba': 0, 'blender': 1}


def _envlight_coord(coordinate_type):
    if coordinate_type not in ENVLIGHT_COORDS:
        raise ValueError('coordinate_type is mitsuba or blender, not %r' % (coordinate_type,))
    return ENVLIGHT_COORDS[coordinate_type]


def _envlight_map(envmap):
    """envmap must be a contiguous float32 [H, W, 3] GPU tensor with 1 <= H, W and H * W < 2^31 -> (H, W)"""
    check_tensor('envmap', envmap, torch.float32, (None, None, 3))
    H, W = envmap.shape[:2]
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise ValueError('envmap of %d x %d texels: the light needs at least one and fewer than 2^31' % (H, W))
    need_gpu(envmap)
    return H, W


def _envlight_table(table, H, W):
    lib = _lib.lib()
    if table.dtype != torch.uint8 or table.dim() != 1 or table.numel() != lib.nefii_envlight_table_bytes(H, W):
        raise ValueError('table must be the uint8 [%d] tensor envlight_table built for a %d x %d map'
                         % (lib.nefii_envlight_table_bytes(H, W), H, W))


def _dirs3(dirs, what='dirs'):
    if dirs.dim() != 2 or dirs.shape[1] != 3:
        raise ValueError('%s must be [n, 3], got %s' % (what, tuple(dirs.shape)))
    return _f32(dirs)


def envlight_table(envmap):
    """the sampling table of a map light (marginal and conditional CDFs, nefii_envlight_build): uint8 device bytes"""
    H, W = _envlight_map(envmap)
    # zero-filled: the alignment padding between the parts is then deterministic too, and equal tables compare equal
    table = torch.zeros(_lib.lib().nefii_envlight_table_bytes(H, W), device=envmap.device, dtype=torch.uint8)
    call('nefii_envlight_build', _ptr(envmap), H, W, _ptr(table))
    return table


# ---- the map light under rotations ------------------------------------------------------------------
def envlight_rotations(rot):
    """rot must be a contiguous float32 [A, 3, 3] GPU tensor, A >= 1 (R: world-from-light, row-major) -> (A, identity):
    identity [A] int32 marks the rotations whose nine floats are exactly the identity; the kernels skip the products for
    them and reproduce the unrotated entry points bit for bit."""
    check_tensor('rot', rot, torch.float32, (None, 3, 3))
    if rot.shape[0] < 1:
        raise ValueError('rot must hold at least one rotation, got %s' % (tuple(rot.shape),))
    need_gpu(rot)
    eye = torch.eye(3, device=rot.device, dtype=torch.float32)
    return rot.shape[0], (rot == eye).reshape(-1, 9).all(dim=1).to(torch.int32).contiguous()


def _envlight_rot_index(rot_index, A, n, device):
    """rot_index: None (rotation 0 for every item) or int32 [n] with values in [0, A) on the items' device"""
    if rot_index is None:
        return None
    if rot_index.dtype != torch.int32 or rot_index.dim() != 1 or rot_index.shape[0] != n:
        raise ValueError('rot_index must be int32 [%d], got %s %s' % (n, rot_index.dtype, tuple(rot_index.shape)))
    if n > 0:
        lo, hi = int(rot_index.min()), int(rot_index.max())
        if lo < 0 or hi >= A:
            raise ValueError('rot_index holds %d .. %d, the %d rotations are 0 .. %d' % (lo, hi, A, A - 1))
    if rot_index.device != device:
        raise ValueError('rot_index is on %s, the items on %s' % (rot_index.device, device))
    return rot_index.contiguous()


# Each operation below is one body: without rot it calls the unrotated entry point (and so launches the kernel that has
# the identity compiled in), with rot [A, 3, 3] the _rot one.  rot is looked at before anything else.
def _envlight_rot(rot):
    """-> (A, identity) of envlight_rotations, (1, None) without a rotation"""
    return (1, None) if rot is None else envlight_rotations(rot)


def _rot_given(rot):
    """the rot of a public _rot wrapper: None, which selects the unrotated entry point below, is no rotation"""
    if rot is None:
        raise ValueError('rot must be a [A, 3, 3] tensor with A >= 1, got NoneType')
    return rot


def _envlight_call(name, head, rot_args, tail):
    """nefii_envlight_<name>(*head, *tail, stream) or nefii_envlight_<name>_rot(*head, *rot_args, *tail, stream)"""
    call('nefii_envlight_' + name + ('_rot' if rot_args else ''), *head, *rot_args, *tail)


def _envlight_mis(envmap, table, coordinate_type, rough, normal, view, uniforms, rot=None):
    """-> wi [A,3,n,3], own_pdf [A,3,n], pdf_table [A,3,n,3], light [A,3,n,3]; A = 1 without rot"""
    A, ident = _envlight_rot(rot)
    coord = _envlight_coord(coordinate_type)
    H, W = _envlight_map(envmap)
    _envlight_table(table, H, W)
    normal_c, view_c = _dirs3(normal, 'normal'), _dirs3(view, 'view')
    n = normal_c.shape[0]
    rough_c, uni_c = _f32(rough).reshape(-1), _f32(uniforms)
    if view_c.shape[0] != n or rough_c.shape[0] != n or uni_c.shape != (n, 7):
        raise ValueError('roughness [n], normal / view [n, 3] and uniforms [n, 7] must agree on n = %d' % n)
    if A > 65535:
        raise ValueError('%d rotations: one launch takes at most 65535' % A)
    wi, own, tab, light = (torch.empty(A, *s, device=normal.device, dtype=torch.float32)
                           for s in ((3, n, 3), (3, n), (3, n, 3), (3, n, 3)))
    _envlight_call('mis_sample', (_ptr(envmap), _ptr(table), H, W, coord),
                   () if rot is None else (_ptr(rot), _ptr(ident), A),
                   (_ptr(rough_c), _ptr(normal_c), _ptr(view_c), _ptr(uni_c), n, _ptr(wi), _ptr(own), _ptr(tab), _ptr(light)))
    return wi, own, tab, light


def _envlight_bounce(envmap, table, coordinate_type, specular, rough, albedo, normal, view, uniforms, want_mix=False,
                     rot=None, rot_index=None):
    A, ident = _envlight_rot(rot)
    coord = _envlight_coord(coordinate_type)
    normal_c, view_c, albedo_c = _dirs3(normal, 'normal'), _dirs3(view, 'view'), _dirs3(albedo, 'albedo')
    m = normal_c.shape[0]
    idx = _envlight_rot_index(rot_index, A, m, normal.device)
    spec_c, rough_c, uni_c = _f32(specular).reshape(-1), _f32(rough).reshape(-1), _f32(uniforms)
    if spec_c.shape[0] != 3:
        raise ValueError('specular must hold 3 values, got %s' % (tuple(specular.shape),))
    if view_c.shape[0] != m or albedo_c.shape[0] != m or rough_c.shape[0] != m or uni_c.shape != (m, 3):
        raise ValueError('roughness [m], albedo / normal / view [m, 3] and uniforms [m, 3] must agree on m = %d' % m)
    H, W = _envlight_map(envmap)
    _envlight_table(table, H, W)
    dev = normal.device
    wo = torch.empty(m, 3, device=dev, dtype=torch.float32)
    weight = torch.empty(m, 3, device=dev, dtype=torch.float32)
    mix = torch.empty(m, device=dev, dtype=torch.float32) if want_mix else None
    _envlight_call('bounce_sample', (_ptr(envmap), _ptr(table), H, W, coord),
                   () if rot is None else (_ptr(rot), _ptr(ident), A, _ptr(idx)),
                   (_ptr(spec_c), _ptr(rough_c), _ptr(albedo_c), _ptr(normal_c), _ptr(view_c), _ptr(uni_c), m, _ptr(wo),
                    _ptr(weight), _ptr(mix)))
    return (wo, weight, mix) if want_mix else (wo, weight)


def _envlight_radiance(envmap, coordinate_type, dirs, rot=None, rot_index=None):
    A, ident = _envlight_rot(rot)
    coord = _envlight_coord(coordinate_type)
    dirs_c = _dirs3(dirs)
    n = dirs_c.shape[0]
    idx = _envlight_rot_index(rot_index, A, n, dirs.device)
    H, W = _envlight_map(envmap)
    rgb = torch.empty(n, 3, device=dirs.device, dtype=torch.float32)
    _envlight_call('radiance', (_ptr(envmap), H, W, coord), () if rot is None else (_ptr(rot), _ptr(ident), A, _ptr(idx)),
                   (_ptr(dirs_c), n, _ptr(rgb)))
    return rgb


def _envlight_pdf(table, H, W, coordinate_type, dirs, rot=None, rot_index=None):
    A, ident = _envlight_rot(rot)
    if H < 1 or W < 1 or H * W >= 1 << 31:
        raise ValueError('bad map shape %d x %d' % (H, W))
    coord = _envlight_coord(coordinate_type)
    dirs_c = _dirs3(dirs)
    n = dirs_c.shape[0]
    idx = _envlight_rot_index(rot_index, A, n, dirs.device)
    _envlight_table(table, H, W)
    pdf = torch.empty(n, device=dirs.device, dtype=torch.float32)
    _envlight_call('pdf', (_ptr(table), H, W, coord), () if rot is None else (_ptr(rot), _ptr(ident), A, _ptr(idx)),
                   (_ptr(dirs_c), n, _ptr(pdf)))
    return pdf


def envlight_mis_sample(envmap, table, coordinate_type, rough, normal, view, uniforms):
    """-> wi [3,n,3], own_pdf [3,n], pdf_table [3,n,3], light [3,n,3]: mis_sample's outputs with the map as the third
    technique, and the map's radiance along the three directions (no gradient)."""
    return tuple(t[0] for t in _envlight_mis(envmap, table, coordinate_type, rough, normal, view, uniforms))


def envlight_mis_sample_rot(envmap, table, coordinate_type, rot, rough, normal, view, uniforms):
    """envlight_mis_sample under each of the A rotations rot [A, 3, 3], one launch -> wi [A,3,n,3], own_pdf [A,3,n],
    pdf_table [A,3,n,3], light [A,3,n,3]; slice a is what rot[a:a + 1] alone returns, rows 0-1 of wi / own_pdf and
    columns 0-1 of their pdf_table are the same bits in every slice (no gradient)."""
    return _envlight_mis(envmap, table, coordinate_type, rough, normal, view, uniforms, _rot_given(rot))


def envlight_bounce_sample(envmap, table, coordinate_type, specular, rough, albedo, normal, view, uniforms,
                           want_mix=False):
    """One recomputed bounce under the map at m secondary hits (nefii_envlight_bounce_sample): specular [3]
    (or [1, 3]), rough [m] (or [m, 1]), albedo / normal / view [m, 3], uniforms [m, 3] -> wo [m, 3], weight [m, 3]
    (, mix_pdf [m] with want_mix): one direction by one-sample MIS over cosine / GGX / map, and the hit's radiance estimate
    along view for unit visibility (no gradient)."""
    return _envlight_bounce(envmap, table, coordinate_type, specular, rough, albedo, normal, view, uniforms, want_mix)


def envlight_bounce_sample_rot(envmap, table, coordinate_type, rot, rot_index, specular, rough, albedo, normal, view,
                               uniforms, want_mix=False):
    """envlight_bounce_sample with hit p under rotation rot[rot_index[p]] (rot_index int32 [m], None: rotation 0 for every
    hit) -> wo [m, 3], weight [m, 3] (, mix_pdf [m])"""
    return _envlight_bounce(envmap, table, coordinate_type, specular, rough, albedo, normal, view, uniforms, want_mix,
                            _rot_given(rot), rot_index)


def envlight_radiance(envmap, coordinate_type, dirs):
    """the map's radiance (nearest texel) along dirs [n, 3] -> [n, 3]"""
    return _envlight_radiance(envmap, coordinate_type, dirs)


def envlight_radiance_rot(envmap, coordinate_type, rot, dirs, rot_index=None):
    """the rotated map's radiance along dirs [n, 3] -> [n, 3]: L(R^T d), R = rot[rot_index[p]] (None: rot[0])"""
    return _envlight_radiance(envmap, coordinate_type, dirs, _rot_given(rot), rot_index)


def envlight_pdf(table, H, W, coordinate_type, dirs):
    """the map technique's solid-angle pdf along dirs [n, 3] -> [n]"""
    return _envlight_pdf(table, H, W, coordinate_type, dirs)


def envlight_pdf_rot(table, H, W, coordinate_type, rot, dirs, rot_index=None):
    """the rotated map technique's solid-angle pdf along dirs [n, 3] -> [n]: p(R^T d)"""
    return _envlight_pdf(table, H, W, coordinate_type, dirs, _rot_given(rot), rot_index)
