"""fp64 numpy oracle of the rotated map light, by composition of tests/envlight_ref.py and
tests/bounce_ref.py.  R is world-from-light, row-major (lighting.rotate_light_sgs' convention) - the kernel's fp32 matrix
promoted to fp64.  For row vectors d [n, 3]: R^T d is d @ R (world -> light), R d is d @ R.T (light -> world).

    radiance / pdf / texel_of / edge_distance   of the rotated light along d: the unrotated ones along d @ R
    sample                                      the unrotated sample's direction @ R.T, its texel and pdf unchanged
    weight_at                                   bounce_ref.weight_at in the light's frame (wo, n, v all @ R): the BRDF and
                                                the two BRDF densities only see dot products, the texel and its sin(phi)
                                                are the rotated lookups

rotations() are the cases of the GPU tests; yaw() / general() build them."""
import numpy as np

import bounce_ref as br
import envlight_ref as er

UP_AXIS = {'mitsuba': 1, 'blender': 2}


def f32(R):
    """a rotation as the kernel holds it: rounded to fp32, promoted back"""
    return np.asarray(R, np.float64).astype(np.float32)


def yaw(angle_deg, coord):
    """the turntable's rotation: about y for mitsuba (from_euler('yxz', [a, 0, 0])), about z for blender
    (from_euler('xyz', [0, 0, a])) - right-handed about the up axis in both; fp32 [3, 3]"""
    a = np.deg2rad(np.float64(angle_deg))
    c, s = np.cos(a), np.sin(a)
    if coord == 'mitsuba':
        R = np.array([[c, 0., s], [0., 1., 0.], [-s, 0., c]])
    else:
        R = np.array([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]])
    return f32(R)


def general(angles_deg=(25., -40., 70.)):
    """Rz(c) Ry(b) Rx(a) of the Euler angles (a, b, c) in degrees (scipy's from_euler('xyz', .): extrinsic); fp32"""
    a, b, c = np.deg2rad(np.asarray(angles_deg, np.float64))
    Rx = np.array([[1., 0., 0.], [0., np.cos(a), -np.sin(a)], [0., np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0., np.sin(b)], [0., 1., 0.], [-np.sin(b), 0., np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0.], [np.sin(c), np.cos(c), 0.], [0., 0., 1.]])
    return f32(Rz @ Ry @ Rx)


def column_yaw_deg(m, W):
    """the yaw that moves the map by m whole columns"""
    return 360. * m / W


def roll_columns(m, coord):
    """np.roll(map, roll_columns(m, coord), axis=1) is the map under yaw(column_yaw_deg(m, W), coord).  u grows with
    theta in the mitsuba mapping and a right-handed yaw about y DEcreases theta = atan2(z, x): the light's texel j shows
    up at j - m; blender's u falls with theta and its yaw about z INcreases theta = atan2(y, x): j - m again."""
    return -m


def rotations(coord, W):
    """the four rotations of the GPU tests for a W-column map: identity, a column-aligned yaw (3 columns), a yaw that is
    not column-aligned (37 degrees) and one general rotation (Euler 25, -40, 70); fp32 [4, 3, 3]"""
    return np.stack([np.eye(3, dtype=np.float32), yaw(column_yaw_deg(3, W), coord), yaw(37., coord), general()])


def to_light(d, R):
    return np.asarray(d, np.float64) @ np.asarray(R, np.float64)


def to_world(d, R):
    return np.asarray(d, np.float64) @ np.asarray(R, np.float64).T


def radiance(envmap, coord, d, R):
    return er.radiance(envmap, coord, to_light(d, R))


def pdf(M, C, coord, d, R):
    return er.pdf(M, C, coord, to_light(d, R))


def texel_of(d, H, W, coord, R):
    return er.texel_of(to_light(d, R), H, W, coord)


def edge_distance(d, H, W, coord, R):
    """of the ROTATED direction: the texel under d @ R is undecided in fp32 within ~1e-5 rad of an edge"""
    return er.edge_distance(to_light(d, R), H, W, coord)


def sample(M, C, coord, u_row, u_col, R):
    """-> (i, j, d [n, 3] in the world, own pdf [n]): the texel and the density are the unrotated draw's"""
    i, j, d, p = er.sample(M, C, coord, u_row, u_col)
    return i, j, to_world(d, R), p


def weight_at(wo, envmap, M, C, coord, n, v, rough, albedo, spec, R, dtype=np.float64, drawn=None):
    """bounce_ref.weight_at under the rotated light for world directions wo [m, 3] (n, v: [3] or [m, 3]); R [3, 3] or one
    per row [m, 3, 3]"""
    R = np.asarray(R, np.float64)
    rot = (lambda x: np.asarray(x, np.float64) @ R) if R.ndim == 2 else \
        (lambda x: np.einsum('mj,mji->mi', np.broadcast_to(np.asarray(x, np.float64), (R.shape[0], 3)), R))
    return br.weight_at(rot(wo), envmap, M, C, coord, rot(n), rot(v), rough, albedo, spec, dtype, drawn)


def sample_texels(envmap, M, C, coord, n, v, rough, albedo, spec, uniforms, R, dtype=np.float64):
    """bounce_ref.sample_texels under the rotated light -> (k, wo in the world, mix, weight, drawn); R [3, 3] or
    [m, 3, 3].  The two BRDF techniques draw in the world (their tangent frame hangs on the normal's x component, it does
    not rotate along); the map's draw is rotated out."""
    u = np.asarray(uniforms, np.float32)
    m = u.shape[0]
    Rm = np.broadcast_to(np.asarray(R, np.float64), (m, 3, 3))
    k = br.technique(u[:, 0])
    nn, vv = (br._rows(x, m, dtype, 3) for x in (n, v))
    rr = br._rows(rough, m, dtype)
    u1, u2 = u[:, 1].astype(dtype), u[:, 2].astype(dtype)
    wo = np.zeros((m, 3), dtype)
    s0, s1, s2 = k == 0, k == 1, k == 2
    wo[s0] = br.sample_cos(nn[s0], u1[s0], u2[s0])
    wo[s1] = br.sample_ggx(nn[s1], vv[s1], rr[s1], u1[s1], u2[s1])
    di, dj = np.zeros(m, np.int64), np.zeros(m, np.int64)
    if s2.any():
        i, j, d, _ = er.sample(M, C, coord, u[s2, 1], u[s2, 2])
        wo[s2] = np.einsum('mij,mj->mi', Rm[s2], d).astype(dtype)
        di[s2], dj[s2] = i, j
    drawn = (s2, di, dj)
    mix, weight = weight_at(wo, envmap, M, C, coord, nn, vv, rr, albedo, spec, Rm, dtype, drawn)
    return k, wo, mix, weight, drawn
