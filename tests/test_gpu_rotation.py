"""The map light under a rotation on the GPU: the four nefii_envlight_*_rot entry points against their
unrotated twins (identity), against each other (batch slices), against the fp64 oracle (tests/rot_ref.py), against the
unrotated kernels on a rolled map (column-aligned yaw), and the bounce estimator's mean against the exact integral."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bounce_ref as br  # noqa: E402
import envlight_ref as er  # noqa: E402
import rot_ref as rr  # noqa: E402
import sg64  # noqa: E402
import test_gpu_bounce as tgb  # noqa: E402
import test_gpu_envlight as tge  # noqa: E402

DEV = torch.device('cuda')
pytestmark = pytest.mark.gpu

N = 50000
MAPS = [(16, 32), 'sun', 'zero_rows', 'all_zero']
SPEC = np.array([0.04, 0.5, 0.9])


def the_map(name):
    return tge.special_map(name)


def rots(coord, W):
    return torch.from_numpy(rr.rotations(coord, W)).to(DEV)


def signed_zero_dirs():
    """axis directions with either sign of zero in the other components: atan2f(-0, -1) is -pi, atan2f(+0, -1) is +pi -
    a product 1 x + 0 y + 0 z would lose the sign and move these across the seam"""
    out = []
    for axis in range(3):
        for s in (1., -1.):
            for z1 in (0., -0.):
                for z2 in (0., -0.):
                    d = [z1, z2]
                    d.insert(axis, s)
                    out.append(d)
    return np.array(out, np.float32)


def dirs_with_seams(n, seed):
    return np.concatenate([signed_zero_dirs(), tge.random_dirs(n - 24, seed)])


def hits(n, seed):
    r, albedo, nrm, view, uni = tgb.secondary_hits(n, seed)
    return [torch.tensor(SPEC, dtype=torch.float32, device=DEV)] + [x.to(DEV) for x in (r, albedo, nrm, view, uni)]


def eq(a, b):
    """bitwise, NaN-free"""
    return all(torch.equal(x, y) and bool(torch.isfinite(x).all()) for x, y in zip(a, b))


# ---- 1. the identity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('coord', er.COORDS)
@pytest.mark.parametrize('name', MAPS, ids=str)
def test_identity_rotation_is_the_unrotated_kernels_bitwise(name, coord):
    from nefii_amd import ops
    from nefii_amd.lighting import EnvmapLight
    env = the_map(name)
    H, W = env.shape[:2]
    light = EnvmapLight(torch.from_numpy(env), coord)
    one = torch.eye(3, device=DEV)[None].contiguous()
    four = rots(coord, W)
    assert torch.equal(four[0], one[0])
    zeros = torch.zeros(N, dtype=torch.int32, device=DEV)
    d = torch.from_numpy(dirs_with_seams(N, 11)).to(DEV)
    rgb, pdf = light.radiance(d), light.pdf(d)
    for rot, idx in ((one, None), (four, None), (four, zeros), (one, zeros)):
        assert torch.equal(ops.envlight_radiance_rot(light.envmap, coord, rot, d, idx), rgb)
        assert torch.equal(ops.envlight_pdf_rot(light.table, H, W, coord, rot, d, idx), pdf)
    r, nrm, view, uni = tge.surface_points(N, 3)
    plain = light.sample(r, nrm, view, uni)
    assert eq([x[0] for x in ops.envlight_mis_sample_rot(light.envmap, light.table, coord, one, r, nrm, view, uni)], plain)
    assert eq([x[0] for x in light.sample_rotations(four, r, nrm, view, uni)], plain)
    args = hits(N, 3)
    plain = ops.envlight_bounce_sample(light.envmap, light.table, coord, *args, want_mix=True)
    for rot, idx in ((one, None), (four, None), (four, zeros)):
        assert eq(ops.envlight_bounce_sample_rot(light.envmap, light.table, coord, rot, idx, *args, want_mix=True), plain)
    # the Python light: rotated(I) is the unrotated light, on today's code path
    same = light.rotated(np.eye(3))
    assert same.rotation is None and same.envmap is light.envmap and same.table is light.table
    assert torch.equal(same.radiance(d), rgb) and eq(same.sample(r, nrm, view, uni), light.sample(r, nrm, view, uni))


# ---- 2. batch slices ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('coord', er.COORDS)
@pytest.mark.parametrize('name', MAPS, ids=str)
def test_batch_slices_are_the_single_rotation_calls(name, coord):
    from nefii_amd import ops
    from nefii_amd.lighting import EnvmapLight
    env = the_map(name)
    H, W = env.shape[:2]
    light = EnvmapLight(torch.from_numpy(env), coord)
    four = rots(coord, W)
    r, nrm, view, uni = tge.surface_points(N, 3)
    batch = light.sample_rotations(four, r, nrm, view, uni)
    assert [tuple(x.shape) for x in batch] == [(4, 3, N, 3), (4, 3, N), (4, 3, N, 3), (4, 3, N, 3)]
    assert eq(batch, light.sample_rotations(four, r, nrm, view, uni))                       # no atomics
    for a in range(4):
        single = ops.envlight_mis_sample_rot(light.envmap, light.table, coord, four[a:a + 1].contiguous(), r, nrm, view, uni)
        assert eq([x[a] for x in batch], [x[0] for x in single])
        # the Python light under that rotation
        assert eq(light.rotated(four[a].cpu()).sample(r, nrm, view, uni), [x[a] for x in batch])
    wi, own, tab, L = batch
    # rows 0-1: the same bits in every slice, and nefii_mis_sample's under any SG light
    for a in range(1, 4):
        assert torch.equal(wi[a, :2], wi[0, :2]) and torch.equal(own[a, :2], own[0, :2])
        assert torch.equal(tab[a, :2, :, :2], tab[0, :2, :, :2])
        assert not torch.equal(wi[a, 2], wi[0, 2])
    g = torch.Generator().manual_seed(5)
    lgt = torch.randn(7, 7, generator=g).to(DEV)
    swi, sown, stab = ops.mis_sample(lgt, r, nrm, view, uni)
    assert torch.equal(swi[:2], wi[3, :2]) and torch.equal(sown[:2], own[3, :2])
    assert torch.equal(stab[:2, :, :2], tab[3, :2, :, :2])
    # the lookups with a rotation per direction: the per-rotation calls, interleaved
    d = torch.from_numpy(tge.random_dirs(N, 12)).to(DEV)
    idx = torch.randint(0, 4, (N,), generator=torch.Generator().manual_seed(1)).to(torch.int32).to(DEV)
    rgb = ops.envlight_radiance_rot(light.envmap, coord, four, d, idx)
    pdf = ops.envlight_pdf_rot(light.table, H, W, coord, four, d, idx)
    args = hits(N, 4)
    bounce = ops.envlight_bounce_sample_rot(light.envmap, light.table, coord, four, idx, *args, want_mix=True)
    for a in range(4):
        sel = idx == a
        lr = light.rotated(four[a].cpu())
        assert torch.equal(rgb[sel], lr.radiance(d)[sel]) and torch.equal(pdf[sel], lr.pdf(d)[sel])
        single = ops.envlight_bounce_sample_rot(light.envmap, light.table, coord, four[a:a + 1].contiguous(), None, *args,
                                                want_mix=True)
        assert eq([x[sel] for x in bounce], [x[sel] for x in single])
        assert eq(lr.bounce_sample(*args), single[:2])
    with pytest.raises(ValueError):
        ops.envlight_radiance_rot(light.envmap, coord, four, d, idx + 1)                    # an index of 4: out of range


# ---- 3. radiance and pdf against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize('coord', er.COORDS)
@pytest.mark.parametrize('name', MAPS, ids=str)
def test_rotated_radiance_and_pdf_match_the_oracle(name, coord):
    from nefii_amd.lighting import EnvmapLight
    env = the_map(name)
    H, W = env.shape[:2]
    light = EnvmapLight(torch.from_numpy(env), coord)
    M, C = tge.read_table(light.table, H, W)
    d = tge.random_dirs(N, 11)
    dt = torch.from_numpy(d).to(DEV)
    for a, R in enumerate(rr.rotations(coord, W)):
        lr = light.rotated(R)
        keep = rr.edge_distance(d, H, W, coord, R) > 1e-5
        assert keep.mean() >= 0.99, (a, keep.mean())              # the condition: at least 99 % of the directions
        rgb = lr.radiance(dt).cpu().numpy()
        assert np.array_equal(rgb[keep], rr.radiance(env, coord, d[keep], R)), a
        got, want = lr.pdf(dt).cpu().numpy()[keep], rr.pdf(M, C, coord, d[keep], R)
        err = np.abs(got - want) / np.maximum(want, 1e-300)
        print('%s %s rotation %d: kept %.4f, pdf max rel err %.3e' % (name, coord, a, keep.mean(), err[want > 0].max()
                                                                       if (want > 0).any() else 0.))
        assert np.allclose(got, want, rtol=1e-5, atol=0), a
        assert np.array_equal(lr.radiance(dt * 3.5).cpu().numpy()[keep], rgb[keep])         # normalised first


# ---- 4. a column-aligned yaw is the rolled map ---------------------------------------------------------------------------
@pytest.mark.parametrize('coord', er.COORDS)
@pytest.mark.parametrize('name', MAPS, ids=str)
def test_column_aligned_yaw_equals_the_rolled_map(name, coord):
    """independent of the oracle: the unrotated kernels on np.roll(map).  Radiance is bitwise.  The rolled map has a table
    of its own - other prefix sums - so the texel probabilities the two pdfs read differ by the tables' rounding: each
    stored CDF value is off by at most half an fp32 ulp of a number <= 1 (3e-8), a difference of two by 6e-8 in either
    table, 1.2e-7 between the tables, on top of the pdf's own 1e-5."""
    from nefii_amd.lighting import EnvmapLight
    env = the_map(name)
    H, W = env.shape[:2]
    m = 3
    R = rr.yaw(rr.column_yaw_deg(m, W), coord)
    light = EnvmapLight(torch.from_numpy(env), coord).rotated(R)
    rolled = EnvmapLight(torch.from_numpy(np.roll(env, rr.roll_columns(m, coord), axis=1).copy()), coord)
    d = tge.random_dirs(N, 13)
    keep = (rr.edge_distance(d, H, W, coord, R) > 1e-5) & (er.edge_distance(d, H, W, coord) > 1e-5)
    assert keep.mean() >= 0.99
    dt = torch.from_numpy(d[keep]).to(DEV)
    assert torch.equal(light.radiance(dt), rolled.radiance(dt))
    Mr, Cr = tge.read_table(rolled.table, H, W)
    i, j, _ = er.texel_of(d[keep], H, W, coord)
    pm = Mr[i] - np.where(i > 0, Mr[np.maximum(i - 1, 0)], 0.)
    pc = Cr[i, j] - np.where(j > 0, Cr[i, np.maximum(j - 1, 0)], 0.)
    got, want = light.pdf(dt).cpu().numpy().astype(np.float64), rolled.pdf(dt).cpu().numpy().astype(np.float64)
    tol = 1e-5 + 1.2e-7 / np.maximum(pm, 1e-30) + 1.2e-7 / np.maximum(pc, 1e-30)
    assert (np.abs(got - want) <= tol * want + 1e-30).all()


# ---- 5. the sampler against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize('coord', er.COORDS)
@pytest.mark.parametrize('name', MAPS, ids=str)
def test_rotated_sampler_matches_the_oracle_on_its_own_table(name, coord):
    """test_sampler_matches_the_oracle_on_its_own_table (tests/test_gpu_envlight.py) under each rotation"""
    from nefii_amd.lighting import EnvmapLight
    env = the_map(name)
    H, W = env.shape[:2]
    light = EnvmapLight(torch.from_numpy(env), coord)
    r, nrm, view, uni = tge.surface_points(N, 3)
    Rs = rr.rotations(coord, W)
    wi_b, own_b, tab_b, L_b = [x.cpu().numpy() for x in light.sample_rotations(torch.from_numpy(Rs), r, nrm, view, uni)]
    M, C = tge.read_table(light.table, H, W)
    u = uni.cpu().numpy()
    n64, v64, r64 = nrm.cpu().double().numpy(), view.cpu().double().numpy(), r.cpu().double().numpy()[:, 0]
    # sin(pi v) of the draw, for the own pdf's tolerance (as the unrotated test: v is rounded to fp32 in the kernel)
    i0, j0, _, p0 = er.sample(M, C, coord, u[:, 4], u[:, 5])
    prev = np.where(i0 > 0, M[np.maximum(i0 - 1, 0)], 0.)
    s = np.sin(np.pi * (i0 + np.clip((u[:, 4] - prev) / np.maximum(M[i0] - prev, 1e-30), 0, 1)) / H)
    tol = 1e-5 + 4e-7 / np.maximum(s, 1e-12)
    for a, R in enumerate(Rs):
        wi, own, tab, L = wi_b[a], own_b[a], tab_b[a], L_b[a]
        i, j, d, p = rr.sample(M, C, coord, u[:, 4], u[:, 5], R)
        assert np.array_equal(i, i0) and np.array_equal(j, j0) and np.array_equal(p, p0)
        ii, jj, _ = rr.texel_of(wi[2], H, W, coord, R)
        inside = rr.edge_distance(wi[2], H, W, coord, R) > 1e-5
        assert (ii[inside] == i[inside]).all() and (jj[inside] == j[inside]).all()
        dmax = np.abs(wi[2] - d).max()
        print('%s %s rotation %d: max |wi[2] - oracle| %.3e' % (name, coord, a, dmax))
        assert dmax < 2e-6
        want = np.maximum(p, 1e-6)
        assert (np.abs(own[2] - want) <= tol * want).all()
        assert np.array_equal(tab[2, :, 2], own[2])
        assert np.array_equal(L[2], env[i, j])
        for k in (0, 1):
            ok = rr.edge_distance(wi[k], H, W, coord, R) > 1e-5
            assert np.allclose(tab[k, ok, 2], rr.pdf(M, C, coord, wi[k, ok], R), rtol=1e-5, atol=0)
            assert np.array_equal(L[k, ok], rr.radiance(env, coord, wi[k, ok], R))
        w2 = wi[2].astype(np.float64)
        assert np.allclose(tab[2, :, 0], np.maximum((w2 * n64).sum(-1), 1e-6) / np.pi, rtol=1e-5, atol=1e-7)
        # the GGX column at the kernel's own w2, rel 1e-3 where fp32 can deliver it.  h = w2 + v carries 1e-7 per
        # component, so the unit half vector is off by about 3e-7 / |h|; pdf_h = c / (pi r^4 root^2), c = h.n, root = c^2 +
        # (1 - c^2) / r^4, moves by at most 4 c (1 / r^4 - 1) / root <= 488 (r = 0.3, c = 1) times that, plus 1 / c times
        # that through the leading c, plus 2 x 123 x 2e-7 from 1 - c^2 near c = 1.  With |h| > 0.5 and c > 1e-2 the three sum
        # to 6e-7 x 488 + 6e-5 + 5e-5 = 4e-4.  Outside (w2 within 29 degrees of -v, or a half vector in the tangent plane,
        # where the kernel clamps c at 1e-6) the column hangs on the last bits of h and is not compared.
        h = w2 + v64
        hl = np.linalg.norm(h, axis=-1)
        c = (h / np.maximum(hl, 1e-300)[:, None] * n64).sum(-1)
        sel = (r64 > 0.3) & (hl > 0.5) & (c > 1e-2)
        assert sel.sum() >= 0.5 * (r64 > 0.3).sum()
        want_ggx = tge.ggx_pdf64(w2[sel], n64[sel], v64[sel], r64[sel])
        print('%s %s rotation %d: GGX column compared on %.4f of r > 0.3, max rel err %.3e' % (
            name, coord, a, sel.sum() / (r64 > 0.3).sum(), (np.abs(tab[2, sel, 1] - want_ggx) / want_ggx).max()))
        assert np.allclose(tab[2, sel, 1], want_ggx, rtol=1e-3, atol=1e-9)


# ---- 6. the bounce sampler per sample ------------------------------------------------------------------------------------
@pytest.mark.parametrize('coord', er.COORDS)
@pytest.mark.parametrize('name', MAPS, ids=str)
def test_rotated_bounce_sample_matches_the_oracle(name, coord):
    """test_bounce_sample_matches_the_oracle (tests/test_gpu_bounce.py) with a rotation per hit: the general rotation for
    half of the hits, the other three for the rest"""
    from nefii_amd import ops
    from nefii_amd.lighting import EnvmapLight
    env = the_map(name)
    H, W = env.shape[:2]
    light = EnvmapLight(torch.from_numpy(env), coord)
    n = N
    r, albedo, nrm, view, uni = tgb.secondary_hits(n, 3)
    args = [torch.tensor(SPEC, dtype=torch.float32, device=DEV)] + [x.to(DEV) for x in (r, albedo, nrm, view, uni)]
    Rs = rr.rotations(coord, W)
    g = np.random.Generator(np.random.Philox(2))
    idx = np.where(g.random(n) < 0.5, 3, g.integers(0, 3, n)).astype(np.int32)
    wo, weight, mix = ops.envlight_bounce_sample_rot(light.envmap, light.table, coord, torch.from_numpy(Rs).to(DEV),
                                                     torch.from_numpy(idx).to(DEV), *args, want_mix=True)
    wo, weight, mix = [x.cpu().numpy() for x in (wo, weight, mix)]
    Rm = Rs[idx].astype(np.float64)
    J = sg64.Judge('rotated bounce %s %s' % (name, coord))
    J.require('finite', bool(np.isfinite(wo).all() and np.isfinite(weight).all() and np.isfinite(mix).all()), '')
    J.require('density floor', bool((mix >= np.float32(1e-6 / (3 * np.pi)) * (1 - 1e-6)).all()), 'min %.3e' % mix.min())
    if name == 'all_zero':
        J.require('zero map', bool((weight == 0).all()), 'weight is exactly 0')
    M, C = tge.read_table(light.table, H, W)
    n_, v_, r_, a_ = [x.double().numpy() for x in (nrm, view, r, albedo)]
    u = uni.numpy()
    k, w64, _, _, drawn = rr.sample_texels(env, M, C, coord, n_, v_, r_, a_, SPEC, u, Rm, np.float64)
    _, w32, _, _, _ = rr.sample_texels(env, M, C, coord, n_, v_, r_, a_, SPEC, u, Rm, np.float32)
    s2 = k == 2
    d2 = np.abs(wo[s2] - w64[s2]).max()
    J.require('direction 2 (map)', d2 < 2e-6, 'max |wo - oracle| %.3e over %d' % (d2, s2.sum()))
    for kk in (0, 1):
        sel = k == kk
        ok = (np.abs(wo[sel] - w64[sel]).max(-1) < 1e-4) & (np.abs(w32[sel] - w64[sel]).max(-1) < 1e-4)
        J.require('direction %d' % kk, ok.mean() > 0.998, 'agree on %d of %d' % (ok.sum(), sel.sum()))
    light_dir = np.einsum('mj,mji->mi', wo.astype(np.float64), Rm)                          # R^T wo per hit
    keep = s2 | (er.edge_distance(light_dir, H, W, coord) > 1e-5)
    J.require('texel edges', (~keep).mean() < 0.02, 'left out %d of %d' % ((~keep).sum(), n))
    m64, g64 = rr.weight_at(wo, env, M, C, coord, n_, v_, r_, a_, SPEC, Rm, np.float64, drawn)
    m32, g32 = rr.weight_at(wo, env, M, C, coord, n_, v_, r_, a_, SPEC, Rm, np.float32, drawn)
    t = torch.from_numpy
    J.quantiles('mix_pdf', t(mix[keep]), t(m64[keep]), t(m32[keep]), qs=tgb.GGX_QS)
    J.quantiles('weight', t(weight[keep]), t(g64[keep]), t(g32[keep]), qs=tgb.GGX_QS)
    for kk in range(3):
        sel = keep & (k == kk)
        J.quantiles('weight, technique %d' % kk, t(weight[sel]), t(g64[sel]), t(g32[sel]), qs=tgb.GGX_QS)
    J.done()


# ---- 7. the bounce estimator's mean against the exact integral -----------------------------------------------------------
def gpu_mean(light, R, nrm, v, rough, albedo, spec, seed):
    """test_gpu_bounce.gpu_mean under light.rotated(R)"""
    return tgb.gpu_mean(light.rotated(R), nrm, v, rough, albedo, spec, seed)


@pytest.mark.parametrize('coord,k', [(c[0], c[1]) for c in br.integral_cases()], ids=lambda x: str(x))
def test_rotated_mean_matches_the_exact_integral(coord, k):
    """The integral of the rotated light at (n, v) is the unrotated one at (R^T n, R^T v): |mean of 2^20 kernel draws
    under the general rotation - that integral| <= 5 se, se = the ORACLE estimator's standard deviation at (R^T n, R^T v)
    (2^18 fp64 draws on the CPU) / sqrt(2^20), test_mean_matches_the_exact_integral's rule and cases"""
    from nefii_amd.lighting import EnvmapLight
    _, _, nrm, v, rough = [c for c in br.integral_cases() if c[0] == coord and c[1] == k][0]
    R = rr.general()
    nl, vl = rr.to_light(nrm, R), rr.to_light(v, R)
    env = br.bright_texel_map()
    light = EnvmapLight(torch.from_numpy(env), coord)
    _, _, std, _ = br.estimate(env, coord, nl, vl, rough, br.ALBEDO, br.SPEC, tgb.ORACLE_DRAWS,
                               1000 + 16 * (coord == 'blender') + k)
    se = std / np.sqrt(tgb.DRAWS)
    s, d = er.integral(env, coord, nl, vl, rough, br.ALBEDO, br.SPEC, sub=8, fine=64)
    m = gpu_mean(light, R, nrm, v, rough, br.ALBEDO, br.SPEC, 300 + k)
    print('%s %d rough %.3f: mean %s integral %s deviation %s se' % (coord, k, rough, m, s + d, np.abs(m - (s + d)) / se))
    assert (np.abs(m - (s + d)) <= 5 * se).all(), (coord, k, rough, m, s + d, se)
