"""The variance-guided denoiser without a GPU: what the oracle (tests/denoise_var_ref.py) does to the shadow
scene beside 6j's filter, the moments and the filter's edge rules on small cases, and the plumbing - symbols, the frame loop's
extra keys, the refusals of denoise_outputs and of both command lines."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import denoise_ref as dr  # noqa: E402
import denoise_var_ref as vr  # noqa: E402

P = vr.START


# ---- 1. against 6j's filter on the shadow scene -----------------------------------------------------------------------
@pytest.fixture(scope='module')
def shadow_errors():
    """rays -> per signal (noisy, 6j's cascade, variance-guided) relative RMSE against the clean signal, 48 x 64"""
    res = {}
    for R in (8, 32):
        g0, g1, clean, s4 = vr.shadow_scene(48, 64, R, 0)
        valid = g0[..., 3] > 0.5
        new = vr.cascade_var(g0, g1, s4, **P)
        old = dr.cascade(g0, g1, s4[..., :3], **dr.START)
        res[R] = [(dr.rel_rmse(s4[s, ..., :3], clean[s], valid), dr.rel_rmse(old[s], clean[s], valid),
                   dr.rel_rmse(new[s, ..., :3], clean[s], valid)) for s in range(2)]
        print('%2d rays: noisy / 6j / variance-guided  diffuse light %.4f / %.4f / %.4f   specular %.4f / %.4f / %.4f'
              % ((R,) + res[R][0] + res[R][1]))
    return res


def test_variance_guided_filter_beats_the_noisy_input_and_6j(shadow_errors):
    """conditions, not tolerances; measured: 8 rays 0.0953 / 0.0701 / 0.0207 and 0.1149 / 0.1030 / 0.0643, 32 rays
    0.0478 / 0.0686 / 0.0117 and 0.0598 / 0.0919 / 0.0332 (noisy / 6j / variance-guided; diffuse light and specular)"""
    for R in (8, 32):
        for s in range(2):
            noisy, old, new = shadow_errors[R][s]
            assert new < noisy and new < old, (R, s, noisy, old, new)
    for s in range(2):
        assert shadow_errors[32][s][2] < shadow_errors[8][s][2]


def test_6j_makes_the_32_ray_shadow_scene_worse(shadow_errors):
    """the defect this feature answers: at 32 rays the fixed relative-luminance stop blurs the shadow edge by more than the
    noise it removes"""
    noisy, old, _ = shadow_errors[32][0]
    assert old > noisy, (noisy, old)


# ---- 2. moments -------------------------------------------------------------------------------------------------------
def test_moments_hand_computed():
    """2 pixels, 3 rays.  Pixel 0: grey samples 1, 2, 3 under albedo 0.5 -> light 2, 4, 6, mean 4, Y = the grey value (the
    Rec. 709 weights sum to 1), sum of squared deviations 8, v = 8 / (3 * 2); specular 0, 3, 3 in the red channel only: mean 2,
    e = 0.2126 * (0, 3, 3), v = 0.2126^2 * 6 / 6.  Pixel 1: equal samples."""
    diffuse = np.array([[1.] * 3, [2.] * 3, [3.] * 3] + [[0.3, 0.6, 0.9]] * 3)
    albedo = np.array([[0.5] * 3] * 3 + [[0.2, 0.4, 0.8]] * 3)
    specular = np.array([[0., 0., 0.], [3., 0., 0.], [3., 0., 0.]] + [[0.7, 0.1, 0.2]] * 3)
    out = vr.moments(diffuse, albedo, specular, np.ones(6, bool), 3)
    assert out.shape == (2, 2, 4)
    assert np.abs(out[0, 0] - [4., 4., 4., 8. / 6.]).max() < 1e-14
    assert np.abs(out[1, 0] - [2., 0., 0., 0.2126 ** 2]).max() < 1e-14
    assert np.abs(out[0, 1, :3] - [1.5, 1.5, 1.125]).max() < 1e-14 and np.abs(out[1, 1, :3] - [0.7, 0.1, 0.2]).max() < 1e-14
    assert out[0, 1, 3] == 0. and out[1, 1, 3] == 0.                                # exactly


def test_moments_equal_samples_floor_misses_and_nan():
    rng = np.random.Generator(np.random.Philox(7))
    R, n = 5, 6
    d, a, s = (rng.uniform(0.2, 2., size=(n, R, 3)).astype(np.float32) for _ in range(3))
    d[0], a[0], s[0] = d[0, :1], a[0, :1], s[0, :1]                                  # pixel 0: equal samples
    a[1] = [1e-5, 0.5, 1e-4]                                                        # pixel 1: albedo under the floor in two channels
    hit = np.ones((n, R), bool)
    hit[2, 3] = False                                                               # pixel 2: one ray missed
    d[3, 2, 1] = np.nan                                                             # pixel 3: a NaN diffuse sample
    s[4, 0, 0] = np.inf                                                             # pixel 4: an inf specular sample
    out = vr.moments(d.reshape(-1, 3), a.reshape(-1, 3), s.reshape(-1, 3), hit.reshape(-1), R)
    assert out[0, 0, 3] == 0. and out[1, 0, 3] == 0. and np.isfinite(out[:, 0]).all()
    assert np.abs(out[0, 1, :3] / (d[1].astype(np.float64).mean(0) / [vr.ALBEDO_FLOOR, 0.5, vr.ALBEDO_FLOOR]) - 1.).max() < 1e-15
    assert abs(vr.ALBEDO_FLOOR - 1e-3) < 1e-10
    assert (out[:, 2] == 0.).all()
    assert not np.isfinite(out[0, 3, 1]) and not np.isfinite(out[0, 3, 3]) and np.isfinite(out[1, 3]).all()
    assert not np.isfinite(out[1, 4, 0]) and not np.isfinite(out[1, 4, 3]) and np.isfinite(out[0, 4]).all()
    assert np.isfinite(out[:, 5]).all() and (out[:, 5, 3] > 0).all()
    a[5, 1, 2] = np.nan                                                             # a NaN albedo: signal 0 is not finite
    out = vr.moments(d.reshape(-1, 3), a.reshape(-1, 3), s.reshape(-1, 3), hit.reshape(-1), R)
    assert not np.isfinite(out[0, 5]).any() and np.isfinite(out[1, 5]).all()


# ---- 3. the filter's edge rules ---------------------------------------------------------------------------------------
def flat(H, W, S=2, seed=0, v=0.01):
    g0, g1 = dr.flat_guides(H, W)
    rng = np.random.Generator(np.random.Philox(seed))
    c4 = np.concatenate([rng.uniform(0.5, 1.5, size=(S, H, W, 3)), np.full((S, H, W, 1), v)], -1)
    return g0, g1, c4


def test_invalid_centre_is_bitwise_and_never_read():
    g0, g1, c4 = flat(9, 11)
    g0[4, 5, 3] = 0.
    c4[:, 4, 5] = [np.nan, -3., np.inf, -1.]
    for dtype in (np.float64, np.float32):
        out = vr.level_var(g0, g1, c4, 1, P['sigma_n'], P['sigma_x'], P['sigma_l'], dtype)
        assert np.array_equal(out[:, 4, 5], c4[:, 4, 5].astype(dtype), equal_nan=True)
        other = c4.copy()
        other[:, 4, 5] = 7.
        out2 = vr.level_var(g0, g1, other, 1, P['sigma_n'], P['sigma_x'], P['sigma_l'], dtype)
        keep = np.ones((9, 11), bool)
        keep[4, 5] = False
        assert np.array_equal(out2[:, keep], out[:, keep]) and np.isfinite(out[:, keep]).all()


def test_zero_weight_sum_carries_all_four_lanes():
    """one pixel whose only tap, itself, is not finite: the weights sum to 0 and the input comes back, negative variance
    included (max(v, 0) is for the uses of v, not for what is carried)"""
    g0, g1 = dr.flat_guides(1, 1)
    c4 = np.array([[[[np.nan, 1., 2., -0.5]]], [[[3., 4., 5., 0.25]]]])
    out = vr.level_var(g0, g1, c4, 1, 32., 0.1, 4.)
    assert np.array_equal(out, c4, equal_nan=True)
    # perpendicular normals everywhere but the centre's own: sigma_n zeroes every other tap, the centre keeps its colour and
    # its own (clamped) variance
    g0, g1, c4 = flat(5, 5)
    g0[..., :3] = (1., 0., 0.)
    g0[2, 2, :3] = (0., 0., 1.)
    out = vr.level_var(g0, g1, c4, 1, 32., 0.1, 4.)
    assert np.abs(out[:, 2, 2] - c4[:, 2, 2]).max() < 1e-15


def test_infinite_sigma_l_is_the_geometry_filter():
    g0, g1, _, s4 = vr.shadow_scene(20, 27, 4, 1)
    s4[0, 10, 10, 3] = 0.                                           # inf * sqrt(0) is not formed
    for step in (1, 4):
        out = vr.level_var(g0, g1, s4, step, P['sigma_n'], P['sigma_x'], np.inf)
        want = dr.level(g0, g1, s4[..., :3], step, P['sigma_n'], P['sigma_x'], np.inf)
        assert np.isfinite(out).all() and np.array_equal(out[..., :3], want)


def test_flat_noise_free_frame_keeps_colour_and_shrinks_variance():
    """A constant colour has equal luminances everywhere, so w = h_i h_j: the colour stays and, where all 25 taps are inside
    the image, a level multiplies a constant variance by sum (h_i h_j)^2 = (sum h^2)^2 = 0.2734375^2, the squared weights of
    denoise_ref.cascaded_kernel_1d(1); L levels by that to the L-th power.  (The taps of a later level are not independent
    any more, so the true variance left by L levels is the squared weights of the CASCADED kernel, (k_L^2).sum()^2 - 2.246e-4
    at L = 5 against 0.0747681^5 = 2.34e-6 carried: the carried lane under-estimates from level 1 on, as in SVGF.)"""
    H = W = 40
    g0, g1 = dr.flat_guides(H, W)
    c4 = np.broadcast_to(np.array([0.7, 0.2, 1.9, 0.04]), (2, H, W, 4)).copy()
    e1 = (dr.cascaded_kernel_1d(1) ** 2).sum() ** 2
    assert abs(e1 - 0.0747681) < 5e-8
    out = c4
    for l in range(3):
        out = vr.level_var(g0, g1, out, 1 << l, P['sigma_n'], P['sigma_x'], P['sigma_l'])
        assert np.abs(out[..., :3] / c4[..., :3] - 1.).max() < 1e-14
        m = 2 * ((1 << (l + 1)) - 1)                                # pixels whose taps of levels 0 .. l all stayed inside
        assert np.abs(out[:, m:H - m, m:W - m, 3] / (0.04 * e1 ** (l + 1)) - 1.).max() < 1e-13
    assert (out[..., 3] <= 0.04).all() and (out[..., 3] > 0).all()


def test_a_non_finite_tap_is_dropped_for_both_signals():
    g0, g1, c4 = flat(24, 31, seed=5)
    c4[1, 10, 12, 3] = np.inf                   # the variance lane of one signal: the pixel is out for both
    out = vr.level_var(g0, g1, c4, 1, P['sigma_n'], P['sigma_x'], np.inf)
    assert np.isfinite(out).all()
    w = np.outer(dr.H5, dr.H5)
    w[2, 2] = 0.
    for s in range(2):
        want = (w[..., None] * c4[s, 8:13, 10:15, :3]).sum((0, 1)) / w.sum()
        assert np.abs(out[s, 10, 12, :3] - want).max() < 1e-14
        assert abs(out[s, 10, 12, 3] - (w * w * np.where(np.isfinite(c4[s, 8:13, 10:15, 3]), c4[s, 8:13, 10:15, 3], 0.)).sum()
                   / w.sum() ** 2) < 1e-16
    # the centre that is not finite has no luminance: with the stop on its weights are still 1, and its neighbours drop it
    out = vr.level_var(g0, g1, c4, 1, P['sigma_n'], P['sigma_x'], P['sigma_l'])
    assert np.isfinite(out).all()
    want = (w[..., None] * c4[0, 8:13, 10:15, :3]).sum((0, 1)) / w.sum()
    assert np.abs(out[0, 10, 12, :3] - want).max() < 1e-14


# ---- 4. plumbing ------------------------------------------------------------------------------------------------------
def test_symbols_signatures_and_sources():
    import ctypes
    from nefii_amd import _lib, build, denoise, ops
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, 'include', 'nefii_amd.h')).read()
    assert 'int nefii_pixel_moments(' in header and 'int nefii_denoise_atrous_variance(' in header
    assert '#define NEFII_ABI_VERSION 19' in header and '#define NEFII_ALBEDO_FLOOR 1e-3f' in header
    assert 'nefii_denoise.hip' in build.SOURCES                 # the one file of the denoiser's kernels
    source = open(os.path.join(build.CSRC, 'nefii_denoise.hip')).read()
    assert 'int nefii_pixel_moments(' in source and 'int nefii_denoise_atrous_variance(' in source
    lib = _lib.lib()
    for name, n_args in (('nefii_pixel_moments', 8), ('nefii_denoise_atrous_variance', 12)):
        f = getattr(lib, name)
        assert f.restype is ctypes.c_int and len(f.argtypes) == n_args, name
    assert denoise.VARIANCE_DEFAULTS == dict(levels=5, sigma_n=32., sigma_x=0.1, sigma_l=4.)
    assert np.float32(denoise.ALBEDO_FLOOR) == np.float32(vr.ALBEDO_FLOOR)
    assert callable(ops.pixel_moments) and callable(ops.denoise_atrous_variance)


def test_entry_points_check_their_arguments_on_the_host():
    from nefii_amd import _lib
    lib = _lib.lib()
    E_ARG, E_SHAPE = -1, -2
    a, b, c, d, e = 256, 512, 768, 1024, 1280           # never dereferenced: every call below is refused on the host
    m = lib.nefii_pixel_moments
    for kw in (dict(diffuse=None), dict(albedo=None), dict(specular=None), dict(hit=None), dict(signals=None),
               dict(signals=1288), dict(rays=1), dict(rays=0), dict(rays=4097), dict(n=0), dict(n=-3)):
        k = dict(dict(diffuse=a, albedo=b, specular=c, hit=d, n=4, rays=8, signals=e), **kw)
        want = E_SHAPE if ('rays' in kw or 'n' in kw) else E_ARG
        assert m(k['diffuse'], k['albedo'], k['specular'], k['hit'], k['n'], k['rays'], k['signals'], None) == want, kw
    f = lib.nefii_denoise_atrous_variance
    good = dict(g0=a, g1=b, src=c, dst=d, n_signals=2, height=8, width=8, step=1, sigma_n=32., sigma_x=0.1, sigma_l=4.)

    def call(**kw):
        k = dict(good, **kw)
        return f(k['g0'], k['g1'], k['src'], k['dst'], k['n_signals'], k['height'], k['width'], k['step'], k['sigma_n'],
                 k['sigma_x'], k['sigma_l'], None)
    for kw in (dict(g0=None), dict(g1=None), dict(src=None), dict(dst=None), dict(dst=c), dict(n_signals=0), dict(n_signals=3),
               dict(step=0), dict(sigma_n=float('inf'))):
        assert call(**kw) == E_ARG, kw
    for side in (0, -5, 16385):
        assert call(height=side) == E_SHAPE and call(width=side) == E_SHAPE
    for k in ('sigma_n', 'sigma_x', 'sigma_l'):
        assert call(**{k: -1.}) == E_ARG and call(**{k: float('nan')}) == E_ARG, k


def test_ops_reject_cpu_tensors_and_bad_buffers():
    from nefii_amd import ops
    H, W = 4, 6
    g0, g1, src, dst = torch.zeros(H * W, 4), torch.zeros(H * W, 4), torch.zeros(2, H * W, 4), torch.zeros(2, H * W, 4)
    args = (H, W, 1, 32., 0.1, 4.)
    with pytest.raises(RuntimeError):                   # well-formed, but not on the GPU: no fallback
        ops.denoise_atrous_variance(g0, g1, src, dst, *args)
    for bad in [(g0[:, :3], g1, src, dst), (g0, g1[:-1], src, dst), (g0, g1, src[:, :, :3], dst), (g0, g1, src, dst[:1]),
                (g0, g1, torch.zeros(3, H * W, 4), torch.zeros(3, H * W, 4)), (g0.double(), g1, src, dst),
                (g0, g1, src.half(), dst), (g0, g1, src, src), (g0, g1, torch.zeros(2, H * W, 8)[:, :, ::2], dst)]:
        with pytest.raises(ValueError):
            ops.denoise_atrous_variance(*bad, *args)
    for bad_args in [(0, W, 1, 32., 0.1, 4.), (H, 16385, 1, 32., 0.1, 4.), (H, W, 0, 32., 0.1, 4.), (H, W, 1, -1., 0.1, 4.),
                     (H, W, 1, 32., float('nan'), 4.), (H, W, 1, 32., 0.1, -0.5), (H, W, 1, float('inf'), 0.1, 4.)]:
        with pytest.raises(ValueError):
            ops.denoise_atrous_variance(g0, g1, src, dst, *bad_args)
    R, n = 4, 12
    d, a, s, hit = torch.zeros(n, 3), torch.zeros(n, 3), torch.zeros(n, 3), torch.ones(n, dtype=torch.bool)
    with pytest.raises(RuntimeError):
        ops.pixel_moments(d, a, s, hit, R)
    with pytest.raises(RuntimeError):
        ops.pixel_moments(d, a, s, hit.to(torch.uint8), R)
    for bad in [(d, a, s, hit, 1), (d, a, s, hit, 4097), (d, a, s, hit, 5), (d[:, :2], a, s, hit, R), (d, a[:-1], s, hit, R),
                (d, a, s.double(), hit, R), (d, a, s, hit.float(), R), (d, a, s, hit[:-1], R),
                (d, torch.zeros(n, 6)[:, ::2], s, hit, R), (torch.zeros(0, 3), a, s, hit, R)]:
        with pytest.raises(ValueError):
            ops.pixel_moments(*bad)


def test_extra_keys_round_trip_and_are_off_by_default():
    from nefii_amd.training import render as R
    assert R.PACK_WIDTH == 27 and len(R.RENDER_KEYS) == 11
    g = torch.Generator().manual_seed(0)
    out = {k: torch.rand(7, w, generator=g) for k, w in R.RENDER_KEYS}
    for k in ('network_object_mask', 'object_mask'):
        out[k] = out[k][:, 0] > 0.5
    plain = R.pack_chunk(out)
    assert plain.shape == (7, 27)
    out['denoise_signals'] = torch.rand(7, 8, generator=g)
    assert torch.equal(R.pack_chunk(out), plain) and torch.equal(R.pack_chunk(out, ()), plain)     # today's bytes
    assert set(R.unpack_chunk(plain)) == {k for k, _ in R.RENDER_KEYS}
    extra = (('denoise_signals', 8),)
    mat = R.pack_chunk(out, extra)
    assert mat.shape == (7, 35) and torch.equal(mat[:, :27], plain)
    back = R.unpack_chunk(mat, extra)
    assert set(back) == {k for k, _ in R.RENDER_KEYS} | {'denoise_signals'}
    for k in back:
        assert torch.equal(back[k], out[k]), k
    with pytest.raises(KeyError):
        R.pack_chunk({k: v for k, v in out.items() if k != 'denoise_signals'}, extra)
    for bad in ((('denoise_signals', 7),),):
        with pytest.raises(ValueError):
            R.pack_chunk(out, bad)
    for bad in ((('points', 3),), (('x', 0),), (('x', 2), ('x', 2))):
        with pytest.raises(ValueError):
            R.check_extra_keys(bad)


class FakeRendererWithSignals(torch.nn.Module):
    """a per-pixel deterministic function of uv with render_frame's keys and denoise_signals [n, 8]"""

    def forward(self, inp):
        from nefii_amd.training import render as R
        uv = inp['uv'].reshape(-1, 2)
        rgb = torch.sigmoid(0.1 * uv @ torch.tensor([[1., -2., 0.5], [0.3, 0.7, -1.]]))
        out = {k: rgb * (i + 1) for i, (k, w) in enumerate(R.RENDER_KEYS) if w == 3}
        out['sg_roughness_values'] = rgb[:, :1]
        out['network_object_mask'] = rgb[:, 0] > 0.5
        out['object_mask'] = inp['object_mask'].reshape(-1)
        out['denoise_signals'] = torch.cat([rgb, rgb[:, :1] ** 2, 2. * rgb, rgb[:, 1:2] ** 2], dim=1)
        return out


def _frame_12x12():
    ys, xs = torch.meshgrid(torch.arange(12), torch.arange(12), indexing='ij')
    return {'uv': torch.stack([xs, ys], -1).reshape(1, -1, 2).float(), 'object_mask': torch.ones(1, 144, dtype=torch.bool),
            'pose': torch.eye(4)[None], 'intrinsics': torch.eye(4)[None]}


def _gather_worker(rank, world, port, tmp):
    import torch.distributed as dist
    from nefii_amd.training import render as R
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    merged = R.render_frame(FakeRendererWithSignals(), _frame_12x12(), 144, num_rays=1, memory_capacity_level=5, rank=rank,
                            world_size=world, extra_keys=(('denoise_signals', 8),))
    if rank == 0:
        torch.save(merged, os.path.join(tmp, 'render.pt'))
    else:
        assert merged is None
    dist.barrier()
    dist.destroy_process_group()


def test_extra_key_survives_the_two_rank_gather(tmp_path):
    """chunk / round-robin / gather / merge over gloo with the extra columns in the fixed-shape buffer, against one process"""
    import socket
    import torch.multiprocessing as mp
    from nefii_amd.training import render as R
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_gather_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    model, full = FakeRendererWithSignals(), _frame_12x12()
    single = R.render_frame(model, full, 144, num_rays=1, memory_capacity_level=5, extra_keys=(('denoise_signals', 8),))
    multi = torch.load(os.path.join(str(tmp_path), 'render.pt'))
    assert set(single) == set(multi) == {k for k, _ in R.RENDER_KEYS} | {'denoise_signals'}
    for k in single:
        if single[k].dtype == torch.bool:
            assert torch.equal(single[k], multi[k]), k
        else:
            assert torch.allclose(single[k], multi[k], atol=1e-6), k         # the chunk sizes differ: the last bit may
    assert single['denoise_signals'].shape == (144, 8)
    assert torch.allclose(single['denoise_signals'], model(full)['denoise_signals'], atol=1e-6)
    plain = R.render_frame(model, full, 144, num_rays=1, memory_capacity_level=5)
    assert set(plain) == {k for k, _ in R.RENDER_KEYS}
    for k in plain:
        assert torch.equal(plain[k], single[k]), k


def test_denoise_outputs_names_pixel_moments_when_the_key_is_missing():
    from nefii_amd import denoise
    outs = {k: torch.zeros(12, 3) for k in ('sg_diffuse_rgb_values', 'sg_specular_rgb_values', 'sg_rgb_values',
                                            'sg_diffuse_albedo_values', 'normal_values', 'points')}
    outs['network_object_mask'] = torch.ones(12, dtype=torch.bool)
    with pytest.raises(ValueError) as e:
        denoise.denoise_outputs(outs, (3, 4), variance=True)
    assert 'pixel_moments' in str(e.value)
    with pytest.raises(ValueError) as e:                # the key is there, in another shape
        denoise.denoise_outputs(dict(outs, denoise_signals=torch.zeros(12, 4)), (3, 4), variance=True)
    assert 'denoise_signals' in str(e.value)
    den = denoise.Denoiser(torch.zeros(12, 3), torch.zeros(12, 3), torch.ones(12, dtype=torch.bool), (3, 4))
    for bad in (torch.zeros(2, 3, 4, 3), torch.zeros(3, 3, 4, 4), torch.zeros(2, 3, 5, 4)):
        with pytest.raises(ValueError):
            den.filter_variance(bad)
    with pytest.raises(ValueError):
        den.filter_variance(torch.zeros(2, 3, 4, 4), levels=0)
    with pytest.raises(RuntimeError):                   # well-formed, on the CPU: no fallback
        den.filter_variance(torch.zeros(2, 3, 4, 4))


def test_model_refuses_pixel_moments_where_it_has_no_meaning():
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    model = IDRNetwork(conf.from_dict(syn.model_conf('conf', hidden=64)))
    assert model.pixel_moments is False
    model.pixel_moments = True
    ctx = {'multi': (1, 4, 8)}
    model.train()
    with pytest.raises(RuntimeError) as e:
        model.ray_moments(ctx, {})
    assert 'eval()' in str(e.value)
    with pytest.raises(RuntimeError):
        model({'uv': torch.zeros(1, 4, 8, 2)})
    model.eval()
    with pytest.raises(ValueError) as e:
        model.ray_moments({'multi': None}, {})
    assert 'multi' in str(e.value)
    with pytest.raises(ValueError) as e:
        model.ray_moments({'multi': (1, 4, 1)}, {})
    assert 'two rays' in str(e.value)
    kind, model.render_type = model.render_type, 'sg'
    with pytest.raises(ValueError) as e:
        model.ray_moments(ctx, {})
    assert 'Monte-Carlo' in str(e.value)
    model.render_type = kind


def _conf_file(tmp_path, render_type):
    p = tmp_path / ('%s.conf' % render_type)
    p.write_text('model {\n  render_type = %s\n}\n' % render_type)
    return str(p)


def refuse(*a, **kw):
    raise AssertionError('a refused command line must not build a runner')


@pytest.mark.parametrize('script', ['render', 'vis_rotate_envlight'])
def test_command_lines_refuse_before_a_gpu_is_touched(tmp_path, script, monkeypatch):
    import importlib
    mod = importlib.import_module('nefii_amd.scripts.' + script)
    monkeypatch.setattr(mod, 'RenderRunner' if script == 'render' else 'TurntableRunner', refuse)
    mc = _conf_file(tmp_path, 'pt_render_indirect_mlp')
    for argv, words in ((['--conf', mc, '--denoise_variance'], ('--denoise_variance', '--denoise')),
                        (['--conf', mc, '--denoise', '--denoise_sigma_luminance', '2'],
                         ('--denoise_sigma_luminance', '--denoise_variance')),
                        (['--conf', mc, '--denoise', '--denoise_variance', '--num_rays', '1'], ('--denoise_variance', '--num_rays')),
                        (['--conf', _conf_file(tmp_path, 'sg'), '--denoise', '--denoise_variance', '--num_rays', '8'],
                         ('--denoise_variance', 'Monte-Carlo')),
                        (['--conf', mc, '--denoise', '--denoise_variance', '--denoise_sigma_luminance', '-1'], ('sigma_l',))):
        with pytest.raises(SystemExit) as e:
            mod.main(argv)
        for w in words:
            assert w in str(e.value), (argv, str(e.value))
    with pytest.raises(AssertionError):                 # a well-formed line gets as far as the runner
        mod.main(['--conf', mc, '--denoise', '--denoise_variance', '--num_rays', '8', '--denoise_sigma_luminance', 'inf'])
