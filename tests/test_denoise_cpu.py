"""The guided a-trous denoiser without a GPU: the numpy oracle (tests/denoise_ref.py) against closed forms
and its own invariants, what it does to a noisy synthetic frame, and the refusals of the entry point, the op and the command
lines."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import denoise_ref as dr  # noqa: E402

P = dr.START


# ---- 1. the cascade ---------------------------------------------------------------------------------------------------
def test_cascaded_kernel_energy():
    """sum of squares of the cascaded dilated 1-D kernel (what is left of white noise's variance), and its square, the 2-D
    factor: the values computed for the issue, to the digits it gives"""
    k1, k5 = dr.cascaded_kernel_1d(1), dr.cascaded_kernel_1d(5)
    assert abs(k1.sum() - 1.) < 1e-15 and abs(k5.sum() - 1.) < 1e-15 and k5.shape == (125,)
    assert abs((k1 ** 2).sum() - 0.2734375) < 1e-15
    assert abs((k1 ** 2).sum() ** 2 - 0.0747681) < 5e-8
    assert abs((k5 ** 2).sum() - 0.0149869) < 5e-8
    assert abs((k5 ** 2).sum() ** 2 - 2.24609e-4) < 5e-10


def impulse_response(side):
    g0, g1 = dr.flat_guides(side, side)
    c = np.zeros((1, side, side, 3))
    c[0, side // 2, side // 2] = 1.
    out = dr.cascade(g0, g1, c, 5, P['sigma_n'], P['sigma_x'], np.inf)
    k = dr.cascaded_kernel_1d(5)
    want = np.zeros((side, side))
    want[side // 2 - 62:side // 2 + 63, side // 2 - 62:side // 2 + 63] = np.outer(k, k)
    return g0, g1, c, out, want


def test_impulse_response_is_the_cascaded_kernel():
    """flat, coplanar, all valid, sigma_c = inf: five levels turn a unit impulse into the outer product of the cascaded
    kernel, within 1e-14.

    On the 160 x 160 frame that holds as it stands on the rows and columns 32 .. 127.  The kernel reaches 62 pixels from the
    impulse, and a pixel further than 47 from it has level-4 taps (32 pixels away) outside the image: they are dropped and
    the rest renormalised, although every dropped tap would have read 0.  So there the definition gives the outer product
    divided by the B3 weight that stayed inside, per axis - also a closed form, and checked on every pixel.  A 192 x 192
    frame (62 + 32 <= 96) has no such pixel, and the plain statement holds on all of it."""
    g0, g1, c, out, want = impulse_response(160)
    assert np.abs(out[0, 32:128, 32:128] - want[32:128, 32:128, None]).max() < 1e-14
    at = np.arange(160)[:, None] + 16 * np.arange(-2, 3)[None, :]
    inside = (((at >= 0) & (at < 160)) * dr.H5).sum(1)
    assert inside.min() == 11. / 16. and (inside[32:128] == 1.).all()
    assert np.abs(out[0] - (want / np.outer(inside, inside))[..., None]).max() < 1e-14
    one = dr.level(g0, g1, c, 1, P['sigma_n'], P['sigma_x'], np.inf)
    assert np.abs(one[0, 78:83, 78:83, 0] - np.outer(dr.H5, dr.H5)).max() < 1e-16
    _, _, _, out, want = impulse_response(192)
    assert np.abs(out[0] - want[..., None]).max() < 1e-14


# ---- 2. basic properties ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    return dr.scene(40, 52, seed=1)


def run(g0, g1, c, levels=3, dtype=np.float64, **kw):
    p = dict(P, **kw)
    return dr.cascade(g0, g1, c, levels, p['sigma_n'], p['sigma_x'], p['sigma_c'], dtype)


def test_constant_signal_is_reproduced(small):
    g0, g1, _, noisy = small
    c = np.broadcast_to(np.array([0.7, 0.2, 1.9]), noisy.shape).copy()
    out = run(g0, g1, c)
    assert np.abs(out / c - 1.).max() < 1e-14


def test_filter_is_homogeneous(small):
    g0, g1, _, noisy = small
    a, b = run(g0, g1, noisy), run(g0, g1, 8. * noisy.astype(np.float64))
    assert np.abs(b / (8. * a) - 1.).max() < 1e-9


def test_invalid_pixels_are_passed_through_and_never_read(small):
    g0, g1, _, noisy = small
    valid = g0[..., 3] > 0.5
    assert (~valid).sum() >= 3 * 52 + 3 and valid.sum() > 0
    for dtype in (np.float64, np.float32):
        out = run(g0, g1, noisy, dtype=dtype)
        assert np.array_equal(out[:, ~valid], noisy[:, ~valid].astype(dtype))       # bitwise: the input's own values
        other = noisy.copy()
        other[:, ~valid] = 1e6 * (1. + np.arange((~valid).sum() * 3, dtype=np.float32).reshape(-1, 3))
        y0, x0 = np.argwhere(~valid)[-1]
        other[0, y0, x0, 1] = np.nan
        out2 = run(g0, g1, other, dtype=dtype)
        assert np.array_equal(out2[:, valid], out[:, valid])


def test_a_nan_pixel_is_skipped_and_filled_from_its_neighbours():
    H, W = 24, 31
    g0, g1 = dr.flat_guides(H, W)
    rng = np.random.Generator(np.random.Philox(5))
    c = rng.uniform(0.5, 1.5, size=(2, H, W, 3))
    c[1, 10, 12, 1] = np.nan                    # one channel of one signal: the pixel is skipped for both
    out = dr.level(g0, g1, c, 1, P['sigma_n'], P['sigma_x'], np.inf)
    assert np.isfinite(out).all()
    w = np.outer(dr.H5, dr.H5)
    w[2, 2] = 0.
    for s in range(2):
        want = (w[..., None] * c[s, 8:13, 10:15]).sum((0, 1)) / w.sum() if s == 0 else \
            np.nansum(w[..., None] * np.where(np.isfinite(c[1, 8:13, 10:15]), c[1, 8:13, 10:15], 0.), (0, 1)) / w.sum()
        assert np.abs(out[s, 10, 12] - want).max() < 1e-14
    # with the colour term on, the rest is still finite and the pixel still filled
    out = run(g0, g1, c, levels=5)
    assert np.isfinite(out).all()
    # a NaN that nothing can fill (its own weights sum to 0) stays: one pixel, no neighbour
    lone = dr.level(g0[:1, :1], g1[:1, :1], np.full((1, 1, 1, 3), np.nan), 1, 32., 0.1, 1.)
    assert np.isnan(lone).all()


# ---- 3. edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_perpendicular_normals_stop_the_filter(dtype):
    H, W = 48, 64
    g0, g1 = dr.flat_guides(H, W)
    g0[:, W // 2:, :3] = (1., 0., 0.)
    c = np.zeros((1, H, W, 3), np.float32)
    c[:, :, :W // 2] = 1.
    out = dr.cascade(g0, g1, c, 5, P['sigma_n'], P['sigma_x'], P['sigma_c'], dtype)
    assert np.array_equal(out, c.astype(dtype))


# ---- 4. noise ---------------------------------------------------------------------------------------------------------
def test_noise_on_the_synthetic_scene_is_at_least_halved():
    """96 x 96, the starting parameters: relative RMSE over the valid pixels against the clean signal, before and after.
    (Gamma(4, 1/4) noise has relative standard deviation 0.5.)"""
    g0, g1, clean, noisy = dr.scene(96, 96, seed=0)
    valid = g0[..., 3] > 0.5
    out = dr.cascade(g0, g1, noisy, P['levels'], P['sigma_n'], P['sigma_x'], P['sigma_c'])
    for s in range(2):
        before, after = dr.rel_rmse(noisy[s], clean[s], valid), dr.rel_rmse(out[s], clean[s], valid)
        print('signal %d: relative RMSE %.4f -> %.4f (ratio %.3f)' % (s, before, after, after / before))
        assert 0.4 < before < 0.6
        assert after <= 0.5 * before


# ---- 5. refusals ------------------------------------------------------------------------------------------------------
def test_entry_point_checks_its_arguments_on_the_host():
    from nefii_amd import _lib
    lib = _lib.lib()
    E_ARG, E_SHAPE = -1, -2
    f = lib.nefii_denoise_atrous
    a, b, c, d = 256, 512, 768, 1024                    # never dereferenced: every call below is refused on the host
    good = dict(n_signals=2, height=8, width=8, step=1, sigma_n=32., sigma_x=0.1, sigma_c=1.)

    def call(g0=a, g1=b, src=c, dst=d, **kw):
        k = dict(good, **kw)
        return f(g0, g1, src, dst, k['n_signals'], k['height'], k['width'], k['step'], k['sigma_n'], k['sigma_x'],
                 k['sigma_c'], None)
    for kw in (dict(g0=None), dict(g1=None), dict(src=None), dict(dst=None), dict(dst=c)):
        assert call(**kw) == E_ARG, kw
    for n in (0, 3, -1):
        assert call(n_signals=n) == E_ARG
    for side in (0, -5, 16385):
        assert call(height=side) == E_SHAPE and call(width=side) == E_SHAPE
    for step in (0, -1):
        assert call(step=step) == E_ARG
    for k in ('sigma_n', 'sigma_x', 'sigma_c'):
        assert call(**{k: -1.}) == E_ARG and call(**{k: float('nan')}) == E_ARG, k
    assert call(sigma_n=float('inf')) == E_ARG          # sigma_c = inf is legal (it runs: tests/test_gpu_denoise.py)


def test_op_rejects_cpu_tensors_and_bad_buffers():
    from nefii_amd import ops
    H, W = 4, 6
    g0, g1, src, dst = torch.zeros(H * W, 4), torch.zeros(H * W, 4), torch.zeros(2, H * W, 4), torch.zeros(2, H * W, 4)
    args = (H, W, 1, 32., 0.1, 1.)
    with pytest.raises(RuntimeError):                   # well-formed, but not on the GPU: no fallback
        ops.denoise_atrous(g0, g1, src, dst, *args)
    for bad in [(g0[:, :3], g1, src, dst), (g0, g1[:-1], src, dst), (g0, g1, src[:, :, :3], dst), (g0, g1, src, dst[:1]),
                (g0, g1, torch.zeros(3, H * W, 4), torch.zeros(3, H * W, 4)), (g0.double(), g1, src, dst),
                (g0, g1, src.half(), dst), (g0, g1, src, dst.double()),
                (torch.zeros(H * W, 8)[:, ::2], g1, src, dst), (g0, g1, torch.zeros(2, H * W, 8)[:, :, ::2], dst)]:
        with pytest.raises(ValueError):
            ops.denoise_atrous(*bad, *args)
    for bad_args in [(0, W, 1, 32., 0.1, 1.), (H, 16385, 1, 32., 0.1, 1.), (H, W, 0, 32., 0.1, 1.), (H, W, 1, -1., 0.1, 1.),
                     (H, W, 1, 32., float('nan'), 1.), (H, W, 1, 32., 0.1, -0.5), (H, W, 1, float('inf'), 0.1, 1.)]:
        with pytest.raises(ValueError):
            ops.denoise_atrous(g0, g1, src, dst, *bad_args)


def test_denoiser_wants_one_view():
    from nefii_amd import denoise
    with pytest.raises(ValueError):
        denoise.Denoiser(torch.zeros(2 * 12, 3), torch.zeros(2 * 12, 3), torch.ones(2 * 12, dtype=torch.bool), (3, 4))
    den = denoise.Denoiser(torch.zeros(12, 3), torch.zeros(12, 3), torch.ones(12, dtype=torch.bool), (3, 4))
    assert den.guides0.shape == (12, 4) and den.guides1.shape == (12, 4) and torch.isfinite(den.guides0).all()
    for bad in (torch.zeros(3, 3, 4, 3), torch.zeros(2, 3, 5, 3), torch.zeros(2, 3, 4, 4)):
        with pytest.raises(ValueError):
            den.filter(bad)
    for levels in (0, 9, 2.5):
        with pytest.raises(ValueError):
            den.filter(torch.zeros(2, 3, 4, 3), levels=levels)
    outs = {k: torch.zeros(24, 3) for k in ('sg_diffuse_rgb_values', 'sg_specular_rgb_values', 'sg_rgb_values',
                                            'sg_diffuse_albedo_values', 'normal_values', 'points')}
    outs['network_object_mask'] = torch.ones(24, dtype=torch.bool)
    with pytest.raises(ValueError):
        denoise.denoise_outputs(outs, (3, 4))


def _conf_file(tmp_path, render_type):
    p = tmp_path / ('%s.conf' % render_type)
    p.write_text('model {\n  render_type = %s\n}\n' % render_type)
    return str(p)


@pytest.mark.parametrize('script', ['render', 'vis_rotate_envlight'])
def test_command_lines_refuse_what_cannot_be_denoised(tmp_path, script):
    import importlib
    mod = importlib.import_module('nefii_amd.scripts.' + script)
    mc = _conf_file(tmp_path, 'pt_render_indirect_mlp')
    with pytest.raises(SystemExit) as e:                # closed-form frames carry no noise
        mod.main(['--conf', _conf_file(tmp_path, 'sg'), '--denoise'])
    assert 'Monte-Carlo' in str(e.value)
    for levels in ('0', '9'):
        with pytest.raises(SystemExit) as e:
            mod.main(['--conf', mc, '--denoise', '--denoise_levels', levels])
        assert 'levels' in str(e.value)
    with pytest.raises(SystemExit) as e:
        mod.main(['--conf', mc, '--denoise', '--denoise_sigma_color', '-1'])
    assert 'sigma_c' in str(e.value)


# ---- 6. the two scripts' command-line surface -----------------------------------------------------------------------
# What the parsers and the runner calls of both scripts gave before they shared add_render_args / runner_kwargs, recorded
# there with the checks and the runner stubbed out; 'conf' is the test's own file.
MINIMAL_OPT = {'checkpoint': 'latest', 'coordinate_type': 'mitsuba', 'data_split_dir': '', 'data_split_dir_test': '',
               'dataset_class': '', 'denoise': False, 'denoise_levels': 5, 'denoise_sigma_color': 1.0,
               'denoise_sigma_luminance': None, 'denoise_sigma_normal': 32.0, 'denoise_sigma_position': 0.1,
               'denoise_variance': False, 'envmap_height': None, 'envmap_indirect': 'mlp', 'envmap_scale': 1.0,
               'envmap_width': None, 'expname': '', 'exps_folder': 'exps', 'gamma': 1.0, 'is_continue': False, 'light_envmap': '',
               'light_sg': '', 'local_rank': -1, 'memory_capacity_level': 18,
               'model_class': 'nefii_amd.model.implicit_differentiable_renderer.IDRNetwork', 'num_rays': 256, 'old_expdir': '',
               'start_index': 0, 'subsample': 1, 'timestamp': 'latest', 'vis_subsample': 1}
FULL_LINE = ['--data_split_dir', 'a', '--data_split_dir_test', 'b', '--gamma', '2.2', '--subsample', '2', '--vis_subsample', '3',
             '--expname', 'robot', '--exps_folder', 'e', '--old_expdir', 'o', '--is_continue', '--timestamp', 't1',
             '--checkpoint', '100', '--memory_capacity_level', '12', '--coordinate_type', 'blender', '--light_sg', 'l.npy',
             '--light_envmap', 'sky.exr', '--envmap_height', '16', '--envmap_width', '32', '--envmap_scale', '0.5',
             '--envmap_indirect', 'bounce', '--start_index', '1', '--num_rays', '8', '--local_rank', '3', '--model_class', 'm.C',
             '--dataset_class', 'd.C']
FULL_OPT = dict(MINIMAL_OPT, **{
    'checkpoint': '100', 'coordinate_type': 'blender', 'data_split_dir': 'a', 'data_split_dir_test': 'b', 'dataset_class': 'd.C',
    'envmap_height': 16, 'envmap_indirect': 'bounce', 'envmap_scale': 0.5, 'envmap_width': 32, 'expname': 'robot',
    'exps_folder': 'e', 'gamma': 2.2, 'is_continue': True, 'light_envmap': 'sky.exr', 'light_sg': 'l.npy', 'local_rank': 3,
    'memory_capacity_level': 12, 'model_class': 'm.C', 'num_rays': 8, 'old_expdir': 'o', 'start_index': 1, 'subsample': 2,
    'timestamp': 't1', 'vis_subsample': 3})
MINIMAL_KWARGS = {'checkpoint': 'latest', 'coordinate_type': 'mitsuba', 'data_split_dir_test': '', 'dataset_class': None,
                  'denoise': False, 'denoise_levels': 5, 'denoise_sigma_color': 1.0, 'denoise_sigma_luminance': None,
                  'denoise_sigma_normal': 32.0, 'denoise_sigma_position': 0.1, 'denoise_variance': False, 'envmap_height': None,
                  'envmap_indirect': 'mlp', 'envmap_scale': 1.0, 'envmap_width': None, 'expname': 'default',
                  'exps_folder_name': 'exps', 'gamma': 1.0, 'light_envmap_path': '', 'light_sg_path': '',
                  'memory_capacity_level': 18, 'model_class': 'nefii_amd.model.implicit_differentiable_renderer.IDRNetwork',
                  'num_rays': 256, 'old_expdir': '', 'start_index': 0, 'subsample': 1, 'timestamp': 'latest', 'vis_subsample': 1}
FULL_KWARGS = dict(MINIMAL_KWARGS, **{
    'checkpoint': '100', 'coordinate_type': 'blender', 'data_split_dir_test': 'b', 'dataset_class': 'd.C', 'envmap_height': 16,
    'envmap_indirect': 'bounce', 'envmap_scale': 0.5, 'envmap_width': 32, 'expname': 'robot', 'exps_folder_name': 'e',
    'gamma': 2.2, 'light_envmap_path': 'sky.exr', 'light_sg_path': 'l.npy', 'memory_capacity_level': 12, 'model_class': 'm.C',
    'num_rays': 8, 'old_expdir': 'o', 'start_index': 1, 'subsample': 2, 'timestamp': 't1', 'vis_subsample': 3})
# what each script has of its own: (in vars(opt), in the runner's kwargs beside the shared ones) on the minimal line
OWN = {'render': ('RenderRunner', ('check_light_args', 'check_denoise_args'), {'trace_tier': None, 'bracket_staged_eval': None},
                  {'trace_tier': None, 'bracket_staged_eval': None, 'local_rank': -1}),
       'vis_rotate_envlight': ('TurntableRunner', ('check_turntable_args',), {'plots_dir': '', 'angle_delta': 15},
                               {'plots_dir': '', 'angle_delta': 15})}


@pytest.mark.parametrize('script', ['render', 'vis_rotate_envlight'])
def test_command_lines_parse_and_call_their_runner_as_before(tmp_path, script, monkeypatch):
    import importlib
    mod = importlib.import_module('nefii_amd.scripts.' + script)
    from nefii_amd.scripts.render import runner_kwargs
    runner, checks, own_opt, own_kwargs = OWN[script]
    conf = _conf_file(tmp_path, 'pt_render_indirect_mlp')
    seen = {}

    class Stub:
        def __init__(self, **kw):
            seen['kwargs'] = kw

        def run(self):
            return []
    monkeypatch.delenv('RANK', raising=False)
    monkeypatch.setattr(mod, runner, Stub)
    for c in checks:                                    # the full line is not one that could run: both lights at once
        monkeypatch.setattr(mod, c, lambda opt: seen.__setitem__('opt', opt))
    mod.main(['--conf', conf])
    assert vars(seen['opt']) == dict(MINIMAL_OPT, conf=conf, **own_opt)
    assert seen['kwargs'] == dict(MINIMAL_KWARGS, conf=conf, **own_kwargs)
    mod.main(['--conf', conf, '--data_split_dir', 'a'])                             # the test split falls back to the split
    assert vars(seen['opt']) == dict(MINIMAL_OPT, conf=conf, data_split_dir='a', **own_opt)
    assert seen['kwargs'] == dict(MINIMAL_KWARGS, conf=conf, data_split_dir_test='a', **own_kwargs)
    mod.main(['--conf', conf] + FULL_LINE + ['--not_an_option', '1'])               # parse_known_args: unknown ones are ignored
    assert vars(seen['opt']) == dict(FULL_OPT, conf=conf, **own_opt)
    assert seen['kwargs'] == dict(FULL_KWARGS, conf=conf, **dict(own_kwargs, **({'local_rank': 3} if script == 'render' else {})))
    assert runner_kwargs(seen['opt']) == dict(FULL_KWARGS, conf=conf)
