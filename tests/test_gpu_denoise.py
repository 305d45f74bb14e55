"""The guided a-trous denoiser on the GPU: nefii_denoise_atrous against the fp64 oracle (tests/denoise_ref.py)
on the kernel's own fp32 inputs, its bitwise guarantees, the frame-level step on a rendered crop of the bowl, and the two
command lines."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import denoise_ref as dr  # noqa: E402
import sg64  # noqa: E402

DEV = torch.device('cuda')
pytestmark = pytest.mark.gpu

P = dr.START


def pack(g0, g1, c):
    """the oracle's arrays -> the op's float4 buffers on the device"""
    S, H, W, _ = c.shape
    src = torch.zeros(S, H * W, 4)
    src[:, :, :3] = torch.from_numpy(np.ascontiguousarray(c, np.float32)).reshape(S, H * W, 3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).reshape(H * W, 4).to(DEV)
    return t(g0), t(g1), src.to(DEV)


def gpu_level(g0, g1, c, step, sigma_n, sigma_x, sigma_c_level):
    """one launch on numpy inputs -> [S, H, W, 3] float32 numpy"""
    from nefii_amd import ops
    S, H, W, _ = c.shape
    a, b, src = pack(g0, g1, c)
    dst = ops.denoise_atrous(a, b, src, torch.full_like(src, float('nan')), H, W, step, sigma_n, sigma_x, sigma_c_level)
    assert (dst[:, :, 3] == 0).all()                    # the fourth lane is carried through
    return dst[:, :, :3].reshape(S, H, W, 3).cpu().numpy()


def judge_level(J, name, g0, g1, c, step, sigma_c_level):
    got = gpu_level(g0, g1, c, step, P['sigma_n'], P['sigma_x'], sigma_c_level)
    r64 = dr.level(g0, g1, c, step, P['sigma_n'], P['sigma_x'], sigma_c_level, np.float64)
    r32 = dr.level(g0, g1, c, step, P['sigma_n'], P['sigma_x'], sigma_c_level, np.float32)
    for s in range(c.shape[0]):
        J.close('%s signal %d' % (name, s), torch.from_numpy(got[s]), torch.from_numpy(r64[s]), torch.from_numpy(r32[s]))
    return got


# ---- 1. against the fp64 oracle ---------------------------------------------------------------------------------------
# 1 x 1 and 3 x 5: fewer pixels than taps; 17 x 33: from level 2 on most taps fall outside; 67 x 130: several workgroups and
# no multiple of the 32 x 8 tile in either direction
@pytest.mark.parametrize('S', [1, 2])
@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (17, 33), (67, 130)], ids=lambda s: '%dx%d' % s)
def test_levels_and_cascade_match_the_oracle(shape, S):
    """every level l = 0 .. 4 (step 2^l, sigma_c 2^-l) on the input the kernel itself produced for it, and the five chained
    kernel levels against five chained fp64 levels; sg64's bound: min(5e-4, max(4 x fp32 oracle's error, 2e-6)) rel-L2"""
    g0, g1, _, noisy = dr.scene(*shape, seed=shape[0], n_signals=S)
    J = sg64.Judge('a-trous %d x %d, S = %d' % (shape + (S,)))
    c = noisy
    for l in range(P['levels']):
        c = judge_level(J, 'level %d' % l, g0, g1, c, 1 << l, P['sigma_c'] * 2. ** -l)
    J.require('finite', bool(np.isfinite(c).all()), '')
    r64 = dr.cascade(g0, g1, noisy, P['levels'], P['sigma_n'], P['sigma_x'], P['sigma_c'], np.float64)
    r32 = dr.cascade(g0, g1, noisy, P['levels'], P['sigma_n'], P['sigma_x'], P['sigma_c'], np.float32)
    for s in range(S):
        J.close('5 levels chained, signal %d' % s, torch.from_numpy(c[s]), torch.from_numpy(r64[s]), torch.from_numpy(r32[s]))
    J.done()


@pytest.mark.parametrize('S', [1, 2])
def test_single_steps_match_the_oracle(S):
    """67 x 130 at steps 1 .. 64, each on the noisy input; at step 64 only the centre column of taps is inside the image"""
    g0, g1, _, noisy = dr.scene(67, 130, seed=67, n_signals=S)
    J = sg64.Judge('a-trous 67 x 130 by step, S = %d' % S)
    for step in (1, 2, 4, 8, 16, 64):
        judge_level(J, 'step %d' % step, g0, g1, noisy, step, P['sigma_c'] / step)
    got = judge_level(J, 'step 1, sigma_c = inf', g0, g1, noisy, 1, float('inf'))
    J.require('finite', bool(np.isfinite(got).all()), '')
    J.done()


def test_denoiser_filter_is_the_chained_kernel():
    """nefii_amd.denoise.Denoiser packs the guides (renormalising the normals) and ping-pongs the levels: equal, bitwise, to
    the launches made by hand"""
    from nefii_amd.denoise import Denoiser
    H, W = 17, 33
    g0, g1, _, noisy = dr.scene(H, W, seed=17)
    t = lambda a: torch.from_numpy(a).to(DEV)
    den = Denoiser(3. * t(g0[..., :3]).reshape(-1, 3), t(g1[..., :3]).reshape(-1, 3), t(g0[..., 3] > 0.5).reshape(-1), (H, W))
    assert (den.guides0[:, :3] - t(g0[..., :3]).reshape(-1, 3)).abs().max() < 3e-7        # renormalised
    assert torch.equal(den.guides0[:, 3] > 0.5, den.valid) and torch.equal(den.guides1, t(g1).reshape(-1, 4))
    den = Denoiser(t(g0[..., :3]).reshape(-1, 3), t(g1[..., :3]).reshape(-1, 3), t(g0[..., 3] > 0.5).reshape(-1), (H, W))
    c2 = noisy
    for l in range(3):
        c2 = gpu_level(den.guides0.cpu().numpy().reshape(H, W, 4), g1, c2, 1 << l, 16., 0.2, 0.5 * 2. ** -l)
    out = den.filter(t(noisy).reshape(2, H * W, 3), levels=3, sigma_n=16., sigma_x=0.2, sigma_c=0.5)
    assert out.shape == (2, H, W, 3) and np.array_equal(out.cpu().numpy(), c2)


# ---- 2. bitwise -------------------------------------------------------------------------------------------------------
def test_bitwise_guarantees():
    g0, g1, _, noisy = dr.scene(67, 130, seed=3)
    valid = g0[..., 3] > 0.5
    assert 0 < (~valid).sum() < valid.size
    for step in (1, 4):
        args = (step, P['sigma_n'], P['sigma_x'], P['sigma_c'])
        a, b = gpu_level(g0, g1, noisy, *args), gpu_level(g0, g1, noisy, *args)
        assert np.array_equal(a, b)                                                 # two runs
        assert np.array_equal(a[:, ~valid], noisy[:, ~valid])                       # invalid pixels: their input
        assert not np.array_equal(a[:, valid], noisy[:, valid])
        for s in range(2):                                                          # no cross-talk between the signals
            assert np.array_equal(gpu_level(g0, g1, noisy[s:s + 1], *args)[0], a[s])
    # NaN and inf at invalid pixels are carried through and read by nobody
    other = noisy.copy()
    other[0, ~valid] = np.nan
    other[1, ~valid] = np.inf
    c = gpu_level(g0, g1, other, 1, P['sigma_n'], P['sigma_x'], P['sigma_c'])
    a = gpu_level(g0, g1, noisy, 1, P['sigma_n'], P['sigma_x'], P['sigma_c'])
    assert np.array_equal(c[:, valid], a[:, valid])
    assert np.isnan(c[0, ~valid]).all() and np.isinf(c[1, ~valid]).all()
    # a NaN at a valid pixel takes that tap out for both signals and is filled from its neighbours: the oracle's rule
    y0, x0 = np.argwhere(valid)[valid.sum() // 2]
    other = noisy.copy()
    other[1, y0, x0, 2] = np.nan
    J = sg64.Judge('a-trous with a NaN pixel')
    got = judge_level(J, 'NaN tap', g0, g1, other, 2, P['sigma_c'])
    J.require('finite', bool(np.isfinite(got[:, valid]).all()), '')
    J.done()


def test_plain_level_neither_reads_nor_alters_the_fourth_lane():
    """nefii_denoise_atrous looks at r, g, b only: whatever lane w of `in` holds - NaN and both infinities included, at valid
    and at invalid pixels - the colour lanes come out the same bits as with zeros there, and lane w comes out as it went in"""
    from nefii_amd import ops
    H, W = 17, 33
    g0, g1, _, noisy = dr.scene(H, W, seed=17)
    valid = (g0[..., 3] > 0.5).reshape(-1)
    a, b, zeros = pack(g0, g1, noisy)
    w = np.random.Generator(np.random.Philox(17)).standard_normal((2, H * W)).astype(np.float32)
    on, off = np.flatnonzero(valid), np.flatnonzero(~valid)
    assert len(on) >= 6 and len(off) >= 1
    picks = on[np.linspace(0, len(on) - 1, 6).astype(int)]
    w[0, picks[0]] = w[1, picks[1]] = w[0, off[0]] = np.nan
    w[0, picks[2]] = w[1, picks[3]] = np.inf
    w[0, picks[4]] = w[1, picks[5]] = w[1, off[0]] = -np.inf
    filled = zeros.clone()
    filled[:, :, 3] = torch.from_numpy(w).to(DEV)
    for step in (1, 4):
        run = lambda src: ops.denoise_atrous(a, b, src, torch.full_like(src, float('nan')), H, W, step, P['sigma_n'], P['sigma_x'],
                                             P['sigma_c']).cpu().numpy()
        plain, other = run(zeros), run(filled)
        assert np.isfinite(plain[:, valid, :3]).all() and not np.array_equal(plain[:, valid, :3], noisy.reshape(2, -1, 3)[:, valid])
        assert np.array_equal(other[:, :, :3], plain[:, :, :3])
        assert np.array_equal(other[:, :, 3], w, equal_nan=True)
        assert np.array_equal(other[:, :, 3].view(np.uint32), w.view(np.uint32))            # bit for bit, NaN payloads too


@pytest.mark.parametrize('symbol', ['nefii_denoise_atrous', 'nefii_denoise_atrous_variance'])
def test_level_entry_points_refuse_the_same_calls(symbol):
    """the two level entry points, called past the Python checks on real buffers: the same malformed calls get the same codes
    and leave `out` as it was, and an infinite third sigma runs"""
    from nefii_amd import _lib
    f = getattr(_lib.lib(), symbol)
    E_ARG, E_SHAPE = -1, -2
    H, W = 3, 5
    g0, g1, _, noisy = dr.scene(H, W, seed=3)
    a, b, src = pack(g0, g1, noisy)
    dst = torch.full_like(src, float('nan'))
    good = dict(dst=dst.data_ptr(), n_signals=2, height=H, width=W, step=1, sigma_n=32., sigma_x=0.1, sigma_3=1.)

    def call(**kw):
        k = dict(good, **kw)
        return f(a.data_ptr(), b.data_ptr(), src.data_ptr(), k['dst'], k['n_signals'], k['height'], k['width'], k['step'],
                 k['sigma_n'], k['sigma_x'], k['sigma_3'], None)
    inf, nan = float('inf'), float('nan')
    for kw in (dict(dst=src.data_ptr()), dict(n_signals=0), dict(n_signals=3), dict(step=0), dict(sigma_n=-1.), dict(sigma_x=-1.),
               dict(sigma_3=-1.), dict(sigma_n=nan), dict(sigma_x=nan), dict(sigma_3=nan), dict(sigma_n=inf)):
        assert call(**kw) == E_ARG, kw
    assert call(height=0) == E_SHAPE and call(width=16385) == E_SHAPE
    torch.cuda.synchronize()
    assert torch.isnan(dst).all()                       # nothing was launched
    assert call(sigma_3=inf) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(dst).all()


# ---- 3. the renderer --------------------------------------------------------------------------------------------------
def bowl_model():
    """tests/test_gpu_bounce.py's model: the fitted bowl, frozen, in evaluation mode"""
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    mc = syn.model_conf('conf')
    sd = syn.make_state_dict(mc, seed=0, scene='bowl_trained')
    model = IDRNetwork(conf.from_dict(mc))
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    model.freeze_geometry()
    model.eval()
    return model


def crop_input(rays=64, size=32, res=64, seed=0):
    """tests/test_gpu_bounce.py's crop - a size x size crop of a res x res view, `rays` jittered rays per pixel - handed over
    per pixel ([1, pixels, rays, 2]), so that the model averages the rays of a pixel as the frame loop's datasets have it"""
    from nefii_amd import synthetic as syn
    g = np.random.Generator(np.random.Philox(seed))
    y, x = np.meshgrid(np.arange(size) + (res - size) // 2, np.arange(size) + (res - size) // 2, indexing='ij')
    uv = np.stack([x, y], -1).reshape(-1, 1, 2) + g.uniform(-0.5, 0.5, size=(size * size, rays, 2))
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 70.
    K[0, 2] = K[1, 2] = res / 2.
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    return {'uv': f(uv.reshape(1, size * size, rays, 2)).to(DEV), 'intrinsics': f(K)[None].to(DEV),
            'pose': f(syn.look_at_origin_pose((0.6, 1.0, 2.2)))[None].to(DEV),
            'object_mask': torch.ones(1, size * size, dtype=torch.bool, device=DEV)}


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_denoised_few_ray_frame_is_closer_to_the_many_ray_frame():
    from nefii_amd.denoise import denoise_outputs
    model = bowl_model()
    size = 32
    frames = {}
    for rays, seed in ((4, 1), (256, 2)):
        torch.manual_seed(seed)
        with torch.no_grad():
            frames[rays] = model(crop_input(rays=rays, size=size, seed=seed))
    few, many = frames[4], frames[256]
    valid = few['network_object_mask'] & many['network_object_mask']
    share = valid.float().mean().item()
    assert few['sg_rgb_values'].shape == (size * size, 3) and share >= 0.25, share          # the precondition
    out = denoise_outputs(few, (size, size), **P)
    raw, den = rel_l2(few['sg_rgb_values'][valid], many['sg_rgb_values'][valid]), \
        rel_l2(out['sg_rgb_values'][valid], many['sg_rgb_values'][valid])
    print('bowl crop %d x %d, valid share %.3f: rel-L2 against 256 rays: 4 rays raw %.4f, denoised %.4f (ratio %.3f)'
          % (size, size, share, raw, den, den / raw))
    for k in ('sg_diffuse_rgb_values', 'sg_specular_rgb_values'):
        print('  %s: raw %.4f, denoised %.4f' % (k, rel_l2(few[k][valid], many[k][valid]), rel_l2(out[k][valid], many[k][valid])))
    assert den < raw
    own = few['network_object_mask']
    assert (~own).any() and torch.isfinite(out['sg_rgb_values']).all()
    for k in ('sg_rgb_values', 'sg_diffuse_rgb_values', 'sg_specular_rgb_values'):
        assert out[k] is not few[k] and torch.equal(out[k][~own], few[k][~own])             # bitwise
        assert not torch.equal(out[k][own], few[k][own])
    s = out['sg_diffuse_rgb_values'] + out['sg_specular_rgb_values']
    assert ((out['sg_rgb_values'] - s)[own].abs() <= 2. ** -23 * s[own].abs()).all()
    assert set(out) == set(few)
    for k in few:
        if k not in ('sg_rgb_values', 'sg_diffuse_rgb_values', 'sg_specular_rgb_values'):
            assert out[k] is few[k], k
    with pytest.raises(ValueError):                     # one view per call
        denoise_outputs(few, (size, size // 2), **P)


# ---- 4. the command lines ---------------------------------------------------------------------------------------------
def experiment(tmp_path):
    """tests/test_gpu_bounce.py's experiment on the 16 x 16 synthetic dataset, under the model's own light"""
    from nefii_amd import conf, synthetic as syn
    mc = syn.model_conf('conf', hidden=64)
    cfg = conf.from_dict({'train': {'model_class': 'nefii_amd.model.implicit_differentiable_renderer.IDRNetwork',
                                    'dataset_class': 'nefii_amd.datasets.synthetic_dataset.SyntheticSceneDataset'},
                          'model': mc})
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    ck = tmp_path / 'scene' / 't0' / 'checkpoints' / 'ModelParameters'
    os.makedirs(str(ck))
    torch.save({'epoch': 1, 'model_state_dict': sd}, str(ck / 'latest.pth'))
    return dict(conf=cfg, exps_folder_name=str(tmp_path), expname='scene', timestamp='t0', checkpoint='latest',
                memory_capacity_level=10, num_rays=2, dataset_kwargs={'n_views': 2, 'img_res': (16, 16)})


@pytest.fixture
def counted(monkeypatch):
    """counts the Denoiser constructions and the launches"""
    from nefii_amd import denoise, ops
    n = {'denoisers': 0, 'launches': 0}

    class Counting(denoise.Denoiser):
        def __init__(self, *a, **kw):
            n['denoisers'] += 1
            super().__init__(*a, **kw)
    real = ops.denoise_atrous

    def launch(*a, **kw):
        n['launches'] += 1
        return real(*a, **kw)
    monkeypatch.setattr(denoise, 'Denoiser', Counting)
    monkeypatch.setattr(ops, 'denoise_atrous', launch)
    return n


def refuse(*a, **kw):
    raise AssertionError('the default path must not touch the denoiser')


def test_render_cli_with_and_without_denoise(tmp_path, counted, monkeypatch):
    from nefii_amd import ops
    from nefii_amd.scripts.render import RenderRunner
    from nefii_amd.utils import exr
    kw = experiment(tmp_path)
    runner = RenderRunner(new_timestamp='den', denoise=True, denoise_levels=3, **kw)
    assert runner.denoise and runner.denoise_params == dict(P, levels=3)
    torch.manual_seed(0)                                            # the pixel jitter and the uniforms: the same in both runs
    assert runner.run() == [0, 1]
    assert counted == {'denoisers': 2, 'launches': 6}               # per frame: one set of guides, one launch per level
    monkeypatch.setattr(ops, 'denoise_atrous', refuse)
    plain = RenderRunner(new_timestamp='plain', **kw)
    assert not plain.denoise
    torch.manual_seed(0)
    assert plain.run() == [0, 1]
    den, raw = [str(tmp_path / 'scene' / t / 'plots') for t in ('den', 'plain')]
    assert sorted(os.listdir(den)) == sorted(os.listdir(raw)) and os.listdir(den)
    changed = False
    for f in os.listdir(den):
        if f.startswith('rerender_rgb'):
            x, y = exr.imread(os.path.join(den, f)), exr.imread(os.path.join(raw, f))
            assert np.isfinite(x).all() and (x >= 0).all(), f
            changed = changed or not np.array_equal(x, y)
        if f.startswith('diffuse_albedo'):
            assert np.array_equal(exr.imread(os.path.join(den, f)), exr.imread(os.path.join(raw, f)))
    assert changed
    for bad in (dict(denoise_levels=0), dict(denoise_levels=9), dict(denoise_sigma_color=-1.)):
        with pytest.raises(ValueError):
            RenderRunner(new_timestamp='bad', denoise=True, **dict(kw, **bad))


def test_turntable_cli_with_and_without_denoise(tmp_path, counted, monkeypatch):
    from PIL import Image
    from nefii_amd import ops
    from nefii_amd.scripts.vis_rotate_envlight import TurntableRunner
    kw = dict(experiment(tmp_path), angle_delta=180, env_height=8, env_width=16)
    torch.manual_seed(0)
    assert TurntableRunner(plots_dir=str(tmp_path / 'den'), new_timestamp='den', denoise=True, **kw).run() == [0, 1]
    # two views, two angles each: the guides are packed once per view and shared by its angles
    assert counted == {'denoisers': 2, 'launches': 2 * 2 * P['levels']}
    monkeypatch.setattr(ops, 'denoise_atrous', refuse)
    torch.manual_seed(0)
    assert TurntableRunner(plots_dir=str(tmp_path / 'plain'), new_timestamp='plain', **kw).run() == [0, 1]
    den, raw = sorted(os.listdir(str(tmp_path / 'den'))), sorted(os.listdir(str(tmp_path / 'plain')))
    assert den == raw and len(den) == 2 * (2 * 3 + 1)
    png = lambda d, f: np.asarray(Image.open(str(tmp_path / d / f)))
    assert any(not np.array_equal(png('den', f), png('plain', f)) for f in den if '-render-' in f)
    for f in den:
        if '-env-' in f or '-gt_rgb-' in f:
            assert np.array_equal(png('den', f), png('plain', f)), f
        if '-material-' in f:                           # normal | albedo are not filtered
            assert np.array_equal(png('den', f)[:, :32], png('plain', f)[:, :32]), f
