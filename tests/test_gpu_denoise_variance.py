"""The variance-guided denoiser on the GPU: nefii_pixel_moments and nefii_denoise_atrous_variance against the fp64
oracle (tests/denoise_var_ref.py) on the kernels' own fp32 inputs, their bitwise guarantees, Denoiser.filter_variance, the
renderer's denoise_signals on a crop of the bowl, and the two command lines."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import denoise_ref as dr  # noqa: E402
import denoise_var_ref as vr  # noqa: E402
import sg64  # noqa: E402

DEV = torch.device('cuda')
pytestmark = pytest.mark.gpu

P = vr.START
ULP = 2. ** -23


# ---- 1. the moments ---------------------------------------------------------------------------------------------------
def ray_buffers(n_pix, R, seed, level=1., spread=None):
    """per-ray diffuse, albedo, specular [n_pix R, 3] float32 and hit [n_pix R]: Gamma(4) noise around `level`, or - spread
    given - relative noise `spread` around it (cancellation in a one-pass formula).  Where the frame has room for them: the
    last pixel has equal samples, the one before a missed ray, pixel 0 an albedo under the floor, pixel 1 a NaN sample."""
    rng = np.random.Generator(np.random.Philox(seed))
    noise = (lambda: rng.gamma(4., 0.25, size=(n_pix, R, 3))) if spread is None else \
        (lambda: 1. + spread * rng.standard_normal(size=(n_pix, R, 3)))
    d, s = (level * rng.uniform(0.5, 1.5, size=(n_pix, 1, 3)) * noise() for _ in range(2))
    a = rng.uniform(0.1, 0.9, size=(n_pix, 1, 3)) * (1. + 0.1 * rng.uniform(-1., 1., size=(n_pix, R, 3)))
    hit = np.ones((n_pix, R), bool)
    special = {}
    if n_pix >= 3:
        d[-1], a[-1], s[-1] = d[-1, :1], a[-1, :1], s[-1, :1]
        hit[-2, R // 2] = False
        special.update(equal=n_pix - 1, missed=n_pix - 2)
    if n_pix >= 5:
        a[0, :, 1] = 2e-4
        d[1, R - 1, 2] = np.nan
        special.update(floor=0, nan=1)
    f = lambda x: np.ascontiguousarray(x.reshape(n_pix * R, -1), np.float32)
    return f(d), f(a), f(s), hit.reshape(-1), special


def gpu_moments(d, a, s, hit, R):
    from nefii_amd import ops
    t = lambda x: torch.from_numpy(x).to(DEV)
    return ops.pixel_moments(t(d), t(a), t(s), t(hit), R).cpu().numpy()


@pytest.mark.parametrize('case', [(1, 2, 1., None), (5, 3, 1., None), (67, 64, 1., None), (33, 65, 1., None), (3, 4096, 1., None),
                                  (67, 64, 1e4, 1e-3)], ids=lambda c: '%dx%d@%g' % c[:3])
def test_pixel_moments_match_the_oracle(case):
    """every finite element within 2^-23 max(|ref|, 1e-30) of the fp64 reference: one fp32 rounding of an fp64 result, doubled
    for the order of the fp64 sums; (33, 65) is one ray past a wave, (3, 4096) the largest R, 67 pixels end inside a workgroup"""
    n_pix, R, level, spread = case
    d, a, s, hit, special = ray_buffers(n_pix, R, seed=R, level=level, spread=spread)
    got = gpu_moments(d, a, s, hit, R)
    ref = vr.moments(d, a, s, hit, R)
    assert got.shape == (2, n_pix, 4) and got.dtype == np.float32
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    err = np.abs(got.astype(np.float64) - ref)[fin] / np.maximum(np.abs(ref[fin]), 1e-30)
    rel_v = err.reshape(-1)[(np.nonzero(fin.reshape(-1))[0] % 4) == 3]
    print('moments %d x %d, level %g: largest error %.3f x 2^-23 of the reference (variance lanes %.3f)'
          % (n_pix, R, level, err.max() / ULP, rel_v.max() / ULP))
    assert (np.abs(got.astype(np.float64) - ref)[fin] <= ULP * np.maximum(np.abs(ref[fin]), 1e-30)).all()
    if 'equal' in special:
        assert (got[:, special['equal'], 3] == 0.).all() and np.isfinite(got[:, special['equal']]).all()
        assert (got[:, special['missed']] == 0.).all()                          # exactly zero, all four lanes, both signals
    if 'nan' in special:
        assert not np.isfinite(got[0, special['nan'], 2]) and not np.isfinite(got[0, special['nan'], 3])
        assert np.isfinite(got[1, special['nan']]).all()
        assert np.isfinite(got[:, special['floor']]).all() and got[0, special['floor'], 1] > 100.
    assert (got[..., 3][np.isfinite(got[..., 3])] >= 0).all()
    assert np.array_equal(gpu_moments(d, a, s, hit, R), got, equal_nan=True)     # two runs, the same bits


# ---- 2. the level against the oracle ----------------------------------------------------------------------------------
def pack(g0, g1, c4):
    S, H, W, _ = c4.shape
    t = lambda x, *shape: torch.from_numpy(np.ascontiguousarray(x, np.float32)).reshape(*shape).to(DEV)
    return t(g0, H * W, 4), t(g1, H * W, 4), t(c4, S, H * W, 4)


def gpu_level(g0, g1, c4, step, sigma_n, sigma_x, sigma_l):
    """one launch on numpy inputs -> [S, H, W, 4] float32 numpy"""
    from nefii_amd import ops
    S, H, W, _ = c4.shape
    a, b, src = pack(g0, g1, c4)
    dst = ops.denoise_atrous_variance(a, b, src, torch.full_like(src, float('nan')), H, W, step, sigma_n, sigma_x, sigma_l)
    return dst.reshape(S, H, W, 4).cpu().numpy()


def judge(J, name, got, r64, r32):
    for s in range(got.shape[0]):
        J.close('%s signal %d colour' % (name, s), torch.from_numpy(got[s, ..., :3]), torch.from_numpy(r64[s, ..., :3]),
                torch.from_numpy(r32[s, ..., :3]))
        J.close('%s signal %d variance' % (name, s), torch.from_numpy(got[s, ..., 3]), torch.from_numpy(r64[s, ..., 3]),
                torch.from_numpy(r32[s, ..., 3]))


def judge_level(J, name, g0, g1, c4, step, sigma_l):
    got = gpu_level(g0, g1, c4, step, P['sigma_n'], P['sigma_x'], sigma_l)
    judge(J, name, got, vr.level_var(g0, g1, c4, step, P['sigma_n'], P['sigma_x'], sigma_l, np.float64),
          vr.level_var(g0, g1, c4, step, P['sigma_n'], P['sigma_x'], sigma_l, np.float32))
    return got


def scene4(H, W, S, seed):
    g0, g1, _, s4 = vr.shadow_scene(H, W, 4, seed)
    return g0, g1, s4[:S]


@pytest.mark.parametrize('S', [1, 2])
@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (17, 33), (67, 130)], ids=lambda s: '%dx%d' % s)
def test_levels_and_cascade_match_the_oracle(shape, S):
    """every level l = 0 .. 4 (step 2^l, the same sigma_l) on the input the kernel itself produced for it, and the five chained
    kernel levels against five chained fp64 levels; colour and the variance lane each under sg64's bound: min(5e-4, max(4 x
    fp32 oracle's error, 2e-6)) rel-L2"""
    g0, g1, s4 = scene4(*shape, S, seed=shape[0])
    J = sg64.Judge('variance-guided a-trous %d x %d, S = %d' % (shape + (S,)))
    c = s4
    for l in range(P['levels']):
        c = judge_level(J, 'level %d' % l, g0, g1, c, 1 << l, P['sigma_l'])
    J.require('finite', bool(np.isfinite(c).all()), '')
    judge(J, '5 levels chained,', c, vr.cascade_var(g0, g1, s4, dtype=np.float64, **P),
          vr.cascade_var(g0, g1, s4, dtype=np.float32, **P))
    J.done()


@pytest.mark.parametrize('S', [1, 2])
def test_single_steps_match_the_oracle(S):
    """67 x 130 at steps 1 .. 64, each on the noisy input; at step 64 only the centre column of taps is inside the image"""
    g0, g1, s4 = scene4(67, 130, S, seed=67)
    J = sg64.Judge('variance-guided a-trous 67 x 130 by step, S = %d' % S)
    for step in (1, 2, 4, 8, 16, 64):
        judge_level(J, 'step %d' % step, g0, g1, s4, step, P['sigma_l'])
    got = judge_level(J, 'step 1, sigma_l = inf', g0, g1, s4, 1, float('inf'))
    judge_level(J, 'step 4, sigma_l = 0.5', g0, g1, s4, 4, 0.5)
    J.require('finite', bool(np.isfinite(got).all()), '')
    J.done()


# ---- 3. bitwise -------------------------------------------------------------------------------------------------------
def test_bitwise_guarantees():
    g0, g1, s4 = scene4(67, 130, 2, seed=3)
    valid = g0[..., 3] > 0.5
    assert 0 < (~valid).sum() < valid.size
    for step in (1, 4):
        args = (step, P['sigma_n'], P['sigma_x'], P['sigma_l'])
        a, b = gpu_level(g0, g1, s4, *args), gpu_level(g0, g1, s4, *args)
        assert np.array_equal(a, b)                                                 # two runs
        assert np.array_equal(a[:, ~valid], s4[:, ~valid])                          # invalid pixels: their four lanes
        assert not np.array_equal(a[:, valid][..., :3], s4[:, valid][..., :3])
        assert (a[:, valid][..., 3] < s4[:, valid][..., 3]).any()
        for s in range(2):                                                          # no cross-talk between the signals
            assert np.array_equal(gpu_level(g0, g1, s4[s:s + 1], *args)[0], a[s])
    # NaN and inf at invalid pixels are carried through and read by nobody
    other = s4.copy()
    other[0, ~valid] = np.nan
    other[1, ~valid] = np.inf
    other[1, ~valid, 3] = -np.inf
    c = gpu_level(g0, g1, other, 1, P['sigma_n'], P['sigma_x'], P['sigma_l'])
    a = gpu_level(g0, g1, s4, 1, P['sigma_n'], P['sigma_x'], P['sigma_l'])
    assert np.array_equal(c[:, valid], a[:, valid])
    assert np.isnan(c[0, ~valid]).all() and np.isinf(c[1, ~valid]).all()
    # a NaN at a valid pixel - in a colour lane, and in the variance lane alone - takes that tap out for both signals and is
    # filled from its neighbours: the oracle's rule
    y0, x0 = np.argwhere(valid)[valid.sum() // 2]
    y1, x1 = np.argwhere(valid)[valid.sum() // 3]
    other = s4.copy()
    other[1, y0, x0, 2] = np.nan
    other[0, y1, x1, 3] = np.inf
    J = sg64.Judge('variance-guided a-trous with non-finite pixels')
    for step in (1, 2):
        got = judge_level(J, 'NaN taps, step %d' % step, g0, g1, other, step, P['sigma_l'])
        J.require('finite', bool(np.isfinite(got[:, valid]).all()), '')
    J.done()


# ---- 4. Denoiser.filter_variance --------------------------------------------------------------------------------------
def test_filter_variance_is_the_chained_kernel():
    from nefii_amd.denoise import Denoiser
    H, W = 17, 33
    g0, g1, s4 = scene4(H, W, 2, seed=17)
    t = lambda a: torch.from_numpy(a).to(DEV)
    den = Denoiser(t(g0[..., :3]).reshape(-1, 3), t(g1[..., :3]).reshape(-1, 3), t(g0[..., 3] > 0.5).reshape(-1), (H, W))
    c = s4
    for l in range(3):
        c = gpu_level(den.guides0.cpu().numpy().reshape(H, W, 4), g1, c, 1 << l, 16., 0.2, 2.5)
    given = t(s4).reshape(2, H * W, 4)
    kept = given.clone()
    interleaved = given.transpose(0, 1).contiguous().transpose(0, 1)                # denoise_outputs' view of [H*W, 8]
    assert not interleaved.is_contiguous()
    for signals in (given, given.reshape(2, H, W, 4), interleaved):
        out = den.filter_variance(signals, levels=3, sigma_n=16., sigma_x=0.2, sigma_l=2.5)
        assert out.shape == (2, H, W, 4) and np.array_equal(out.cpu().numpy(), c)
    assert torch.equal(given, kept)                                                 # the caller's tensor is not a ping-pong buffer


# ---- 5. the renderer --------------------------------------------------------------------------------------------------
def bowl_model():
    """tests/test_gpu_denoise.py's model: the fitted bowl, frozen, in evaluation mode"""
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
    """tests/test_gpu_denoise.py's crop - a size x size crop of a res x res view, `rays` jittered rays per pixel - handed over
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


def test_renderer_signals_and_the_denoised_few_ray_frame(monkeypatch):
    """Bowl crop 32 x 32, 8 rays (seed 1) against 256 (seed 2).  Measured on one MI355X, rel-L2 of sg_rgb against the 256-ray
    crop: raw 0.2703, 6j 0.1585, variance-guided 0.1661 (asserted: below raw; 6j's figure is printed beside it, not asserted)."""
    from nefii_amd import ops
    from nefii_amd.denoise import DEFAULTS, denoise_outputs
    model = bowl_model()
    size, R = 32, 8
    torch.manual_seed(2)
    with torch.no_grad():
        many = model(crop_input(rays=256, size=size, seed=2))
    assert 'denoise_signals' not in many
    seen = {}
    real = ops.pixel_moments

    def hook(diffuse, albedo, specular, hit, rays):                                 # the per-ray buffers of this very forward
        seen['args'] = [x.cpu().numpy() for x in (diffuse, albedo, specular, hit)] + [rays]
        return real(diffuse, albedo, specular, hit, rays)
    monkeypatch.setattr(ops, 'pixel_moments', hook)
    model.pixel_moments = True
    torch.manual_seed(1)
    with torch.no_grad():
        few = model(crop_input(rays=R, size=size, seed=1))
    model.pixel_moments = False
    assert set(few) == set(many) | {'denoise_signals'} and few['denoise_signals'].shape == (size * size, 8)
    own = few['network_object_mask']
    valid = own & many['network_object_mask']
    share = valid.float().mean().item()
    assert few['sg_rgb_values'].shape == (size * size, 3) and share >= 0.25, share            # the precondition
    assert seen['args'][4] == R and seen['args'][0].shape == (size * size * R, 3)
    # the variance lanes, and the colour lanes, are the oracle's on the per-ray buffers
    sig = few['denoise_signals'].cpu().numpy().astype(np.float64).reshape(size * size, 2, 4).transpose(1, 0, 2)
    ref = vr.moments(*seen['args'])
    assert np.isfinite(ref).all() and (np.abs(sig - ref) <= ULP * np.maximum(np.abs(ref), 1e-30)).all()
    assert np.array_equal(ref[0].any(-1), own.cpu().numpy()) and (ref[0, own.cpu().numpy(), 3] > 0).mean() > 0.9
    # colour lanes x albedo against the renderer's own means: torch's fp32 mean of 8 rays against the fp64 mean, two
    # roundings and a product - 4 fp32 ulps at the scale of the buffer's largest value
    albedo = few['sg_diffuse_albedo_values']
    s = few['denoise_signals']
    above = own & (albedo.min(dim=1).values >= 1e-3)
    assert above.float().mean().item() >= 0.25
    for name, mine, theirs in (('diffuse', albedo * s[:, 0:3], few['sg_diffuse_rgb_values']),
                               ('specular', s[:, 4:7], few['sg_specular_rgb_values'])):
        scale = theirs[above].abs().max().item()
        worst = (mine - theirs)[above].abs().max().item()
        print('  %s: colour lanes x albedo against the rendered mean: largest difference %.2f ulps at scale %.3g'
              % (name, worst / (ULP * scale), scale))
        assert worst <= 4 * ULP * scale
    # the frame-level step
    out = denoise_outputs(few, (size, size), variance=True, **P)
    old = denoise_outputs({k: v for k, v in few.items() if k != 'denoise_signals'}, (size, size), **DEFAULTS)
    e = {k: (rel_l2(few[k][valid], many[k][valid]), rel_l2(old[k][valid], many[k][valid]), rel_l2(out[k][valid], many[k][valid]))
         for k in ('sg_rgb_values', 'sg_diffuse_rgb_values', 'sg_specular_rgb_values')}
    print('bowl crop %d x %d, valid share %.3f, rel-L2 against 256 rays, %d rays raw / 6j / variance-guided:' % (size, size, share, R))
    for k, v in e.items():
        print('  %s: %.4f / %.4f / %.4f' % ((k,) + v))
    raw, _, den = e['sg_rgb_values']
    assert den < raw
    assert (~own).any() and torch.isfinite(out['sg_rgb_values']).all()
    for k in ('sg_rgb_values', 'sg_diffuse_rgb_values', 'sg_specular_rgb_values'):
        assert out[k] is not few[k] and torch.equal(out[k][~own], few[k][~own])             # bitwise
        assert not torch.equal(out[k][own], few[k][own])
    t = out['sg_diffuse_rgb_values'] + out['sg_specular_rgb_values']
    assert ((out['sg_rgb_values'] - t)[own].abs() <= 2. ** -23 * t[own].abs()).all()
    assert set(out) == set(few) | {'denoise_variance'}
    for k in few:
        if k not in ('sg_rgb_values', 'sg_diffuse_rgb_values', 'sg_specular_rgb_values'):
            assert out[k] is few[k], k
    left = out['denoise_variance']
    assert left.shape == (size * size, 2) and torch.isfinite(left).all() and (left >= 0).all()
    given = torch.stack([s[:, 3], s[:, 7]], 1)                                      # sum w^2 v / (sum w)^2 <= the largest tap's v
    assert (left[own].max(dim=0).values <= given[own].max(dim=0).values * (1. + 1e-5)).all()
    assert (left[own].mean(dim=0) < given[own].mean(dim=0)).all()
    with pytest.raises(ValueError):                     # one view per call
        denoise_outputs(few, (size, size // 2), variance=True, **P)


# ---- 6. the command lines ---------------------------------------------------------------------------------------------
def experiment(tmp_path):
    """tests/test_gpu_denoise.py's experiment on the 16 x 16 synthetic dataset, under the model's own light"""
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
                memory_capacity_level=10, num_rays=8, dataset_kwargs={'n_views': 2, 'img_res': (16, 16)})


CHUNKS = math.ceil(16 * 16 / (2 ** 10 // 8))            # of a frame: 2^memory_capacity_level // num_rays pixels each


@pytest.fixture
def counted(monkeypatch):
    """counts the Denoiser constructions and the launches of the three ops"""
    from nefii_amd import denoise, ops
    n = {'denoisers': 0, 'launches': 0, 'variance_launches': 0, 'moments': 0}

    class Counting(denoise.Denoiser):
        def __init__(self, *a, **kw):
            n['denoisers'] += 1
            super().__init__(*a, **kw)

    def counting(name, key):
        real = getattr(ops, name)

        def launch(*a, **kw):
            n[key] += 1
            return real(*a, **kw)
        monkeypatch.setattr(ops, name, launch)
    monkeypatch.setattr(denoise, 'Denoiser', Counting)
    counting('denoise_atrous', 'launches')
    counting('denoise_atrous_variance', 'variance_launches')
    counting('pixel_moments', 'moments')
    return n


def refuse(*a, **kw):
    raise AssertionError('without --denoise_variance nothing of it is called')


def test_render_cli_with_denoise_variance(tmp_path, counted, monkeypatch):
    from nefii_amd import ops
    from nefii_amd.scripts.render import RenderRunner
    from nefii_amd.utils import exr
    kw = experiment(tmp_path)
    assert CHUNKS == 2
    runner = RenderRunner(new_timestamp='var', denoise=True, denoise_variance=True, denoise_levels=3, **kw)
    assert runner.denoise_variance and runner.denoise_params == dict(P, levels=3) and runner.model.pixel_moments
    torch.manual_seed(0)
    assert runner.run() == [0, 1]
    # per frame: one set of guides, one launch of the new filter per level, none of the old one, one moments launch per chunk
    assert counted == {'denoisers': 2, 'launches': 0, 'variance_launches': 6, 'moments': 2 * CHUNKS}
    monkeypatch.setattr(ops, 'denoise_atrous_variance', refuse)
    monkeypatch.setattr(ops, 'pixel_moments', refuse)
    old = RenderRunner(new_timestamp='den', denoise=True, denoise_levels=3, **kw)
    assert not old.denoise_variance and old.denoise_params == dict(dr.START, levels=3) and not old.model.pixel_moments
    torch.manual_seed(0)
    assert old.run() == [0, 1]
    assert counted == {'denoisers': 4, 'launches': 6, 'variance_launches': 6, 'moments': 2 * CHUNKS}
    var, den = [str(tmp_path / 'scene' / t / 'plots') for t in ('var', 'den')]
    assert sorted(os.listdir(var)) == sorted(os.listdir(den)) and os.listdir(var)
    assert sum(f.endswith('.png') for f in os.listdir(var)) == 2
    changed = False
    for f in os.listdir(var):
        if f.startswith('rerender_rgb'):
            x, y = exr.imread(os.path.join(var, f)), exr.imread(os.path.join(den, f))
            assert np.isfinite(x).all() and (x >= 0).all(), f
            changed = changed or not np.array_equal(x, y)
        if f.startswith('diffuse_albedo'):
            assert np.array_equal(exr.imread(os.path.join(var, f)), exr.imread(os.path.join(den, f)))
    assert changed
    for bad in (dict(denoise=False), dict(num_rays=1), dict(denoise_sigma_luminance=-1.)):
        with pytest.raises(ValueError):
            RenderRunner(new_timestamp='bad', **dict(dict(kw, denoise=True, denoise_variance=True), **bad))
    with pytest.raises(ValueError):
        RenderRunner(new_timestamp='bad', denoise=True, denoise_sigma_luminance=2., **kw)


def test_turntable_cli_with_denoise_variance(tmp_path, counted, monkeypatch):
    from PIL import Image
    from nefii_amd import ops
    from nefii_amd.scripts.vis_rotate_envlight import TurntableRunner
    kw = dict(experiment(tmp_path), angle_delta=180, env_height=8, env_width=16)
    torch.manual_seed(0)
    assert TurntableRunner(plots_dir=str(tmp_path / 'var'), new_timestamp='var', denoise=True, denoise_variance=True,
                           **kw).run() == [0, 1]
    # two views, two angles each: the guides once per view; levels launches per angle; moments per chunk and angle
    assert counted == {'denoisers': 2, 'launches': 0, 'variance_launches': 2 * 2 * P['levels'], 'moments': 2 * 2 * CHUNKS}
    monkeypatch.setattr(ops, 'denoise_atrous_variance', refuse)
    monkeypatch.setattr(ops, 'pixel_moments', refuse)
    torch.manual_seed(0)
    assert TurntableRunner(plots_dir=str(tmp_path / 'den'), new_timestamp='den', denoise=True, **kw).run() == [0, 1]
    assert counted == {'denoisers': 4, 'launches': 2 * 2 * dr.START['levels'], 'variance_launches': 2 * 2 * P['levels'],
                       'moments': 2 * 2 * CHUNKS}
    var, den = sorted(os.listdir(str(tmp_path / 'var'))), sorted(os.listdir(str(tmp_path / 'den')))
    assert var == den and len(var) == 2 * (2 * 3 + 1)
    png = lambda d, f: np.asarray(Image.open(str(tmp_path / d / f)))
    assert any(not np.array_equal(png('var', f), png('den', f)) for f in var if '-render-' in f)
    for f in var:
        if '-env-' in f or '-gt_rgb-' in f:
            assert np.array_equal(png('var', f), png('den', f)), f
        if '-material-' in f:                           # normal | albedo are not filtered
            assert np.array_equal(png('var', f)[:, :32], png('den', f)[:, :32]), f
