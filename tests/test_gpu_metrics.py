"""The image metrics on the GPU: nefii_image_metrics against the fp64 oracle (tests/metrics_ref.py) on the
kernel's own fp32 inputs, its bitwise guarantees, nefii_amd.metrics against scripts/evaluate.py's functions, and
`evaluate --gpu` against `evaluate` on a synthetic split.

The bound is absolute, 1e-9 on every level mean and on MS-SSIM, and 1e-9 relative on the squared error.  It is derived, not
measured: the values are <= 1 and fp64's unit round-off is 1.1e-16; the subtraction e - mu^2 amplifies it by at most 1 / C2 =
1.1e3; a few dozen operations and a double sum follow.  That leaves two decades of margin.  Every test prints what it
measured (-s shows it)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import metrics_ref as mr  # noqa: E402

DEV = torch.device('cuda')
pytestmark = pytest.mark.gpu

BOUND = 1e-9


def gpu(x, y, levels, data_range=1.0):
    """numpy [B, H, W, C] float32 -> (stats [B, levels, C, 2], sq_err [B, C]) as numpy float64"""
    from nefii_amd import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    stats, sq = ops.image_metrics(t(x), t(y), levels, data_range)
    assert stats.dtype == torch.float64 and sq.dtype == torch.float64 and stats.is_cuda and sq.is_cuda
    return stats.cpu().numpy(), sq.cpu().numpy()


def three_pairs(H, W, C, seed):
    """random images, a noisy copy, an anti-correlated checker: [3, H, W, C] each"""
    pairs = [mr.random_pair(H, W, C, seed), mr.noisy_pair(H, W, C, seed + 1), mr.checker_pair(H, W, C)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def judge(x, y, levels, what):
    """a batch of three through the kernel: each image against the oracle and, bitwise, against the same image run alone"""
    B = x.shape[0]
    stats, sq = gpu(x, y, levels)
    assert stats.shape == (B, levels, x.shape[3], 2) and sq.shape == (B, x.shape[3])
    worst = [0., 0., 0.]
    for b in range(B):
        want, want_sq = mr.stats(x[b], y[b], levels), mr.squared_error(x[b], y[b])
        worst[0] = max(worst[0], np.abs(stats[b] - want).max())
        worst[1] = max(worst[1], (np.abs(sq[b] - want_sq) / want_sq).max())
        if levels == mr.LEVELS:
            worst[2] = max(worst[2], abs(mr.ms_ssim_from_stats(stats[b]) - mr.ms_ssim(x[b], y[b])))
        alone, alone_sq = gpu(x[b:b + 1], y[b:b + 1], levels)
        assert np.array_equal(alone[0], stats[b]) and np.array_equal(alone_sq[0], sq[b]), (what, b)    # no cross-talk
    print('%s: level means %.3e, squared error %.3e relative, MS-SSIM %.3e' % ((what,) + tuple(worst)))
    assert np.isfinite(stats).all() and np.isfinite(sq).all()
    assert worst[0] <= BOUND and worst[1] <= BOUND and worst[2] <= BOUND, (what, worst)
    return stats, sq


# ---- 1. against the fp64 oracle ---------------------------------------------------------------------------------------
# a workgroup owns 16 x 32 valid positions, a 26 x 42 patch.  11 x 11: one window; 11 x 27, 12 x 13: part of one tile; 25 x 41,
# 26 x 42, 27 x 43: one position below, at and above the tile's edges; 42 x 74: two tiles each way exactly; 43 x 75: one more
ONE_LEVEL = [(11, 11), (11, 27), (12, 13), (25, 41), (26, 42), (27, 43), (26, 43), (27, 42), (42, 74), (43, 75)]
FIVE_LEVELS = [(161, 163), (176, 161), (168, 176)]


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('shape', ONE_LEVEL, ids=lambda s: '%dx%d' % s)
def test_one_level_matches_the_oracle(shape, C):
    x, y = three_pairs(*shape, C, seed=shape[0] * 100 + shape[1])
    stats, _ = judge(x, y, 1, '%d x %d x %d' % (shape + (C,)))
    if min(shape) >= 12:
        assert (stats[2, 0, :, 1] < 0).all()            # the checker's structure term is negative


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('shape', FIVE_LEVELS, ids=lambda s: '%dx%d' % s)
def test_five_levels_match_the_oracle(shape, C):
    x, y = three_pairs(*shape, C, seed=shape[0] + 7)
    stats, _ = judge(x, y, 5, '%d x %d x %d, five levels' % (shape + (C,)))
    assert (stats[2, 0, :, 1] < 0).all() and mr.ms_ssim_from_stats(stats[2]) == 0.     # clamped by the relu
    one, _ = gpu(x, y, 1)
    assert np.array_equal(one[:, 0], stats[:, 0])       # level 0 of MS-SSIM is SSIM's


def test_data_range_scales_the_constants():
    x, y = three_pairs(43, 75, 3, seed=5)
    a, _ = gpu(x, y, 1)
    b, sq = gpu(x * np.float32(255), y * np.float32(255), 1, data_range=255.)
    want = np.stack([mr.stats(x[i] * np.float32(255), y[i] * np.float32(255), 1, 255.) for i in range(3)])
    assert np.abs(b - want).max() <= BOUND
    assert np.abs(a - b).max() < 1e-3 and not np.array_equal(a, b)      # the same images up to the fp32 rounding of x 255


# ---- 2. bitwise -------------------------------------------------------------------------------------------------------
def test_bitwise_guarantees():
    x, y = three_pairs(168, 176, 3, seed=11)
    a, a_sq = gpu(x, y, 5)
    b, b_sq = gpu(x, y, 5)
    assert np.array_equal(a, b) and np.array_equal(a_sq, b_sq)                  # two runs
    gpu(y, x, 5)                                                                # the cached workspace is used in between
    b, b_sq = gpu(x, y, 5)
    assert np.array_equal(a, b) and np.array_equal(a_sq, b_sq)
    same, same_sq = gpu(x, x.copy(), 5)
    assert (same_sq == 0.).all()                                                # identical inputs: exactly 0
    assert np.abs(same - 1.).max() < 1e-12
    x1, y1 = three_pairs(43, 75, 4, seed=12)
    a, a_sq = gpu(x1, y1, 1)
    b, b_sq = gpu(x1, y1, 1)
    assert np.array_equal(a, b) and np.array_equal(a_sq, b_sq)
    order = [2, 0, 1]                                                           # a place in the batch changes nothing
    c, c_sq = gpu(x1[order], y1[order], 1)
    assert np.array_equal(c, a[order]) and np.array_equal(c_sq, a_sq[order])


# ---- 3. nefii_amd.metrics ---------------------------------------------------------------------------------------------
def test_metrics_module_matches_evaluate():
    from nefii_amd import metrics
    from nefii_amd.scripts import evaluate as ev
    x, y = three_pairs(168, 176, 3, seed=21)
    t = lambda a: torch.from_numpy(a).to(DEV)
    want = {'ssim': [ev.calculate_ssim(x[b], y[b]) for b in range(3)], 'ms_ssim': [ev.calculate_ms_ssim(x[b], y[b]) for b in range(3)],
            'psnr': [ev.calculate_psnr(x[b], y[b]) for b in range(3)], 'mse': [ev.calculate_mse(x[b], y[b]) for b in range(3)]}
    got = {'ssim': metrics.ssim(t(x), t(y)), 'ms_ssim': metrics.ms_ssim(t(x), t(y)), 'psnr': metrics.psnr(t(x), t(y)),
           'mse': metrics.mse(t(x), t(y))}
    both = metrics.ssim_and_ms_ssim(t(x), t(y))
    every = metrics.all_metrics(t(x), t(y))
    for k in want:
        assert isinstance(got[k], list) and len(got[k]) == 3 and all(isinstance(v, float) for v in got[k])
        err = max(abs(a - b) for a, b in zip(got[k], want[k]))
        print('%s: %.3e' % (k, err))
        assert err <= BOUND, (k, got[k], want[k])
        assert every[k] == got[k]
    assert both == (got['ssim'], got['ms_ssim'])
    # one image: Python floats
    one = {'ssim': metrics.ssim(t(x[1]), t(y[1])), 'ms_ssim': metrics.ms_ssim(t(x[1]), t(y[1])),
           'psnr': metrics.psnr(t(x[1]), t(y[1])), 'mse': metrics.mse(t(x[1]), t(y[1]))}
    for k in want:
        assert isinstance(one[k], float) and one[k] == got[k][1]
    assert metrics.ssim_and_ms_ssim(t(x[1]), t(y[1])) == (one['ssim'], one['ms_ssim'])
    assert metrics.psnr(t(x[0]), t(x[0]).clone()) == float('inf') and metrics.mse(t(x[0]), t(x[0]).clone()) == 0.
    # data_range, one channel, a side too small for five scales
    assert abs(metrics.ssim(t(x[0, ..., :1] * np.float32(255)), t(y[0, ..., :1] * np.float32(255)), data_range=255.) -
               ev.calculate_ssim(x[0, ..., :1] * np.float32(255), y[0, ..., :1] * np.float32(255), 255.)) <= BOUND
    small = metrics.all_metrics(t(x[0, :100]), t(y[0, :100]))
    assert np.isnan(small['ms_ssim']) and abs(small['ssim'] - ev.calculate_ssim(x[0, :100], y[0, :100])) <= BOUND
    with pytest.raises(ValueError):
        metrics.ms_ssim(t(x[0, :160]), t(y[0, :160]))


# ---- 4. evaluate --gpu ------------------------------------------------------------------------------------------------
def synthetic_split(tmp_path, H=168, W=176, views=(0, 3)):
    from PIL import Image
    from nefii_amd.utils import exr
    g = np.random.Generator(np.random.Philox(4))
    gt, plots = tmp_path / 'scene' / 'test', tmp_path / 'exp' / 'plots'
    for d in ('image', 'diffuse', 'roughness', 'sp_rgb', 'mask'):
        (gt / d).mkdir(parents=True)
    plots.mkdir(parents=True)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = (((yy - H / 2) / (0.4 * H)) ** 2 + ((xx - W / 2) / (0.4 * W)) ** 2 < 1).astype(np.uint8) * 255
    smooth = lambda: (0.45 + 0.4 * np.sin(xx / g.uniform(5, 12) + g.uniform(0, 3))[..., None] *
                      np.cos(yy / g.uniform(4, 9))[..., None] * g.uniform(0.5, 1, 3)).astype(np.float32)
    noisy = lambda a, s: np.clip(a + g.normal(0, s, a.shape), 0.01, None).astype(np.float32)
    for i in views:
        Image.fromarray(mask).save(gt / 'mask' / ('%06d.png' % i))
        truth = {k: smooth() for k in ('rgb', 'diffuse', 'rough', 'sp')}
        exr.imwrite(str(gt / 'image' / ('%06d.exr' % i)), truth['rgb'])
        exr.imwrite(str(gt / 'diffuse' / ('%06d_diffuse.00.exr' % i)), truth['diffuse'])
        exr.imwrite(str(gt / 'roughness' / ('%06d.exr' % i)), truth['rough'])
        exr.imwrite(str(gt / 'sp_rgb' / ('%06d_sprgb.00.exr' % i)), truth['sp'])
        exr.imwrite(str(plots / ('rerender_rgb-%03d.exr' % i)), noisy(truth['rgb'], 0.02))
        exr.imwrite(str(plots / ('diffuse_albedo-%03d.exr' % i)), noisy(truth['diffuse'] * np.float32(0.5), 0.01))
        exr.imwrite(str(plots / ('roughness-%03d.exr' % i)), noisy(truth['rough'], 0.05))
        exr.imwrite(str(plots / ('specular_rgb-%03d.exr' % i)), noisy(truth['sp'] * np.float32(1.1), 0.03))
    return str(plots), str(gt), tmp_path / 'exp' / 'results.txt'


def test_evaluate_with_and_without_gpu(tmp_path, monkeypatch):
    from nefii_amd import ops
    from nefii_amd.scripts import evaluate as ev
    plots, gt, results = synthetic_split(tmp_path)
    calls = []
    real = ops.image_metrics
    monkeypatch.setattr(ops, 'image_metrics', lambda *a, **kw: calls.append(a[2]) or real(*a, **kw))
    host = ev.main(plots, gt)
    assert calls == []                                  # without the flag the device path is not touched
    first = results.read_text()
    dev = ev.main(plots, gt, gpu=True)
    assert calls == [5, 5, 1, 5, 1, 5] * 2              # one call per image pair: four evaluate_rgb, two evaluate_raw per view
    second = results.read_text()
    assert set(dev) == set(host) == {'rgb', 'diffuse', 'diffuse_align', 'roughness', 'sp_rgb'}
    for key in host:
        assert list(dev[key]) == list(host[key])
        for k, v in host[key].items():
            if k == 'lpips':
                assert np.isnan(v) and np.isnan(dev[key][k])
            else:
                print('%s %s: host %.12f, device %.12f' % (key, k, v, dev[key][k]))
                assert np.isfinite(v) and abs(dev[key][k] - v) <= BOUND, (key, k, v, dev[key][k])
    assert 0.3 < host['rgb']['ssim'] < 1 and 0.3 < host['rgb']['ms_ssim'] < 1 and 20 < host['rgb']['psnr'] < 60
    assert second.startswith(first) and second[len(first):] == first and first.count('>>>>>>>>>>') == 5
