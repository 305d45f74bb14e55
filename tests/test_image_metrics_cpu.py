"""The GPU image metrics without a GPU: the numpy oracle (tests/metrics_ref.py) against scripts/evaluate.py's
torch calls and on special images, and the refusals of the entry point, the op, nefii_amd.metrics and `evaluate --gpu`.
(tests/test_metrics_cpu.py pins evaluate.py itself against the reference's numbers.)"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import metrics_ref as mr  # noqa: E402

from nefii_amd.scripts import evaluate as ev  # noqa: E402

SMALL = [(11, 11), (12, 13), (43, 75)]
LARGE = [(161, 163), (176, 161), (168, 176)]        # five levels; 161 -> 81 -> 41 -> 21 -> 11 is odd at every level


# ---- 1. the oracle against evaluate ----------------------------------------------------------------------------------
def test_window_is_evaluates():
    assert np.array_equal(mr.window(), ev.gaussian_window().numpy())
    assert mr.MS_WEIGHTS == ev.MS_WEIGHTS


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('shape', SMALL + LARGE, ids=lambda s: '%dx%d' % s)
def test_oracle_matches_evaluate(shape, C):
    pairs = [mr.random_pair(*shape, C, seed=shape[0] + C), mr.noisy_pair(*shape, C, seed=shape[1] + C)]
    for x, y in pairs:
        assert abs(mr.ssim(x, y) - ev.calculate_ssim(x, y)) < 1e-12
        if shape in LARGE:
            assert abs(mr.ms_ssim(x, y) - ev.calculate_ms_ssim(x, y)) < 1e-12
        # the level statistics themselves, per channel, against _ssim_cs
        t = lambda a: torch.from_numpy(a).double().permute(2, 0, 1)[None]
        s, cs = ev._ssim_cs(t(x), t(y), 1.0, ev.gaussian_window())
        st = mr.stats(x, y, 1)
        assert np.abs(st[0, :, 0] - s[0].numpy()).max() < 1e-12 and np.abs(st[0, :, 1] - cs[0].numpy()).max() < 1e-12
    x, y = pairs[0]
    assert abs(mr.ssim(x * 255, y * 255, 255.) - ev.calculate_ssim(x * 255, y * 255, 255.)) < 1e-12


@pytest.mark.parametrize('shape', [(11, 11), (12, 13), (13, 12), (43, 75), (21, 22), (161, 163)], ids=lambda s: '%dx%d' % s)
def test_pooling_rule_is_torchs(shape):
    """even sides pair (2i, 2i+1); odd sides pair (2i-1, 2i) with a zero in front and still divide by 4"""
    x, _ = mr.random_pair(*shape, 2, seed=7)
    t = torch.from_numpy(x).double().permute(2, 0, 1)[None]
    want = F.avg_pool2d(t, 2, padding=[s % 2 for s in shape])[0].permute(1, 2, 0).numpy()
    got = mr.pool(x.astype(np.float64))
    assert got.shape == want.shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2, 2)
    assert np.abs(got - want).max() < 1e-15
    levels = mr.pyramid(x)
    assert [l.shape[0] for l in levels] == [shape[0]] + [-(-shape[0] // 2 ** k) for k in range(1, 5)]


# ---- 2. special images -----------------------------------------------------------------------------------------------
def test_identical_images_give_one():
    x, _ = mr.noisy_pair(168, 176, 3, seed=1)
    st = mr.stats(x, x, 5)
    assert np.abs(st - 1.).max() < 1e-12
    assert abs(mr.ssim(x, x) - 1.) < 1e-12 and abs(mr.ms_ssim(x, x) - 1.) < 1e-12
    assert (mr.squared_error(x, x) == 0.).all()


def test_anticorrelated_checker_is_clamped():
    x, y = mr.checker_pair(168, 176, 3)
    st = mr.stats(x, y, 5)
    assert (st[0, :, 1] < -0.5).all() and (st[0, :, 0] < 0).all()               # level 0: the structure term is negative
    assert mr.ms_ssim(x, y) == 0.                                               # relu: one factor is 0
    assert abs(mr.ms_ssim(x, y) - ev.calculate_ms_ssim(x, y)) < 1e-12
    assert abs(mr.ssim(x, y) - ev.calculate_ssim(x, y)) < 1e-12


def test_constant_images():
    a, b = np.full((168, 176, 2), 0.25, np.float32), np.full((168, 176, 2), 0.75, np.float32)
    st = mr.stats(a, b, 1)
    lum = (2 * 0.25 * 0.75 + 1e-4) / (0.25 ** 2 + 0.75 ** 2 + 1e-4)
    assert np.abs(st[0, :, 1] - 1.).max() < 1e-12 and np.abs(st[0, :, 0] - lum).max() < 1e-12        # no variance: cs = C2 / C2
    assert abs(mr.ssim(a, b) - ev.calculate_ssim(a, b)) < 1e-12
    assert abs(mr.ms_ssim(a, b) - ev.calculate_ms_ssim(a, b)) < 1e-12
    assert np.abs(mr.squared_error(a, b) - 168 * 176 * 0.25).max() < 1e-9
    assert abs(mr.squared_error(a, b).sum() / (168 * 176 * 2) - ev.calculate_mse(a, b)) < 1e-15


# ---- 3. refusals -----------------------------------------------------------------------------------------------------
def test_entry_point_checks_its_arguments_on_the_host():
    from nefii_amd import _lib
    lib = _lib.lib()
    E_ARG, E_SHAPE = -1, -2
    win = (ctypes.c_double * 11)(*mr.window().tolist())
    ptr = dict(x=256, y=512, ws=768, stats=1024, sq=1280)         # never dereferenced: every call below is refused on the host
    good = dict(B=1, H=168, W=176, C=3, levels=5)

    def call(window=win, **kw):
        p, k = dict(ptr), dict(good)
        for name, v in kw.items():
            (p if name in p else k)[name] = v
        return lib.nefii_image_metrics(p['x'], p['y'], k['B'], k['H'], k['W'], k['C'], k['levels'], window, 1e-4, 9e-4, p['ws'],
                                       p['stats'], p['sq'], None)

    def size(**kw):
        k = dict(good, **kw)
        return lib.nefii_image_metrics_workspace_bytes(k['B'], k['H'], k['W'], k['C'], k['levels'])
    for name in ptr:
        assert call(**{name: None}) == E_ARG, name
    assert call(window=None) == E_ARG
    for levels in (0, 2, 4, 6, -1):
        assert call(levels=levels) == E_ARG and size(levels=levels) == E_ARG
    for kw in (dict(C=0), dict(C=5), dict(B=0), dict(B=-3), dict(H=10, levels=1), dict(W=10, levels=1), dict(H=0, levels=1),
               dict(H=160), dict(W=160), dict(H=16385), dict(W=16385), dict(H=16385, levels=1)):
        assert call(**kw) == E_SHAPE and size(**kw) == E_SHAPE, kw
    # what is accepted: the workspace holds levels 1 .. 4 of both images in fp64 and three doubles per tile
    assert size(H=11, W=11, levels=1, C=1) == 3 * 8
    assert size(H=161, W=161, levels=1) == 3 * 10 * 5 * 3 * 8
    pyramid = sum(2 * 3 * h * w for h, w in ((84, 88), (42, 44), (21, 22), (11, 11)))
    tiles = sum(-(-(h - 10) // 16) * -(-(w - 10) // 32) for h, w in ((168, 176), (84, 88), (42, 44), (21, 22), (11, 11)))
    assert size() == (pyramid + 3 * 3 * tiles) * 8
    assert size(B=4) == 4 * size()
    assert size(H=16384, W=16384, C=4, levels=5) > 2 ** 32


def test_op_refuses_bad_tensors():
    from nefii_amd import ops
    x = torch.zeros(1, 168, 176, 3)
    with pytest.raises(RuntimeError):                   # well-formed, but not on the GPU: no fallback
        ops.image_metrics(x, x.clone(), 5)
    with pytest.raises(RuntimeError):
        ops.image_metrics(x, x.clone(), 1, data_range=255.)
    for a, b in [(x.double(), x.double()), (x, x.half()), (x[0], x[0]), (x, x[:, :, :175]), (x, torch.zeros(1, 176, 168, 3)),
                 (torch.zeros(1, 168, 176, 6)[..., ::2], x), (x, x.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)),
                 (torch.zeros(1, 168, 176, 5), torch.zeros(1, 168, 176, 5)), (torch.zeros(1, 168, 176, 0), torch.zeros(1, 168, 176, 0)),
                 (torch.zeros(0, 168, 176, 3), torch.zeros(0, 168, 176, 3)), (x.numpy(), x.numpy())]:
        with pytest.raises(ValueError):
            ops.image_metrics(a, b, 1)
    for levels in (0, 2, 3):
        with pytest.raises(ValueError):
            ops.image_metrics(x, x.clone(), levels)
    for dr in (0., -1., float('nan'), float('inf')):
        with pytest.raises(ValueError):
            ops.image_metrics(x, x.clone(), 1, data_range=dr)
    small, tiny = torch.zeros(1, 160, 176, 3), torch.zeros(1, 10, 176, 3)
    with pytest.raises(ValueError) as e:
        ops.image_metrics(small, small.clone(), 5)
    assert 'larger than 160' in str(e.value)
    with pytest.raises(ValueError):
        ops.image_metrics(tiny, tiny.clone(), 1)
    with pytest.raises(RuntimeError):                   # 160 is enough for one level
        ops.image_metrics(small, small.clone(), 1)
    assert np.array_equal(np.array(list(ops.metrics_window())), mr.window())


def test_metrics_module_refusals():
    from nefii_amd import metrics
    x = torch.zeros(168, 176, 3)
    for f in (metrics.ssim, metrics.ms_ssim, metrics.ssim_and_ms_ssim, metrics.psnr, metrics.mse, metrics.all_metrics):
        with pytest.raises(RuntimeError):               # CPU tensors
            f(x, x.clone())
        with pytest.raises(RuntimeError):
            f(x[None], x[None].clone())
        for a, b in [(x, x[:167]), (x.double(), x.double()), (x[0], x[0]), (x[None, None], x[None, None]),
                     (x.permute(1, 0, 2), x.permute(1, 0, 2)), (x.numpy(), x.numpy())]:
            with pytest.raises(ValueError):
                f(a, b)
    for f in (metrics.ms_ssim, metrics.ssim_and_ms_ssim):
        with pytest.raises(ValueError) as e:
            f(x[:160], x[:160].clone())
        assert 'larger than 160' in str(e.value)


# ---- 4. the command line ---------------------------------------------------------------------------------------------
def test_evaluate_gpu_without_a_device_leaves_before_reading(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(SystemExit) as e:
        ev.main(str(tmp_path / 'no' / 'plots'), str(tmp_path / 'no' / 'test'), gpu=True)     # neither exists: nothing is listed
    assert e.value.code == 2 and 'needs a usable GPU' in capsys.readouterr().err
    assert not (tmp_path / 'no').exists()
    with pytest.raises(FileNotFoundError):              # without the flag the walk starts
        ev.main(str(tmp_path / 'no' / 'plots'), str(tmp_path / 'no' / 'test'))


def test_evaluate_gpu_command_line_without_a_device(tmp_path):
    """the command itself, in a process that sees no device"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1', PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, '-m', 'nefii_amd.scripts.evaluate', '--gpu', '--pre_dir', str(tmp_path / 'plots'),
                        '--gt_dir', str(tmp_path / 'test')], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, r.stderr[-2000:]
    assert 'evaluate --gpu needs a usable GPU' in r.stderr and 'Traceback' not in r.stderr
    assert not (tmp_path / 'results.txt').exists()


# ---- 5. structure ----------------------------------------------------------------------------------------------------
def test_the_kernels_are_part_of_the_library():
    from nefii_amd import _lib, build
    assert 'nefii_metrics.hip' in build.SOURCES and os.path.exists(os.path.join(build.CSRC, 'nefii_metrics.hip'))
    header = open(os.path.join(ROOT, 'include', 'nefii_amd.h')).read()
    assert 'int nefii_image_metrics(' in header and 'int64_t nefii_image_metrics_workspace_bytes(' in header
    assert _lib.ABI_VERSION == 19 and '#define NEFII_ABI_VERSION 19' in header
    assert 'nefii_image_metrics' in _lib.SIGNATURES and 'nefii_image_metrics_workspace_bytes' in _lib.SIGNATURES
    src = open(os.path.join(build.CSRC, 'nefii_metrics.hip')).read()
    code = '\n'.join(ln.split('//')[0] for ln in src.splitlines())
    assert 'atomic' not in code.lower()                 # plain stores and fixed-order sums only
