"""CPU checks of the SG envmap fit (nefii_amd.lighting, scripts/fit_envmap, the nefii_envfit_* boundary): resampling,
rotation, the restated objective against tests/golden/envfit_ref.npz, and the host-side argument checks (no GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'envfit_ref.npz')


def sg_envmap64(lgt, dirs, eps=1e-8):
    lgt, dirs = torch.as_tensor(lgt).double(), torch.as_tensor(dirs).double()
    a = lgt[:, :3] / (torch.norm(lgt[:, :3], dim=-1, keepdim=True) + eps)
    return torch.exp(lgt[:, 3].abs() * (dirs @ a.T - 1.)) @ lgt[:, 4:].abs()


def coverage_brute(img, H, W):
    """each output pixel: the area-weighted mean of the input pixels its footprint overlaps, in 2-D directly"""
    h, w = img.shape[:2]
    out = np.zeros((H, W) + img.shape[2:])
    for I in range(H):
        y0, y1 = I * h / H, (I + 1) * h / H
        for J in range(W):
            x0, x1 = J * w / W, (J + 1) * w / W
            acc, area = 0., 0.
            for i in range(h):
                oy = max(0., min(y1, i + 1) - max(y0, i))
                for j in range(w):
                    a = oy * max(0., min(x1, j + 1) - max(x0, j))
                    acc = acc + a * img[i, j]
                    area += a
            out[I, J] = acc / area
    return out


def test_resample_area_integer_factor_gives_block_means():
    from nefii_amd.lighting import resample_area
    img = np.random.default_rng(0).random((12, 20, 3)).astype(np.float32) * 5
    out = resample_area(img, 4, 5)
    assert out.shape == (4, 5, 3) and out.dtype == np.float32
    np.testing.assert_allclose(out, img.astype(np.float64).reshape(4, 3, 5, 4, 3).mean(axis=(1, 3)), rtol=1e-7)
    t = resample_area(torch.from_numpy(img).double(), 6, 10)
    assert isinstance(t, torch.Tensor) and t.shape == (6, 10, 3) and t.dtype == torch.float64
    np.testing.assert_allclose(t.numpy(), img.astype(np.float64).reshape(6, 2, 10, 2, 3).mean(axis=(1, 3)), rtol=1e-12)
    assert resample_area(img[..., 0], 3, 4).shape == (3, 4)


def test_resample_area_non_integer_matches_brute_force_coverage_and_keeps_the_mean():
    from nefii_amd.lighting import resample_area
    img = np.random.default_rng(1).random((13, 17, 3)) * 3
    for H, W in [(5, 7), (6, 4), (13, 9), (26, 40)]:          # down, down, one axis, up
        out = resample_area(img, H, W)
        assert out.shape == (H, W, 3)
        np.testing.assert_allclose(out, coverage_brute(img, H, W), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(out.mean(axis=(0, 1)), img.mean(axis=(0, 1)), rtol=1e-12)
    assert np.array_equal(resample_area(img, 13, 17), img)


def test_rotate_light_sgs_identity_is_the_canonical_form():
    from nefii_amd.lighting import rotate_light_sgs
    lgt = np.random.default_rng(2).standard_normal((9, 7)).astype(np.float32)
    out = rotate_light_sgs(lgt, [0, 0, 0])
    want = np.concatenate((lgt[:, :3] / (np.linalg.norm(lgt[:, :3], axis=-1, keepdims=True) + 1e-8),
                           np.abs(lgt[:, 3:4]), np.abs(lgt[:, 4:])), axis=-1)
    assert out.dtype == np.float32 and out.shape == (9, 7)
    np.testing.assert_allclose(out, want, rtol=1e-6, atol=1e-7)


def test_rotated_light_at_d_is_the_original_at_rt_d():
    from scipy.spatial.transform import Rotation
    from nefii_amd.lighting import rotate_light_sgs
    g = torch.Generator().manual_seed(3)
    lgt = torch.randn(16, 7, generator=g, dtype=torch.float64)
    lgt[:, 3] *= 20
    d = torch.nn.functional.normalize(torch.randn(500, 3, generator=g, dtype=torch.float64), dim=-1)
    for angles in ([90, 0, 0], [30, -45, 120]):
        R = torch.from_numpy(Rotation.from_euler('yxz', angles, degrees=True).as_matrix())
        rot = rotate_light_sgs(lgt, angles)
        assert isinstance(rot, torch.Tensor) and rot.dtype == torch.float64
        np.testing.assert_allclose(sg_envmap64(rot, d, eps=0.).numpy(), sg_envmap64(lgt, d @ R, eps=0.).numpy(),
                                   rtol=1e-6, atol=1e-12)


def test_restated_objective_matches_the_fixture():
    from nefii_amd.lighting import init_light_sgs
    from nefii_amd.training.render import envmap_directions
    z = np.load(GOLDEN)
    H, W = z['target'].shape[:2]
    assert torch.equal(init_light_sgs(128, 0), torch.from_numpy(z['init']))
    dirs = envmap_directions(H, W, coordinate_type='blender').reshape(-1, 3)
    p = torch.from_numpy(z['init']).double().requires_grad_(True)
    loss = torch.mean((sg_envmap64(p, dirs) - torch.from_numpy(z['target']).reshape(-1, 3).double()) ** 2)
    loss.backward()
    assert abs(loss.item() - float(z['loss64'])) <= 1e-10 * float(z['loss64'])
    np.testing.assert_allclose(p.grad.numpy(), z['grad64'], rtol=1e-8, atol=1e-12 * np.abs(z['grad64']).max())
    assert list(z['curve_steps']) == [0, 10, 100, 1000, 3000] and z['curve'][-1] < z['curve'][0]


def test_envfit_host_argument_checks_need_no_gpu():
    from nefii_amd import _lib
    lib = _lib.lib()
    assert lib.nefii_envfit_workspace_bytes(256 * 512, 128) == 512 * (128 * 7 + 1) * 4
    assert lib.nefii_envfit_workspace_bytes(257, 7) == 2 * (7 * 7 + 1) * 4
    for n, m in [(0, 128), (100, 0), (100, 513), (-5, 4)]:
        assert lib.nefii_envfit_workspace_bytes(n, m) == 0
    fake = ctypes.c_void_p(64)                       # non-null, never dereferenced: the checks fail first
    assert lib.nefii_envfit_loss_grad(None, 128, fake, fake, 100, 1e-8, fake, fake, fake, None, None) == -1
    assert lib.nefii_envfit_loss_grad(fake, 128, fake, fake, 100, 1e-8, None, fake, fake, None, None) == -1
    for n, m in [(0, 128), (100, 0), (100, 513), (-1, 8)]:
        assert lib.nefii_envfit_loss_grad(fake, m, fake, fake, n, 1e-8, fake, fake, fake, None, None) == -2
    args = lambda m, n, iters, losses=fake: (fake, fake, fake, m, fake, fake, n, 1e-8, 1e-2, 0.9, 0.999, 1e-8, 0, iters,
                                             fake, losses, None)
    assert lib.nefii_envfit_adam(*args(128, 100, 10, None)) == -1
    assert lib.nefii_envfit_adam(*args(128, 100, -1)) == -1
    assert lib.nefii_envfit_adam(*args(600, 100, 10)) == -2
    assert lib.nefii_envfit_adam(*args(128, 0, 10)) == -2


def test_envfit_ops_refuse_cpu_tensors():
    from nefii_amd import ops
    lgt, d = torch.zeros(4, 7), torch.zeros(10, 3)
    with pytest.raises(RuntimeError):
        ops.envfit_loss_grad(lgt, d, d)
    with pytest.raises(RuntimeError):
        ops.envfit_adam(lgt, torch.zeros_like(lgt), torch.zeros_like(lgt), d, d, 0, 5)
    with pytest.raises(ValueError):
        ops.envfit_loss_grad(torch.zeros(4, 6), d, d)
    with pytest.raises(ValueError):
        ops.envfit_loss_grad(torch.zeros(600, 7), d, d)


def test_fit_envmap_cli_arguments(capsys):
    from nefii_amd.scripts import fit_envmap
    with pytest.raises(SystemExit) as e:
        fit_envmap.parse_args(['--help'])
    assert e.value.code == 0 and '--coordinate_type' in capsys.readouterr().out
    a = fit_envmap.parse_args(['--envmap', '/x/sky.exr', '--rotate', '90,0,-30', '--iters', '10'])
    assert a.out_dir == '/x/sky' and a.rotate == [90., 0., -30.] and a.num_lobes == 128 and a.iters == 10
    assert (a.height, a.width, a.coordinate_type, a.lr, a.log_every) == (256, 512, 'mitsuba', 1e-2, 100)
    for bad in (['--rotate', '90,0'], ['--num_lobes', '0'], ['--log_every', '0'], ['--coordinate_type', 'opengl']):
        with pytest.raises(SystemExit) as e:
            fit_envmap.parse_args(['--envmap', 'a.exr'] + bad)
        assert e.value.code != 0


def test_log_image_is_the_reference_tone_map():
    from nefii_amd.scripts.fit_envmap import log_image
    t, f = np.full((2, 3, 3), 0.25, np.float32), np.full((2, 3, 3), 4.0, np.float32)
    im = log_image(t, f)
    assert im.shape == (4, 3, 3) and im.dtype == np.uint8
    assert im[0, 0, 0] == np.uint8(0.25 ** (1 / 2.2) * 255.) and im[3, 0, 0] == 255


def test_lights_over_512_lobes_are_refused_with_a_value_error(tmp_path):
    """every kernel that takes lgtSGs stops at NEFII_MAX_LOBES: the wrappers and load_light say so before any launch"""
    import numpy as np
    from nefii_amd import ops
    from nefii_amd.model.sg_envmap_material import EnvmapMaterialNetwork
    big, n = torch.zeros(ops.MAX_LOBES + 1, 7), torch.zeros(1, 3)
    for call in (lambda: ops.SGRenderFn.apply(big, torch.zeros(1, 3), torch.ones(1, 1), n, n, n),
                 lambda: ops.EnvRadianceFn.apply(big, n, 1e-8),
                 lambda: ops.mis_sample(big, torch.ones(1), n, n, torch.zeros(1, 7)),
                 lambda: ops.envfit_loss_grad(big, n, n),
                 lambda: ops.SGRenderFn.apply(torch.zeros(0, 7), torch.zeros(1, 3), torch.ones(1, 1), n, n, n)):
        with pytest.raises(ValueError, match='1 <= M <= 512'):
            call()
    net = EnvmapMaterialNetwork(dims=[32], num_lgt_sgs=8, num_base_materials=1)
    np.save(str(tmp_path / 'ok.npy'), np.ones((ops.MAX_LOBES, 7), np.float32))
    net.load_light(str(tmp_path / 'ok.npy'))
    assert net.lgtSGs.shape == (ops.MAX_LOBES, 7) and net.numLgtSGs == ops.MAX_LOBES
    np.save(str(tmp_path / 'big.npy'), np.ones((ops.MAX_LOBES + 1, 7), np.float32))
    with pytest.raises(ValueError, match='512'):
        net.load_light(str(tmp_path / 'big.npy'))
