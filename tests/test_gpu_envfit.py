"""The fused SG envmap fit on the GPU (nefii_envfit_loss_grad / nefii_envfit_adam, nefii_amd.lighting,
scripts/fit_envmap) against fp64 torch autograd, torch.optim.Adam and the fixture's reference loss curve
(tests/golden/envfit_ref.npz: sunrise.exr at 64 x 128, blender convention)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'envfit_ref.npz')
DEV = torch.device('cuda:0')


def fixture():
    from nefii_amd.training.render import envmap_directions
    z = np.load(GOLDEN)
    H, W = z['target'].shape[:2]
    dirs = envmap_directions(H, W, coordinate_type='blender').reshape(-1, 3).contiguous()
    return z, torch.from_numpy(z['target']).reshape(-1, 3).contiguous(), dirs


def loss_grad64(lgt, dirs, target, eps=1e-8):
    p = lgt.double().clone().requires_grad_(True)
    d = dirs.double()
    a = p[:, :3] / (torch.norm(p[:, :3], dim=-1, keepdim=True) + eps)
    rgb = torch.exp(p[:, 3].abs() * (d @ a.T - 1.)) @ p[:, 4:].abs()
    loss = torch.mean((rgb - target.double()) ** 2)
    loss.backward()
    return loss.item(), p.grad


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize('M,n', [(128, 8192), (100, 8192 - 77), (7, 5000), (300, 3001)])
def test_loss_and_gradient_match_fp64_autograd(M, n):
    from nefii_amd import ops
    from nefii_amd.lighting import init_light_sgs
    z, target, dirs = fixture()
    lgt = torch.from_numpy(z['init'])[:M].clone() if M <= 128 else init_light_sgs(M, 1)
    lgt[3, 4] = 0.                      # exact zeros: abs has gradient 0 there (torch's sign(0))
    lgt[5, 4:] = 0.
    lgt[2, 3] = 0.
    target, dirs = target[:n].contiguous(), dirs[:n].contiguous()
    loss64, g64 = loss_grad64(lgt, dirs, target)
    loss, g = ops.envfit_loss_grad(lgt.to(DEV), dirs.to(DEV), target.to(DEV))
    g = g.cpu()
    assert abs(loss.item() - loss64) <= 1e-5 * loss64, (loss.item(), loss64)
    for name, sl in (('axes', slice(0, 3)), ('lambda', slice(3, 4)), ('mu', slice(4, 7))):
        assert rel(g[:, sl], g64[:, sl]) <= 1e-4, (name, rel(g[:, sl], g64[:, sl]))
    assert g[3, 4] == 0 and torch.all(g[5, 4:] == 0) and g[2, 3] == 0
    # the fused forward agrees with the background-radiance kernel (eps = 0 there; |v| + 1e-8 rounds to |v| or one ulp off)
    _, _, rgb = ops.envfit_loss_grad(lgt.to(DEV), dirs.to(DEV), target.to(DEV), want_rgb=True)
    env = ops.EnvRadianceFn.apply(lgt.to(DEV), dirs.to(DEV), 0.0)
    assert rel(rgb.cpu(), env.cpu()) <= 1e-5


def test_adam_step_equals_torch_adam_on_the_kernel_gradient():
    from nefii_amd import ops
    z, target, dirs = fixture()
    target, dirs = target.to(DEV), dirs.to(DEV)
    lgt = torch.from_numpy(z['init']).to(DEV)
    p = torch.nn.Parameter(lgt.clone())
    opt = torch.optim.Adam([p], lr=1e-2)
    m, v = torch.zeros_like(lgt), torch.zeros_like(lgt)
    for step in range(3):
        loss, g = ops.envfit_loss_grad(p.detach().contiguous(), dirs, target)
        p.grad = g.clone()
        opt.step()
        losses = ops.envfit_adam(lgt, m, v, dirs, target, step, 1)
        assert losses[0].item() == loss.item()               # the same kernels: bitwise
        st = opt.state[p]
        tol = torch.clamp(p.detach().abs() * 2.0 ** -23, min=1e-6)   # 1e-6, or one float ulp of a large parameter
        assert torch.all((lgt - p.detach()).abs() <= tol), (lgt - p.detach()).abs().max().item()
        torch.testing.assert_close(m, st['exp_avg'], atol=1e-6, rtol=0)
        torch.testing.assert_close(v, st['exp_avg_sq'], atol=1e-6, rtol=0)
        with torch.no_grad():
            p.copy_(lgt)                                     # keep both walks on one trajectory


@pytest.mark.parametrize('M', [1, 512])
@pytest.mark.parametrize('n', [1, 255, 257])
def test_loss_and_gradient_at_the_shape_boundaries(M, n):
    """one lobe and the most lobes (NEFII_MAX_LOBES), with n below one 256-direction tile, one short of it and one over
    it (a second, nearly empty slab)"""
    from nefii_amd import ops
    from nefii_amd.lighting import init_light_sgs
    _, target, dirs = fixture()
    idx = torch.randperm(dirs.shape[0], generator=torch.Generator().manual_seed(n))[:n]
    target, dirs = target[idx].contiguous(), dirs[idx].contiguous()
    lgt = init_light_sgs(M, 2)
    lgt[0, :3] = 1.3 * dirs[0] + torch.tensor([0.3, -0.2, 0.25])    # a lobe near every direction: no gradient underflows
    lgt[0, 3] = 5.
    lgt[0, 5] = 0.
    loss64, g64 = loss_grad64(lgt, dirs, target)
    loss, g = ops.envfit_loss_grad(lgt.to(DEV), dirs.to(DEV), target.to(DEV))
    g = g.cpu()
    assert abs(loss.item() - loss64) <= 1e-5 * loss64, (loss.item(), loss64)
    for name, sl in (('axes', slice(0, 3)), ('lambda', slice(3, 4)), ('mu', slice(4, 7))):
        assert rel(g[:, sl], g64[:, sl]) <= 1e-4, (name, rel(g[:, sl], g64[:, sl]))
    assert g[0, 5] == 0


def test_adam_step_at_512_lobes_equals_torch_adam():
    from nefii_amd import ops
    from nefii_amd.lighting import init_light_sgs
    _, target, dirs = fixture()
    target, dirs = target.to(DEV), dirs.to(DEV)
    lgt = init_light_sgs(ops.MAX_LOBES, 3).to(DEV)
    p = torch.nn.Parameter(lgt.clone())
    opt = torch.optim.Adam([p], lr=1e-2)
    m, v = torch.zeros_like(lgt), torch.zeros_like(lgt)
    loss, g = ops.envfit_loss_grad(lgt, dirs, target)
    p.grad = g.clone()
    opt.step()
    losses = ops.envfit_adam(lgt, m, v, dirs, target, 0, 1)
    assert losses[0].item() == loss.item()
    tol = torch.clamp(p.detach().abs() * 2.0 ** -23, min=1e-6)
    assert torch.all((lgt - p.detach()).abs() <= tol), (lgt - p.detach()).abs().max().item()
    torch.testing.assert_close(m, opt.state[p]['exp_avg'], atol=1e-6, rtol=0)
    torch.testing.assert_close(v, opt.state[p]['exp_avg_sq'], atol=1e-6, rtol=0)
    with pytest.raises(ValueError, match='512'):
        ops.envfit_loss_grad(torch.zeros(ops.MAX_LOBES + 1, 7, device=DEV), dirs, target)


def test_fit_is_bitwise_reproducible():
    from nefii_amd.lighting import SGEnvmapFitter
    z, target, dirs = fixture()
    runs = []
    for _ in range(2):
        f = SGEnvmapFitter(target, dirs, lgt=torch.from_numpy(z['init']), device=DEV)
        f.fit(50)
        st = f.state()
        f2 = SGEnvmapFitter(target, dirs, num_lobes=128, seed=5, device=DEV)
        f2.load(st)                                          # resume through state() / load()
        losses = f2.fit(150)
        runs.append((losses, f2.state()))
    (l0, s0), (l1, s1) = runs
    assert torch.equal(l0, l1) and s0['step'] == s1['step'] == 200
    for k in ('lgtSGs', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(s0[k], s1[k]), k


def test_fit_follows_the_reference_loss_curve():
    from nefii_amd.lighting import SGEnvmapFitter
    z, target, dirs = fixture()
    steps, curve = [int(s) for s in z['curve_steps']], z['curve']
    f = SGEnvmapFitter(target, dirs, lgt=torch.from_numpy(z['init']), device=DEV)
    losses = f.fit(steps[-1] + 1).numpy()
    assert abs(losses[0] - curve[0]) <= 1e-5 * curve[0], (losses[0], curve[0])
    for s, ref in zip(steps, curve):
        if s >= 100:
            assert losses[s] <= 1.1 * ref, (s, losses[s], ref)


def test_fit_envmap_cli_light_relights_through_load_light(tmp_path):
    from nefii_amd.model.sg_envmap_material import EnvmapMaterialNetwork
    from nefii_amd.training.render import write_envmap
    from nefii_amd.utils import exr
    from PIL import Image
    z = np.load(GOLDEN)
    H, W = z['target'].shape[:2]
    src = tmp_path / 'sky.exr'
    exr.imwrite(str(src), np.concatenate([z['target'], np.ones((H, W, 1), np.float32)], -1))   # RGBA, as sunrise.exr
    out = tmp_path / 'fit'
    cmd = [sys.executable, '-m', 'nefii_amd.scripts.fit_envmap', '--envmap', str(src), '--out_dir', str(out),
           '--height', str(H // 2), '--width', str(W // 2), '--coordinate_type', 'blender', '--iters', '300',
           '--log_every', '100', '--rotate', '90,0,0']
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    M = 128
    sg = np.load(out / ('sg_%d.npy' % M))
    assert sg.shape == (M, 7) and sg.dtype == np.float32 and (out / ('sg_%d_rot.npy' % M)).exists()
    assert np.asarray(Image.open(out / ('log_im_%d.png' % M))).shape == (H, W // 2, 3)
    net = EnvmapMaterialNetwork(dims=[32], num_lgt_sgs=M, num_base_materials=1).to(DEV)
    net.load_light(str(out / ('sg_%d.npy' % M)))
    env = write_envmap(types.SimpleNamespace(envmap_material_network=net), str(tmp_path / 'plots'),
                       coordinate_type='blender', H=H // 2, W=W // 2).cpu()
    fitted = torch.from_numpy(exr.imread(str(out / ('envmap_%d.exr' % M))))
    assert fitted.shape == env.shape == (H // 2, W // 2, 3)
    assert rel(env, fitted) <= 1e-5
