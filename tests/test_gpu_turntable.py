"""The light turntable on the GPU: render_turntable on the fitted bowl - what it traces (ray counts per
call), every frame against a standalone render under the rotated light with the same uniforms, the shared material
buffers, the background, what it leaves behind, a column-aligned yaw against the rolled map, and the command line."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import envlight_ref as er  # noqa: E402
import rot_ref as rr  # noqa: E402
import test_gpu_bounce as tgb  # noqa: E402

DEV = torch.device('cuda')
pytestmark = pytest.mark.gpu

ANGLES = [0., 90., 217.5]
A = len(ANGLES)
RAYS = 4                        # per pixel of the 24 x 24 crop
MATERIAL_KEYS = ('normal_values', 'sg_diffuse_albedo_values', 'sg_roughness_values', 'sg_specular_reflection_values',
                 'points', 'idr_rgb_values', 'network_object_mask', 'object_mask')
# DESIGN.md section 4 documents the default trace schedules as bit-identical however the rays are grouped into calls, and
# the MLP kernels evaluate every row on its own: a frame of the turntable is then the standalone frame bit for bit.
# (False would be a finding for 6i: the masks must still be equal and RGB within the 5e-4 budget line.)
BITWISE = True


@contextlib.contextmanager
def recording(model):
    """the number of rays of every ray_tracer call: a plain wrapper around its forward, taken off again afterwards"""
    rt = model.ray_tracer
    calls = []
    inner = rt.forward

    def forward(*args, **kwargs):
        d = kwargs['ray_directions']
        calls.append(d.shape[0] * d.shape[1])
        return inner(*args, **kwargs)
    rt.forward = forward
    try:
        yield calls
    finally:
        del rt.forward


@pytest.fixture(scope='module')
def scene():
    s = tgb.Scene()
    s.total = s.inp['uv'].shape[1]
    s.n = int(s.hit.sum().item())
    yield s
    s.model.set_envmap_light(None)


def sky_light():
    from nefii_amd.lighting import EnvmapLight
    return EnvmapLight(tgb.sky(), 'mitsuba')


def rotations():
    from nefii_amd.lighting import turntable_rotations
    return turntable_rotations(ANGLES, 'mitsuba')


@contextlib.contextmanager
def replay(scene, uni=None, buni=None):
    m = scene.model
    m.uniforms_override = scene.uni if uni is None else uni
    m.bounce_uniforms_override = scene.buni if buni is None else buni
    try:
        yield
    finally:
        m.uniforms_override, m.bounce_uniforms_override = None, None


def turntable(scene, R, **kw):
    from nefii_amd.training.render import render_turntable
    with replay(scene, **kw):
        return render_turntable(scene.model, scene.inp, scene.total, R)


def frame(scene, **kw):
    from nefii_amd.training.render import render_frame
    with replay(scene, **kw):
        return render_frame(scene.model, scene.inp, scene.total)


def same_frame(what, got, want, keys=None):
    """the rule of the frame comparisons: bit for bit on every key (BITWISE); in any case equal masks and RGB within the
    5e-4 budget line (relative L2)"""
    if keys is None:
        assert sorted(got) == sorted(want)
        keys = sorted(want)
    exact = True
    for k in keys:
        a, b = got[k], want[k]
        if a is None and b is None:
            continue
        same = torch.equal(a, b)
        exact &= same
        if a.dtype == torch.bool:
            assert same, (what, k)
        elif not same:
            rel = ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
            print('%s %s: not bitwise, rel L2 %.3e, max abs %.3e' % (what, k, rel, (a - b).abs().max().item()))
            if 'rgb' in k:
                assert rel <= 5e-4, (what, k, rel)
    print('%s: %s' % (what, 'bitwise equal on %d keys' % len(keys) if exact else 'NOT bitwise'))
    if BITWISE:
        assert exact, what


# ---- what is traced ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['mlp', 'bounce', 'sg'])
def test_ray_counts_per_call(scene, mode):
    """one primary call, ONE secondary call of (2 + A) n rays, and in bounce mode one tertiary call: A (rows 0-1 hits) + the
    row-2 hits of every angle"""
    model = scene.model
    model.set_envmap_light(None if mode == 'sg' else sky_light(), 'mlp' if mode == 'sg' else mode)
    with recording(model) as calls:
        frames = turntable(scene, rotations())
    assert len(frames) == A
    n = scene.n
    assert calls[0] == scene.total and calls[1] == (2 + A) * n, (calls, n)
    assert len(calls) == (3 if mode == 'bounce' else 2), calls
    if mode == 'bounce':
        with replay(scene):
            outs = model.forward_turntable(scene.inp, rotations())
        sec = torch.stack([o['secondary_mask'].reshape(3, n) for o in outs])          # [A, 3, n]
        assert torch.equal(sec[0, :2], sec[1, :2]) and torch.equal(sec[0, :2], sec[2, :2])
        assert calls[2] == int(sec.sum().item()) and calls[2] > 0
    # the standalone frames trace 3 n secondary rays each: 3 A n against (2 + A) n
    with recording(model) as calls:
        frame(scene)
    assert calls[:2] == [scene.total, 3 * n]
    assert 'forward' not in vars(model.ray_tracer)                                     # the wrapper is gone


def test_ray_counts_over_several_chunks(scene):
    """chunks are the outer loop: three chunks of the crop (2^10 rays each) are three primary and three secondary calls"""
    from nefii_amd.training.render import render_turntable
    model = scene.model
    model.set_envmap_light(sky_light(), 'mlp')
    hits = [int(h.sum().item()) for h in torch.split(scene.hit, 1024)]
    with recording(model) as calls:
        torch.manual_seed(5)
        frames = render_turntable(model, scene.inp, scene.total, rotations(), memory_capacity_level=10)
    want = []
    for size, n in zip([1024, 1024, scene.total - 2048], hits):
        want += [size, (2 + A) * n]
    assert calls == want, (calls, want)
    assert all(f['sg_rgb_values'].shape == (scene.total, 3) and torch.isfinite(f['sg_rgb_values']).all() for f in frames)
    assert all(torch.equal(f['network_object_mask'], scene.hit) for f in frames)


# ---- the frames ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['mlp', 'bounce'])
def test_map_light_frames_equal_standalone_renders(scene, mode):
    from nefii_amd.utils import rend_util
    model = scene.model
    light = sky_light()
    R = rotations()
    model.set_envmap_light(light, mode)
    miss_search = model.ray_tracer.miss_search
    from nefii_amd.training.render import render_turntable
    with replay(scene):
        frames = render_turntable(model, scene.inp, scene.total, R)
        # leftovers: the light, its mode, the overrides and the tracer's switch are as they were
        assert model.uniforms_override is scene.uni and model.bounce_uniforms_override is scene.buni
    assert model.envmap_light is light and model.envmap_indirect == mode and light.rotation is None
    assert model.ray_tracer.miss_search == miss_search
    with replay(scene):
        chunk = model.forward_turntable(scene.inp, R)
    assert model.envmap_light is light
    for a in range(A):
        model.set_envmap_light(light.rotated(R[a]), mode)
        same_frame('%s angle %g' % (mode, ANGLES[a]), frames[a], frame(scene))
        with replay(scene), torch.no_grad():
            alone = model(scene.inp)
        same_frame('%s angle %g, chunk' % (mode, ANGLES[a]), chunk[a], alone,
                   keys=['secondary_mask', 'secondary_dir', 'network_object_mask', 'sg_rgb_values',
                         'sg_diffuse_rgb_values', 'sg_specular_rgb_values'])
    # angle 0: the plain frame under the light itself
    model.set_envmap_light(light, mode)
    same_frame('%s angle 0 against render_frame' % mode, frames[0], frame(scene))
    # the frames do differ, the material buffers do not
    assert not torch.equal(frames[0]['sg_rgb_values'], frames[1]['sg_rgb_values'])
    assert not torch.equal(frames[1]['sg_rgb_values'], frames[2]['sg_rgb_values'])
    for a in range(1, A):
        for k in MATERIAL_KEYS:
            assert torch.equal(frames[a][k], frames[0][k]), (a, k)
    # the background: the rotated map's texel along the camera ray
    dirs, _ = rend_util.get_camera_params(scene.inp['uv'], scene.inp['pose'], scene.inp['intrinsics'])
    dirs = dirs.reshape(-1, 3)
    bg = ~scene.hit
    assert bg.any()
    for a in range(A):
        want = light.radiance_rotations(R[a:a + 1], dirs[bg].contiguous())
        assert torch.equal(frames[a]['sg_rgb_values'][bg], want), a
        assert torch.equal(want, light.rotated(R[a]).radiance(dirs[bg]))
    # a second turntable replays the first
    again = turntable(scene, R)
    assert all(torch.equal(x['sg_rgb_values'], y['sg_rgb_values']) for x, y in zip(frames, again))


def test_sg_light_frames_equal_standalone_renders(scene):
    """the model's own SG light: frame a against a standalone render with the lobes rotated by rotate_light_sgs'
    arithmetic (lighting.rotate_light_sgs_matrix of the same fp32 matrix); angle 0 against the plain frame"""
    from nefii_amd.lighting import rotate_light_sgs, rotate_light_sgs_matrix
    model = scene.model
    model.set_envmap_light(None)
    R = rotations()
    net = model.envmap_material_network
    own = net.lgtSGs.data.clone()
    frames = turntable(scene, R)
    assert torch.equal(net.lgtSGs.data, own) and model.envmap_light is None
    # angle 0 - exactly the identity - is the light as it is: the plain frame
    same_frame('sg angle 0 against render_frame', frames[0], frame(scene))
    try:
        for a in range(A):
            net.lgtSGs.data = rotate_light_sgs_matrix(own, R[a])
            if a > 0:
                same_frame('sg angle %g' % ANGLES[a], frames[a], frame(scene))
            else:
                # rotate_light_sgs by 0 degrees normalises the lobe axes and writes |lambda|, |mu|: the same light to
                # rounding, not the same bits
                alone = frame(scene)
                assert torch.equal(alone['network_object_mask'], frames[0]['network_object_mask'])
                rel = ((alone['sg_rgb_values'] - frames[0]['sg_rgb_values']).norm() / alone['sg_rgb_values'].norm()).item()
                print('sg angle 0 against rotate_light_sgs by 0 degrees: rel L2 %.3e' % rel)
                assert rel <= 5e-4
            # the host-side helper the fit script uses gives the same lobes to rounding
            host = rotate_light_sgs(own, [ANGLES[a], 0., 0.], seq='yxz')
            assert torch.allclose(host, net.lgtSGs.data, rtol=0, atol=2e-7)
    finally:
        net.lgtSGs.data = own
    assert not torch.equal(frames[0]['sg_rgb_values'], frames[1]['sg_rgb_values'])
    for a in range(1, A):
        for k in MATERIAL_KEYS:
            assert torch.equal(frames[a][k], frames[0][k]), (a, k)


# ---- a column-aligned yaw against the rolled map -------------------------------------------------------------------------
def test_column_aligned_yaw_equals_the_rolled_map(scene):
    """90 degrees are 32 columns of the 128-column sky: the frame under that yaw against the frame under np.roll of the
    map, unrotated.  "The same uniforms" are the same DRAW: the rolled row's conditional CDF is another prefix sum and
    inverts one number to another texel, so column 5 of the uniforms is mapped through the two tables to the same texel
    and the same offset inside it (fp64 on the host, rounded to fp32 - the direction then moves by about 1e-7 / P(j|i)
    texels); the row (column 4) reads the marginal, which a roll leaves alone up to the order of its fp64 row sums.
    Compared: the rays of pixels none of whose 3 x RAYS sampled directions lie within 1e-5 rad of a texel edge (in either
    map) - at least 90 % of the surface pixels - with equal hit masks and RGB within the 5e-4 budget line."""
    from nefii_amd.lighting import EnvmapLight
    model = scene.model
    env = tgb.sky().numpy()
    H, W = env.shape[:2]
    m = 32
    light = EnvmapLight(torch.from_numpy(env), 'mitsuba')
    rolled = EnvmapLight(torch.from_numpy(np.roll(env, rr.roll_columns(m, 'mitsuba'), axis=1).copy()), 'mitsuba')
    R = rotations()[1:2]
    assert np.abs(R[0].numpy() - rr.yaw(rr.column_yaw_deg(m, W), 'mitsuba')).max() <= 6e-8
    model.set_envmap_light(light, 'mlp')
    with replay(scene):
        got = model.forward_turntable(scene.inp, R)[0]
    # the same draw on the rolled table
    import test_gpu_envlight as tge
    M, C = [x.astype(np.float64) for x in tge.read_table(light.table, H, W)]
    Mr, Cr = [x.astype(np.float64) for x in tge.read_table(rolled.table, H, W)]
    u = scene.uni.cpu().numpy().astype(np.float64)
    i = np.minimum(np.searchsorted(M, u[:, 4], side='right'), H - 1)
    ir = np.minimum(np.searchsorted(Mr, u[:, 4], side='right'), H - 1)
    j = np.array([min(np.searchsorted(C[a], x, side='right'), W - 1) for a, x in zip(i, u[:, 5])])
    prev = np.where(j > 0, C[i, np.maximum(j - 1, 0)], 0.)
    du = np.clip((u[:, 5] - prev) / np.maximum(C[i, j] - prev, 1e-300), 0., 1.)
    jr = (j - m) % W
    prev_r = np.where(jr > 0, Cr[i, np.maximum(jr - 1, 0)], 0.)
    u5 = prev_r + du * (Cr[i, jr] - prev_r)
    uni = scene.uni.clone()
    uni[:, 5] = torch.from_numpy(u5.astype(np.float32)).to(DEV)
    model.set_envmap_light(rolled, 'mlp')
    with replay(scene, uni=uni), torch.no_grad():
        want = model(scene.inp)
    # the pixels to compare
    n = scene.n
    wi = want['secondary_dir'].reshape(3, n, 3).cpu().numpy()
    wr = got['secondary_dir'].reshape(3, n, 3).cpu().numpy()
    clear = np.ones(n, bool)
    for k in range(3):
        clear &= er.edge_distance(wi[k], H, W, 'mitsuba') > 1e-5
        clear &= rr.edge_distance(wr[k], H, W, 'mitsuba', R[0].numpy()) > 1e-5
    clear &= (i == ir)                                    # the marginal's row, on either table
    from nefii_amd.utils import rend_util
    dirs, _ = rend_util.get_camera_params(scene.inp['uv'], scene.inp['pose'], scene.inp['intrinsics'])
    dirs = dirs.reshape(-1, 3).cpu().numpy()
    # background rays: the camera direction itself looks the texel up
    ray_ok = (er.edge_distance(dirs, H, W, 'mitsuba') > 1e-5) & (rr.edge_distance(dirs, H, W, 'mitsuba', R[0].numpy()) > 1e-5)
    ray_ok[scene.hit.cpu().numpy()] = clear
    hit_pix = scene.hit.cpu().numpy().reshape(-1, RAYS).any(1)
    pix_ok = ray_ok.reshape(-1, RAYS).all(1)
    share = (pix_ok & hit_pix).sum() / hit_pix.sum()
    print('pixels compared: %.4f of %d surface pixels' % (share, hit_pix.sum()))
    assert share >= 0.90
    sel = torch.from_numpy(np.repeat(pix_ok, RAYS)).to(DEV)
    hsel = sel[scene.hit]
    assert torch.equal(got['network_object_mask'], want['network_object_mask'])
    sm_a, sm_b = got['secondary_mask'].reshape(3, n)[:, hsel], want['secondary_mask'].reshape(3, n)[:, hsel]
    print('secondary masks that differ: %d of %d' % ((sm_a != sm_b).sum().item(), sm_a.numel()))
    assert torch.equal(sm_a, sm_b)
    dmax = (got['secondary_dir'].reshape(3, n, 3)[:, hsel] - want['secondary_dir'].reshape(3, n, 3)[:, hsel]).abs().max()
    print('max |direction difference| %.3e' % dmax.item())
    for k in ('sg_rgb_values', 'sg_diffuse_rgb_values', 'sg_specular_rgb_values'):
        a, b = got[k][sel], want[k][sel]
        rel = ((a - b).norm() / b.norm()).item()
        print('%s: rel L2 %.3e' % (k, rel))
        assert rel <= 5e-4, (k, rel)
    # background rays see the rolled map's texel, bitwise, away from the edges
    bg = ~scene.hit & torch.from_numpy(ray_ok).to(DEV)
    assert bg.any() and torch.equal(got['sg_rgb_values'][bg], want['sg_rgb_values'][bg])


# ---- the command line ----------------------------------------------------------------------------------------------------
def test_turntable_cli(tmp_path):
    from PIL import Image
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.scripts.vis_rotate_envlight import TurntableRunner
    from nefii_amd.utils import exr
    mc = syn.model_conf('conf', hidden=64)
    cfg = conf.from_dict({'train': {'model_class': 'nefii_amd.model.implicit_differentiable_renderer.IDRNetwork',
                                    'dataset_class': 'nefii_amd.datasets.synthetic_dataset.SyntheticSceneDataset'},
                          'model': mc})
    sd = syn.make_state_dict(mc, seed=0, bumpy=0.02)
    ck = tmp_path / 'scene' / 't0' / 'checkpoints' / 'ModelParameters'
    os.makedirs(str(ck))
    torch.save({'epoch': 1, 'model_state_dict': sd}, str(ck / 'latest.pth'))
    exr.imwrite(str(tmp_path / 'sky.exr'), tgb.br.lognormal_map(24, 48, 8, 1.0))
    kw = dict(conf=cfg, exps_folder_name=str(tmp_path), expname='scene', timestamp='t0', checkpoint='latest',
              memory_capacity_level=10, num_rays=2, dataset_kwargs={'n_views': 2, 'img_res': (16, 16)}, angle_delta=120,
              env_height=16, env_width=32)
    for name, extra in (('map', dict(light_envmap_path=str(tmp_path / 'sky.exr'), envmap_height=12, envmap_width=24)),
                        ('sg', {})):
        out = tmp_path / ('turn_' + name)
        written = TurntableRunner(plots_dir=str(out), new_timestamp='run_' + name, **dict(kw, **extra)).run()
        assert written == [0, 1]
        want = ['%d-%s-%d.png' % (i, kind, a) for i in (0, 1) for a in (0, 120, 240) for kind in ('render', 'material', 'env')]
        want += ['%d-gt_rgb-0.png' % i for i in (0, 1)]
        assert sorted(os.listdir(str(out))) == sorted(want)
        png = lambda f: np.asarray(Image.open(str(out / f)))
        for i in (0, 1):
            for a in (0, 120, 240):
                assert png('%d-render-%d.png' % (i, a)).shape == (16, 16, 3)
                assert png('%d-material-%d.png' % (i, a)).shape == (16, 64, 3)
                assert png('%d-env-%d.png' % (i, a)).shape == (16, 32, 3)
            assert png('%d-gt_rgb-0.png' % i).shape == (16, 16, 3)
            assert not np.array_equal(png('%d-env-0.png' % i), png('%d-env-120.png' % i))
            assert not np.array_equal(png('%d-render-0.png' % i), png('%d-render-120.png' % i))
            # the material buffers do not turn with the light: normal | albedo are the first two panels
            assert np.array_equal(png('%d-material-0.png' % i)[:, :32], png('%d-material-120.png' % i)[:, :32])
    with pytest.raises(ValueError):
        TurntableRunner(plots_dir=str(tmp_path / 'bad'), new_timestamp='bad', **dict(kw, angle_delta=7))
