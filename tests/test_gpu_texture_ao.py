"""The ambient-occlusion bake on the GPU (csrc/nefii_texbake.hip, nefii_amd/texture.py) against the numpy
restatement of tests/texbake_ao_ref.py: the ray kernel's uniforms bit for bit, its origins and directions to fp32 rounding, the
accumulate kernel's occlusion exactly and its bent normal to one fp32 ulp; then a whole bake of the fitted bowl - convex outside,
concave inside - its rays against the CPU oracle tracer, and the command line.  Budget: a few seconds per test."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import texbake_ao_ref as ref  # noqa: E402
import texbake_ref  # noqa: E402

DEV = torch.device('cuda:0')
AXIS = np.array([0.0, 0.55, 0.835]) / np.linalg.norm([0.0, 0.55, 0.835])      # the bowl's axis: its opening faces along it


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ray_inputs(m, seed):
    rng = np.random.default_rng(seed)
    pos = (rng.random((m, 3)) * 1.8 - 0.9).astype(np.float32)
    normal = ref.unit_normals(m, rng)
    sdf = rng.normal(0.0, 5e-3, size=m).astype(np.float32)
    gnorm = rng.uniform(0.5, 1.5, size=m).astype(np.float32)
    texel = rng.integers(0, 2 ** 26, size=m).astype(np.int64)
    return pos, normal, sdf, gnorm, texel


# ---- the ray kernel against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 2, 33, 64])
@pytest.mark.parametrize('m', [1, 63, 64, 65, 1000])
def test_ray_kernel_matches_the_reference(m, K):
    """Measured on an MI355X over all 20 cases: directions within 4.0e-7 of the fp64 restatement (bound 3e-6: phi carries under
    one ulp of 2 pi, 7.5e-7; sinf / cosf 2 ulp; the rotation 3 ulp; the normalisation 2 ulp), origins and uniforms bit for bit,
    | |d| - 1 | <= 1.6e-7, d.n >= 1.7e-3."""
    from nefii_amd import ops
    seed, bias = 7 + K, 3e-3
    pos, normal, sdf, gnorm, texel = ray_inputs(m, 100 * K + m)
    args = [gpu(a) for a in (pos, normal, sdf, gnorm, texel)]
    origins, dirs, uniforms = ops.bake_ao_rays(*args, K, seed, bias, want_uniforms=True)
    assert origins.shape == (m, 3) and dirs.shape == (K, m, 3) and uniforms.shape == (K, m, 2)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (origins, dirs, uniforms))
    o, d, u = origins.cpu().numpy(), dirs.cpu().numpy(), uniforms.cpu().numpy()
    w_u = ref.uniforms(texel, K, seed)
    assert np.array_equal(u.view(np.uint32), w_u.view(np.uint32))                                      # bit for bit
    w_o = ref.origins(pos, normal, sdf, gnorm, bias).astype(np.float64)
    o_err = np.abs(o.astype(np.float64) - w_o)
    assert (o_err <= 2.0 ** -23 * np.maximum(1.0, np.abs(w_o))).all()
    w_d = ref.directions(w_u, normal)
    d_err = np.abs(d.astype(np.float64) - w_d).max()
    length = np.abs(np.linalg.norm(d.astype(np.float64), axis=2) - 1.0).max()
    cos = (d.astype(np.float64) * normal[None].astype(np.float64)).sum(2)
    print('m = %d, K = %d: max |dir - reference| %.3e (bound 3e-6), max |origin - reference| %.3e, max ||d| - 1| %.3e, '
          'min d.n %.3e' % (m, K, d_err, o_err.max(), length, cos.min()))
    assert d_err <= 3e-6
    assert length <= 2e-6
    assert (cos > 0.0).all()
    # without the uniforms: the same rays
    o2, d2, none = ops.bake_ao_rays(*args, K, seed, bias)
    assert none is None and torch.equal(o2, origins) and torch.equal(d2, dirs)
    # in two calls that split the texels mid-range: bitwise the one-call result
    if m > 1:
        cut = m // 3 + 1
        a = ops.bake_ao_rays(*(t[:cut].contiguous() for t in args), K, seed, bias, want_uniforms=True)
        b = ops.bake_ao_rays(*(t[cut:].contiguous() for t in args), K, seed, bias, want_uniforms=True)
        assert torch.equal(torch.cat([a[0], b[0]]), origins)
        assert torch.equal(torch.cat([a[1], b[1]], 1), dirs) and torch.equal(torch.cat([a[2], b[2]], 1), uniforms)
    # another seed turns every texel's sequence
    assert not torch.equal(ops.bake_ao_rays(*args, K, seed + 1, bias)[1], dirs)


# ---- the accumulate kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [1, 33, 64])
@pytest.mark.parametrize('m', [1, 65, 1000])
def test_accumulate_kernel_matches_the_reference(m, K):
    """Measured on an MI355X: ao equal in all 18 runs, bent within 3.0e-8 of the fp64 restatement (bound 2^-23 = 1.19e-7)."""
    from nefii_amd import ops
    D = 0.3
    rng = np.random.default_rng(1000 * K + m)
    pos, normal, _, _, texel = ray_inputs(m, K + m)
    dirs = ref.directions(ref.uniforms(texel, K, 5), normal).astype(np.float32)
    hit = rng.random((K, m)) < 0.5
    near = rng.random((K, m)) < 0.5
    if m > 1:
        hit[:, 1], near[:, 1] = True, True                             # every ray occluded, whatever the distance
        hit[:, 2] = False                                              # every ray free
    else:
        hit[:], near[:] = True, True
    reach = np.where(near, np.float32(0.5 * D), np.float32(2.0 * D)).astype(np.float32)
    pts = pos[None] + reach[..., None] * dirs                          # 0.5 D or 2 D from the origin: none on the threshold
    pts[~hit] = np.nan                                                 # the point of a miss is unspecified: never looked at
    g = [gpu(a) for a in (hit, pts, pos, dirs, normal)]
    for distance in (D, 0.0):
        ao, bent = ops.bake_ao_accumulate(*g, distance)
        assert ao.shape == (m,) and bent.shape == (m, 3) and ao.dtype == torch.float32 and bent.dtype == torch.float32
        w_ao, w_bent, occluded = ref.accumulate(hit, pts, pos, dirs, normal, distance)
        assert np.array_equal(occluded, hit & near if distance > 0 else hit)
        assert np.array_equal(ao.cpu().numpy(), w_ao)                                                  # exactly
        err = np.abs(bent.cpu().numpy().astype(np.float64) - w_bent).max()
        print('m = %d, K = %d, distance %g: ao equal, max |bent - reference| %.3e (bound %.3e)' % (m, K, distance, err, 2.0 ** -23))
        assert err <= 2.0 ** -23
        col = 1 if m > 1 else 0
        assert ao[col].item() == 0.0 and torch.equal(bent[col].cpu(), torch.from_numpy(normal[col]))   # all occluded: the normal
        if m > 1:
            assert ao[2].item() == 1.0
    # a uint8 mask is the bool mask
    ao8, bent8 = ops.bake_ao_accumulate(g[0].view(torch.uint8), *g[1:], 0.0)
    assert torch.equal(ao8, ao) and torch.equal(bent8, bent)


def test_kernels_refuse_before_anything_is_enqueued():
    from nefii_amd import _lib, ops
    lib = _lib.lib()
    m, K = 65, 4
    pos, normal, sdf, gnorm, texel = (gpu(a) for a in ray_inputs(m, 3))
    origins = torch.full((m, 3), 7.0, device=DEV)
    dirs = torch.full((1025, m, 3), 7.0, device=DEV)
    ao, bent = torch.full((m,), 7.0, device=DEV), torch.full((m, 3), 7.0, device=DEV)
    hit, pts = torch.ones(1025, m, dtype=torch.uint8, device=DEV), torch.zeros(1025, m, 3, device=DEV)
    p = lambda t: t.data_ptr()                                                                    # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    for bad_K, status in ((0, -2), (1025, -2)):
        assert lib.nefii_bake_ao_rays(p(pos), p(normal), p(sdf), p(gnorm), p(texel), m, bad_K, 0, 0.0, p(origins), p(dirs), None,
                                      stream) == status
        assert lib.nefii_bake_ao_accumulate(p(hit), p(pts), p(origins), p(dirs), p(normal), m, bad_K, 0.0, p(ao), p(bent),
                                            stream) == status
    assert lib.nefii_bake_ao_rays(p(pos), p(normal), None, p(gnorm), p(texel), m, K, 0, 0.0, p(origins), p(dirs), None, stream) == -1
    assert lib.nefii_bake_ao_accumulate(None, p(pts), p(origins), p(dirs), p(normal), m, K, 0.0, p(ao), p(bent), stream) == -1
    torch.cuda.synchronize()
    for t in (origins, dirs, ao, bent):                                # nothing was written
        assert bool((t == 7.0).all())
    for bad_K in (0, 1025):
        with pytest.raises(ValueError, match='rays'):
            ops.bake_ao_rays(pos, normal, sdf, gnorm, texel, bad_K)
    with pytest.raises(ValueError):
        ops.bake_ao_accumulate(hit, pts, origins, dirs[:1025], normal)
    with pytest.raises(ValueError):
        ops.bake_ao_rays(pos, normal, sdf[:5], gnorm, texel, K)
    o, d, _ = ops.bake_ao_rays(pos, normal, sdf, gnorm, texel, K)                                 # the next call is served as ever
    assert torch.isfinite(d).all() and ops.bake_ao_rays(pos[:0], normal[:0], sdf[:0], gnorm[:0], texel[:0], K)[1].shape == (K, 0, 3)


# ---- a whole bake of the fitted bowl -----------------------------------------------------------------------------------------
def scene_model(scene, model_name):
    from nefii_amd import conf, synthetic as syn
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    mc = syn.model_conf(model_name)
    sd = syn.make_state_dict(mc, seed=0, scene=scene)
    model = IDRNetwork(conf.from_dict(mc))
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV)
    model.freeze_geometry()
    model.eval()
    return model, mc, sd


@pytest.fixture(scope='module')
def bowl():
    """the recipe of test_gpu_texture.py's fixture, and one occlusion bake of 32 rays that the tests below share"""
    from nefii_amd import texture
    from nefii_amd.mesh import extract_mesh
    model, mc, sd = scene_model('bowl_trained', 'conf')
    m = extract_mesh(model, resolution=96, keep='largest', simplify=4)
    size = 12 * texbake_ref.atlas(m.faces.shape[0], 8192)['n']      # the smallest size with cells of 12 texels
    baked = texture.bake_textures(model, m, size)
    occ = texture.bake_occlusion(model, m, baked, rays=32)
    return dict(model=model, mc=mc, sd=sd, mesh=m, size=size, baked=baked, occ=occ)


def shells(baked):
    """(outer, inner) masks [T,T] of the covered texels on the bowl's outer and inner shell, away from the rim"""
    pos = baked.position.double()
    radius = pos.norm(dim=2)
    below = (pos * torch.from_numpy(AXIS).to(DEV)).sum(2) < -0.25
    return baked.covered & below & (radius > 0.64), baked.covered & below & (radius > 0.55) & (radius < 0.60)


def test_bake_of_the_fitted_bowl_separates_the_shells(bowl):
    """Measured on an MI355X: 2526 faces, 181 872 owned texels, 5.82e6 rays in 0.96 s; mean ao 1.0000 over 13 374 covered
    texels of the outer shell, 0.2652 over 10 807 of the inner one (the CPU oracle tracer gave 1.000 and 0.358 at 48 points
    each, which set the bounds asserted here), 0.6618 over all covered texels."""
    baked, occ = bowl['baked'], bowl['occ']
    T = bowl['size']
    assert occ.ao.shape == (T, T) and occ.bent_normal.shape == (T, T, 3)
    assert occ.ao.dtype == torch.float32 and occ.bent_normal.dtype == torch.float32 and occ.ao.is_cuda and occ.bent_normal.is_cuda
    unowned = baked.owner < 0
    assert unowned.any() and not occ.ao[unowned].any() and not occ.bent_normal[unowned].any()
    meta = occ.meta
    assert sorted(meta) == sorted(['rays', 'distance', 'bias', 'seed', 'traced_rays', 'off_surface_texels', 'ao_s',
                                   'mean_ao_covered'])
    assert (meta['rays'], meta['distance'], meta['bias'], meta['seed']) == (32, None, 0.0, 0)
    assert meta['traced_rays'] == 32 * baked.meta['owned_texels'] and meta['ao_s'] > 0
    assert sorted(baked.meta) == sorted(['size', 'cell', 'leg', 'pad', 'owned_texels', 'covered_texels', 'project', 'bake_s',
                                         'raster_s', 'network_s'])                                # the material bake's keys stay
    owned = ~unowned
    ao = occ.ao[owned]
    assert ao.min() >= 0.0 and ao.max() <= 1.0 and bool((ao * 32 == (ao * 32).round()).all())     # multiples of 1 / 32
    assert (occ.bent_normal[owned].norm(dim=1) - 1.0).abs().max().item() < 1e-6
    assert abs(meta['mean_ao_covered'] - occ.ao[baked.covered].double().mean().item()) < 1e-12
    outer, inner = shells(baked)
    n_outer, n_inner = int(outer.sum()), int(inner.sum())
    ao_outer, ao_inner = occ.ao[outer].double().mean().item(), occ.ao[inner].double().mean().item()
    print('bowl, %d faces, %d^2: %d owned texels, %d rays in %.4f s (%.3g rays/s); mean ao %.4f over %d covered texels of the outer '
          'shell, %.4f over %d of the inner shell, %.4f over all covered; %d texels off the surface' % (
              bowl['mesh'].faces.shape[0], T, baked.meta['owned_texels'], meta['traced_rays'], meta['ao_s'],
              meta['traced_rays'] / meta['ao_s'], ao_outer, n_outer, ao_inner, n_inner, meta['mean_ao_covered'],
              meta['off_surface_texels']))
    assert n_outer > 1000 and n_inner > 1000
    assert ao_outer >= 0.98
    assert 0.2 <= ao_inner <= 0.55
    # on the open outer shell the bent normal is the normal up to the sampling of 32 directions: independent cosine-weighted
    # draws sum to (2 / 3) 32 along the normal and sqrt(32 / 4) across it per axis, a mean cosine of 0.982; the bound leaves
    # twice that angle's variance
    cos_outer = (occ.bent_normal[outer] * baked.normal[outer]).sum(1).mean().item()
    print('mean cosine between bent normal and normal on the outer shell %.5f' % cos_outer)
    assert cos_outer > 0.96


def test_a_second_bake_and_a_bake_in_chunks_give_the_same_bits(bowl):
    from nefii_amd import texture
    model, m, baked, occ = (bowl[k] for k in ('model', 'mesh', 'baked', 'occ'))
    again = texture.bake_occlusion(model, m, baked, rays=32)
    assert torch.equal(again.ao, occ.ao) and torch.equal(again.bent_normal, occ.bent_normal)
    parts = texture.bake_occlusion(model, m, baked, rays=32, ray_chunk=32 * 1000)
    assert baked.meta['owned_texels'] > 3000 and baked.meta['owned_texels'] % 1000 != 0
    assert torch.equal(parts.ao, occ.ao) and torch.equal(parts.bent_normal, occ.bent_normal)
    assert parts.meta['traced_rays'] == occ.meta['traced_rays']


def test_distance_seed_encoding_and_report(bowl):
    """Measured on an MI355X: covered means 0.66183 (seed 0), 0.66191 (seed 1), 0.93877 with distance 0.1; verify_occlusion at
    500 points with 64 rays: mean |lookup - estimate| 0.0233 beside a noise floor of 0.0352 for the bake's 32 rays."""
    from nefii_amd import texture
    model, m, baked, occ = (bowl[k] for k in ('model', 'mesh', 'baked', 'occ'))
    near = texture.bake_occlusion(model, m, baked, rays=32, distance=0.1)
    assert near.meta['distance'] == 0.1 and bool((near.ao >= occ.ao).all()) and bool((near.ao > occ.ao).any())
    other = texture.bake_occlusion(model, m, baked, rays=32, seed=1)
    diff = abs(other.meta['mean_ao_covered'] - occ.meta['mean_ao_covered'])
    print('seed 0 / 1: covered means %.5f / %.5f; distance 0.1: covered mean %.5f' % (
        occ.meta['mean_ao_covered'], other.meta['mean_ao_covered'], near.meta['mean_ao_covered']))
    assert other.meta['seed'] == 1 and not torch.equal(other.ao, occ.ao) and diff < 0.02
    enc = texture.encode_occlusion(baked, occ)
    T = bowl['size']
    assert enc['ao'].shape == (T, T) and enc['bent_normal'].shape == (T, T, 4) and enc['orm'].shape == (T, T, 4)
    assert all(v.dtype == torch.uint8 for v in enc.values())
    owned = baked.owner >= 0
    want = (255.0 * occ.ao.double() + 0.5).floor().to(torch.uint8)
    assert torch.equal(enc['ao'], want) and torch.equal(enc['orm'][..., 0], enc['ao'])
    assert torch.equal(enc['orm'][..., 1], texture.encode_textures(baked)['roughness']) and not enc['orm'][..., 2].any()
    assert torch.equal(enc['orm'][..., 3] == 255, owned) and not enc['orm'][~owned].any()
    report = texture.verify_occlusion(model, m, baked, occ, 500, rays=64)
    print(json.dumps(report))
    assert report['samples'] == 500 and report['bake_rays'] == 32 and 0.0 <= report['ao_mean'] <= report['ao_max'] <= 1.0
    assert report['noise_floor'] > report['verify_noise_floor'] > 0.0


def test_rays_of_the_bake_against_the_oracle_tracer(bowl):
    """24 covered texels of a bake with 16 rays: the kernel's own 384 rays through oracle/tracer.py (fp32, eval mode) on the
    CPU.  Measured on an MI355X: 0 of 384 hit masks flipped."""
    from nefii_amd import ops, texture
    from nefii_amd.model.path_tracing_render import trace_occluders
    from oracle import nets, tracer
    model, mc, sd, m, baked = (bowl[k] for k in ('model', 'mc', 'sd', 'mesh', 'baked'))
    K = 16
    occ = texture.bake_occlusion(model, m, baked, rays=K)
    cov = baked.covered.reshape(-1).nonzero()[:, 0]
    idx = cov[torch.randperm(cov.shape[0], generator=torch.Generator().manual_seed(0))[:24].to(DEV)].sort()[0]
    x = baked.position.reshape(-1, 3)[idx].contiguous()
    normal = baked.normal.reshape(-1, 3)[idx].contiguous()
    with torch.no_grad():
        sdf, _, g = model.implicit_network.value_feature_gradient(x)
        origins, dirs, _ = ops.bake_ao_rays(x, normal, sdf.reshape(-1).contiguous(), g.norm(dim=1), idx, K)
        o = origins.unsqueeze(0).expand(K, 24, 3).reshape(-1, 3).contiguous()
        pts, hit = trace_occluders(o, dirs, model)
    field = lambda y: nets.sdf_forward(sd, mc['implicit_network'], y)[:, 0]                          # noqa: E731
    want = tracer.trace(field, o.cpu(), dirs.reshape(-1, 3).cpu(), torch.ones(K * 24, dtype=torch.bool), mc['ray_tracer'], False)
    flips = (hit.cpu() != want['hit']).view(K, 24)
    n_flips = int(flips.sum())
    print('[ao rays] %d rays of %d texels, hit-mask flips vs the oracle tracer %d; %d hits' % (K * 24, 24, n_flips, int(hit.sum())))
    assert n_flips <= max(1, int(0.004 * K * 24))
    assert 0 < int(want['hit'].sum()) < K * 24
    w_ao, _, _ = ref.accumulate(want['hit'].view(K, 24).numpy(), want['points'].view(K, 24, 3).numpy(), origins.cpu().numpy(),
                                dirs.cpu().numpy(), normal.cpu().numpy(), 0.0)
    got = occ.ao.reshape(-1)[idx].cpu().numpy()
    flipped = flips.any(0).numpy()
    assert np.array_equal(got[~flipped], w_ao[~flipped])
    assert (np.abs(got[flipped] - w_ao[flipped]) <= 1.0 / K).all()


# ---- the command line --------------------------------------------------------------------------------------------------------
def _hocon(d):
    out = []
    for k, v in d.items():
        if isinstance(v, dict):
            out.append('%s { %s }' % (k, _hocon(v)))
        elif isinstance(v, (list, tuple)):
            out.append('%s = [%s]' % (k, ', '.join(str(x) for x in v)))
        elif isinstance(v, bool):
            out.append('%s = %s' % (k, 'True' if v else 'False'))
        else:
            out.append('%s = %s' % (k, v))
    return '\n'.join(out)


def test_cli_end_to_end(tmp_path):
    from PIL import Image
    from nefii_amd import synthetic as syn
    from nefii_amd.utils.obj import read_mtl
    mc = syn.model_conf('conf')
    sd = syn.make_state_dict(mc, seed=0, scene='bowl_trained')
    conf_path = tmp_path / 'run.conf'
    conf_path.write_text('train {\n model_class = model.implicit_differentiable_renderer.IDRNetwork\n}\nmodel { %s }\n' % _hocon(mc))
    ck = tmp_path / 'exps' / 'bowl' / '2026_01_01_00_00_00' / 'checkpoints' / 'ModelParameters'
    ck.mkdir(parents=True)
    torch.save({'epoch': 7, 'model_state_dict': sd}, str(ck / 'latest.pth'))
    base = [sys.executable, '-m', 'nefii_amd.scripts.extract_mesh', '--conf', str(conf_path), '--resolution', '96', '--expname',
            'bowl', '--exps_folder_name', str(tmp_path / 'exps'), '--texture', '432', '--simplify', '4', '--keep', 'largest']
    (tmp_path / 'a').mkdir()
    (tmp_path / 'b').mkdir()
    r = subprocess.run(base + ['--out', str(tmp_path / 'a' / 'bowl.ply'), '--texture_ao', '16', '--texture_orm',
                               '--texture_bent_normal', '--verify_ao', '500'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    plain = subprocess.run(base + ['--out', str(tmp_path / 'b' / 'bowl.ply')], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    old = ['bowl.mtl', 'bowl.obj', 'bowl.ply', 'bowl_albedo.png', 'bowl_normal.png', 'bowl_roughness.png']
    assert sorted(os.listdir(tmp_path / 'b')) == old
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(old + ['bowl_ao.png', 'bowl_bent_normal.png', 'bowl_orm.png'])
    # without --texture_ao every file is what it was: the occlusion run adds files and two lines to the MTL, no more
    for name in old:
        if name != 'bowl.mtl':
            assert (tmp_path / 'a' / name).read_bytes() == (tmp_path / 'b' / name).read_bytes(), name
    mtl_a, mtl_b = (tmp_path / 'a' / 'bowl.mtl').read_text(), (tmp_path / 'b' / 'bowl.mtl').read_text()
    assert mtl_a.startswith(mtl_b) and mtl_a[len(mtl_b):].splitlines()[-1] == 'map_Ka bowl_ao.png' and 'map_Ka' not in mtl_b
    assert len(mtl_b.splitlines()) == 8 and mtl_b.splitlines()[2:5] == ['newmtl baked', 'Kd 1 1 1', 'map_Kd bowl_albedo.png']
    assert read_mtl(str(tmp_path / 'a' / 'bowl.mtl'))['map_Ka'] == 'bowl_ao.png'
    images = {}
    for k in ('ao', 'bent_normal', 'orm', 'roughness', 'albedo'):
        with Image.open(str(tmp_path / 'a' / ('bowl_%s.png' % k))) as im:
            images[k] = np.array(im)
    assert images['ao'].shape == (432, 432) and images['bent_normal'].shape == (432, 432, 4) and images['orm'].shape == (432, 432, 4)
    assert np.array_equal(images['orm'][..., 1], images['roughness']) and np.array_equal(images['orm'][..., 0], images['ao'])
    assert not images['orm'][..., 2].any() and np.array_equal(images['orm'][..., 3], images['albedo'][..., 3])
    assert images['ao'].max() == 255 and (images['ao'][images['albedo'][..., 3] == 255] < 128).any()    # open outside, shut inside
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    print(lines[0])
    print([ln for ln in r.stdout.splitlines() if 'ambient occlusion' in ln][0])
    assert rec['samples'] == 500 and rec['size'] == 432 and rec['bake_rays'] == 16 and 0.0 <= rec['ao_mean'] <= rec['ao_max'] <= 1.0
