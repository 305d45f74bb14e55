"""The shared first stage of the staged min-SDF search (csrc/nefii_tracer.hip: minsdf_share / shared_walk) on
the GPU, through nefii_trace_rays: a ray whose wave holds a finished search of the same row of draws takes its bounds from that
ray's evaluated depths - through the slope bound L, used sideways - instead of evaluating a first stage of its own.  While L
holds nothing but the number of single-pass evaluations may change: points, hit mask and depths are bit-identical with the
sharing (NEFII_MINSDF_SHARE=1, the default), without it (=0) and without the staging (minsdf_lipschitz = 0)."""
import functools

import pytest
import torch

from nefii_amd import _lib, ops, synthetic as syn
from trace_cmp import build_sdf

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
CAM = (0.2, 0.1, 2.0)


@functools.lru_cache(maxsize=None)
def _net(case):
    """(model conf, packed SDF, tau, largest |grad sdf| found) of the 512-wide trained bowl / of tracer_bumpy_h512's net"""
    if case == 'bowl':
        mc = syn.model_conf('conf')
        sd = syn.make_state_dict(mc, seed=2, scene='bowl_trained')
    else:
        mc = syn.model_conf('physg', hidden=512)
        sd = syn.make_state_dict(mc, seed=0, bumpy=0.004)
    pm = build_sdf(mc, sd, f16x3=True)
    pm32 = build_sdf(mc, sd)
    tau = ops.calibrate_coarse_tau(pm)
    gmax = ops.calibrate_lipschitz(lambda x: ops.sdf_value_grad(pm32, x)[2], DEV, safety=1.0)
    return mc, pm, tau, gmax


def _pixels(n_pixels, seed, radii=(0.62, 0.8, 0.92), jitter=0.003):
    """64 jittered rays from one camera through each of n_pixels points of the plane through the origin that faces it: a few
    millimetres apart at equal depth, as the sub-pixel rays of one pixel are.  The points lie off the object (both test
    geometries end inside radius 0.6) and inside the bounding sphere: rays that miss, i.e. that run the min-SDF search."""
    g = torch.Generator().manual_seed(seed)
    cam = torch.tensor(CAM)
    z = -cam / cam.norm()
    x = torch.linalg.cross(z, torch.tensor([0.0, 1.0, 0.0]))
    x = x / x.norm()
    y = torch.linalg.cross(z, x)
    o, d = [], []
    for k in range(n_pixels):
        ang = 6.2831853 * torch.rand(1, generator=g).item()
        tgt = radii[k % len(radii)] * (torch.cos(torch.tensor(ang)) * x + torch.sin(torch.tensor(ang)) * y)
        jit = (torch.rand(64, 2, generator=g) - 0.5) * 2.0 * jitter
        dd = tgt[None] + jit[:, :1] * x[None] + jit[:, 1:] * y[None] - cam[None]
        o.append(cam[None].expand(64, 3))
        d.append(dd / dd.norm(dim=1, keepdim=True))
    return torch.cat(o), torch.cat(d)


def _random(n, seed, spread=0.6):
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(n, 3, generator=g)
    o = o / o.norm(dim=-1, keepdim=True) * (1.5 + torch.rand(n, 1, generator=g))
    d = torch.randn(n, 3, generator=g) * spread - o
    return o, d / d.norm(dim=-1, keepdim=True)


def _cases():
    """name -> (origins, dirs, object mask, rows of draws, minsdf_group, are these pixel bundles)"""
    g = torch.Generator().manual_seed(77)
    steps = torch.rand(100, generator=g)
    po, pd = _pixels(3, 5)
    ro, rd = _random(229, 6)
    bundle = (torch.cat([po, ro[:37]]), torch.cat([pd, rd[:37]]))         # 3 waves of one pixel each + a wave with 27 dead lanes
    n = bundle[0].shape[0]
    ones = torch.ones(n, dtype=torch.bool)
    return {
        'pixels+37': (*bundle, ones, steps, 0, True),
        'random229': (ro, rd, torch.ones(229, dtype=torch.bool), steps, 0, False),
        'copies64': (po[:1].expand(64, 3).contiguous(), pd[:1].expand(64, 3).contiguous(), torch.ones(64, dtype=torch.bool),
                     steps, 0, True),
        'mixed-mask': (*bundle, torch.rand(n, generator=g) < 0.5, steps, 0, True),
        # one row of draws per 100 rays: the second and the fourth wave hold rays of two rows, which share nothing
        'group100': (*bundle, ones, torch.rand(3, 100, generator=g).reshape(-1), 100, True),
    }


def _trace(mc, pm, case, tau, lip, tier, kept=None):
    o, d, om, steps, group, _ = case
    tp = ops.make_tracer_params(mc['ray_tracer'], True, 'f16x3w', coarse_tau=tau, minsdf_lipschitz=lip, trace_tier=tier,
                                minsdf_group=group)
    lin = torch.linspace(0, 1, steps=tp.n_steps).to(DEV)
    return ops.trace_rays(pm, tp, o.to(DEV).contiguous(), d.to(DEV).contiguous(), om.to(DEV), lin, steps.to(DEV),
                          want_counters=True, keep_workspace=kept)


def _flags(kept):
    """the rays' flag words of a finished trace (they follow the workspace's float arrays, as ops.trace_iterations reads them)"""
    out = []
    for ws, _lo, n in kept:
        stride = (4 * n + 255) // 256 * 256
        begin = _lib.TRACE_WS_FLOAT_ARRAYS * stride
        out.append(ws[begin:begin + 4 * n].view(torch.int32))
    return torch.cat(out)


@pytest.mark.parametrize('net', ['bowl', 'bumpy'])
def test_shared_first_stage_changes_no_output(net, monkeypatch):
    mc, pm, tau, gmax = _net(net)
    for name, case in _cases().items():
        for tier in (0, 1):
            monkeypatch.setenv('NEFII_MINSDF_SHARE', '1')
            plain = _trace(mc, pm, case, tau, 0.0, tier)
            cp = plain[3].cpu().long()
            assert cp[:, _lib.CNT_COARSE_SAMPLES].sum() == 0
            for f in (1.0, 1.5):
                got = {}
                for share in ('0', '1'):
                    monkeypatch.setenv('NEFII_MINSDF_SHARE', share)
                    kept = []
                    got[share] = _trace(mc, pm, case, tau, f * gmax, tier, kept)
                    what = (net, name, tier, f, share)
                    for k, out in enumerate(('points', 'hit mask', 'depths')):
                        assert torch.equal(got[share][k], plain[k]), (what, out)
                    # every ray is done when nefii_trace_max_rounds rounds have run: nobody is left waiting for a donor
                    assert ((_flags(kept) & 7) == 0).all(), what
                c0, c1 = got['0'][3].cpu().long(), got['1'][3].cpu().long()
                for c in (c0, c1):
                    assert c[:, _lib.CNT_LIP_AUDIT].max() == 0, (net, name, tier, f)
                    assert ops.algorithmic_evals(c, 100).sum() == ops.algorithmic_evals(cp, 100).sum()
                    assert c[:, _lib.CNT_SEARCHES].sum() == cp[:, _lib.CNT_SEARCHES].sum()
                e0, e1 = ops.executed_evals(c0, 100)[1].sum().item(), ops.executed_evals(c1, 100)[1].sum().item()
                print('[minsdf share %s %s tier=%d L %.2f x] %d searches: single-pass evaluations %d unstaged, %d staged, %d shared; '
                      'probes %d -> %d' % (net, name, tier, f, cp[:, _lib.CNT_SEARCHES].sum().item(),
                                           ops.executed_evals(cp, 100)[1].sum().item(), e0, e1,
                                           c0[:, _lib.CNT_PROBES].sum().item(), c1[:, _lib.CNT_PROBES].sum().item()))
                assert c0[:, _lib.CNT_COARSE_SAMPLES].sum() > 0, 'no min-SDF search ran: the case checks nothing'
                assert e1 <= e0, (net, name, tier, f, e1, e0)
                if case[5]:
                    assert e1 < e0, (net, name, tier, f, e1, e0)


def test_shared_first_stage_audit_fires_on_a_false_claim(monkeypatch):
    """A claimed L of 0.05, far below the slope: depths evaluated lie below the bounds they were given - also the sideways
    ones - and the audit column says so, as it does without the sharing."""
    mc, pm, tau, gmax = _net('bowl')
    monkeypatch.setenv('NEFII_MINSDF_SHARE', '1')
    for name in ('pixels+37', 'random229'):
        bad = _trace(mc, pm, _cases()[name], tau, 0.05, 0)
        viol = bad[3][:, _lib.CNT_LIP_AUDIT].cpu().contiguous().view(torch.float32).max().item()
        print('[minsdf share %s] claimed L 0.05 (largest gradient seen %.2f): largest violation %.3e' % (name, gmax, viol))
        assert viol > 0.0


def test_shared_first_stage_on_a_dent(monkeypatch):
    """syn.add_sdf_dent: a steep pocket of radius 0.01 just off the surface, bundles of rays grazing through it.  With an L that
    covers the pocket's slope the outputs are bit-identical; what the calibrated L (which does not find the pocket) gives is
    printed, not asserted (DESIGN section 4 records it)."""
    from test_gpu_kernels import _dent_scene
    mc, sd, c = _dent_scene(value_scale=1.0)
    pm, pm32 = build_sdf(mc, sd, f16x3=True), build_sdf(mc, sd)
    tau = ops.calibrate_coarse_tau(pm)
    floor = ops.calibrate_lipschitz(lambda x: ops.sdf_value_grad(pm32, x)[2], DEV)
    cd = c.to(DEV)
    box = cd[None] + (torch.rand(20000, 3, device=DEV, generator=torch.Generator(DEV).manual_seed(3)) - 0.5) * 0.02
    steep = ops.sdf_value_grad(pm32, box)[2].norm(dim=1).max().item()
    # rays across the pocket, at right angles to the direction from the origin, along the one heading of those tried on the
    # CPU on which they pass the bowl without touching it: their lowest SDF value, 0.01 - 0.02, lies in the pocket
    g = torch.Generator().manual_seed(8)
    t = torch.linalg.cross(c, torch.tensor([0.0, 1.0, 1.0]))
    t = t / t.norm()
    o = (c - 2.0 * t)[None].expand(256, 3).contiguous()
    d = c[None] + torch.randn(256, 3, generator=g) * 0.003 - o
    d = d / d.norm(dim=1, keepdim=True)
    case = (o, d, torch.ones(256, dtype=torch.bool), torch.rand(100, generator=g), 0, True)
    monkeypatch.setenv('NEFII_MINSDF_SHARE', '1')
    plain = _trace(mc, pm, case, tau, 0.0, 0)
    assert not plain[1].any() and plain[3][:, _lib.CNT_SEARCHES].sum() == 256, 'the rays were to miss and search'
    for what, lip in (('covering', 1.5 * max(steep, floor)), ('calibrated', floor)):
        res = {}
        for share in ('0', '1'):
            monkeypatch.setenv('NEFII_MINSDF_SHARE', share)
            got = _trace(mc, pm, case, tau, lip, 0)
            c_ = got[3].cpu().long()
            viol = c_[:, _lib.CNT_LIP_AUDIT].to(torch.int32).contiguous().view(torch.float32).max().item()
            same = all(torch.equal(got[k], plain[k]) for k in range(3))
            res[share] = (same, viol, ops.executed_evals(c_, 100)[1].sum().item())
            if what == 'covering':
                assert same and viol == 0.0, (share, same, viol)
        print('[minsdf share dent] %s L %.3f (steepest found in the pocket %.2f, calibrated %.3f), %d searches: unshared identical '
              '%s, audit %.3e, %d single-pass evaluations; shared identical %s, audit %.3e, %d' % (
                  what, lip, steep, floor, plain[3][:, _lib.CNT_SEARCHES].sum().item(), *res['0'], *res['1']))
