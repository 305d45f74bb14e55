"""Helpers the tracer tests share (tests/test_gpu_kernels.py, tests/test_gpu_mlp_shapes.py, tests/test_gpu_tracer_rays.py): packing an SDF net, tracing a batch
on the GPU, and comparing a trace with oracle/tracer.py."""
import torch

from oracle import nets

DEV = 'cuda:0'


def build_sdf(mc, sd, f16x3=False):
    from nefii_amd import ops
    specs, enc = ops.sdf_specs(mc['implicit_network'], mc['feature_vector_size'])
    pm = ops.PackedMLP(specs, ops.ACT_SOFTPLUS100, ops.HEAD_NONE, enc, 0, DEV, f16x3=f16x3)
    ws, bs = [], []
    for l in range(len(specs)):
        w, b = nets.linear_params(sd, 'implicit_network.lin%d' % l)
        ws.append(w.to(DEV))
        bs.append(b.to(DEV))
    pm.pack(ws, bs)
    return pm


def run_gpu_trace(mc, sd, o, d, om, training, steps, precision='f32', coarse_tau=0.0, coarse_cap=0, pm=None, **tier):
    from nefii_amd import ops
    pm = pm or build_sdf(mc, sd, f16x3=precision.startswith('f16x3'))
    tp = ops.make_tracer_params(mc['ray_tracer'], training, precision, coarse_tau=coarse_tau, coarse_cap=coarse_cap, **tier)
    lin = torch.linspace(0, 1, steps=tp.n_steps).to(DEV)
    st = steps.to(DEV) if steps is not None else torch.rand(tp.n_steps).to(DEV)
    return ops.trace_rays(pm, tp, o.to(DEV).contiguous(), d.to(DEV).contiguous(), om.to(DEV), lin, st,
                          want_counters=True)


def compare_trace(sdf, o, d, got, ref_hit, ref_dists, what, argmin_rays=None, worst=True):
    """hit mask equal up to a bounded number of knife-edge flips.  Depth of surface hits: median at fp32
    rounding level; the worst ray may differ by ~one sdf_threshold (5e-5) when `sdf <= threshold` flips on
    summation-order noise and one side takes an extra step.  `argmin_rays`: rays whose depth is the argmin
    over 100 samples (misses; in training mode also masked-out hits, ray_tracing.py:89-97) - near-ties flip
    the winner, so these are compared through the SDF value they reach.  worst=False: the median and 95 % bounds only - for callers
    that hold every single ray to a bound of its own (tests/trace64.py's judge: the worst ray within one sdf_threshold of fp64, which
    a parameter set may put above the 1.5e-4 asserted here)."""
    pts, hit, dist, _ = got
    hit, dist, pts = hit.cpu(), dist.cpu(), pts.cpu()
    flips = (hit != ref_hit).sum().item()
    print('[tracer %s] %d rays, hit-mask flips vs reference %d' % (what, hit.numel(), flips))
    assert flips <= max(1, int(0.004 * hit.numel())), (what, flips)
    same = hit == ref_hit
    if argmin_rays is None:
        argmin_rays = ~ref_hit
    h = same & ~argmin_rays
    if h.any():
        err = (dist[h] - ref_dists[h]).abs()
        assert not worst or err.max().item() < 1.5e-4, (what, err.max().item())
        assert err.median().item() < 2e-6, (what, err.median().item())
        assert (err < 5e-6).float().mean().item() > 0.95, what
    m = same & argmin_rays
    if m.any():
        a = sdf(o[m] + dist[m].unsqueeze(-1) * d[m])
        b = sdf(o[m] + ref_dists[m].unsqueeze(-1) * d[m])
        ds = (a - b).abs()
        # a march that takes one extra <=5e-5 step shifts all 100 samples; on a bumpy field (|grad| ~ 10)
        # that moves the reached SDF value by up to ~1e-3 for a handful of rays
        assert not worst or ds.max().item() < 5e-3, (what, ds.max().item())
        assert (ds < 2e-5).float().mean().item() > 0.95, (what, (ds < 2e-5).float().mean().item())
        assert ((dist[m] - ref_dists[m]).abs() < 2e-5).float().mean().item() > 0.93, what
    assert (pts - (o + dist.unsqueeze(-1) * d)).abs().max().item() < 1e-6


def argmin_set(ref_hit, obj, training):
    return (~ref_hit | ~obj) if training else ~ref_hit
