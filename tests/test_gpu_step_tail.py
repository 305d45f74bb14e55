"""The kernels that open and close the training step against float64 (tests/tail64.py holds the references, the bounds and the
case lists): nefii_idr_loss through IDRLoss / ops.IdrLossFn, nefii_prepare_hits, nefii_assemble_rows / nefii_gather_rows,
nefii_material_head_global and nefii_camera_rays - and the argument checks of their wrappers, which refuse a call that would
read past the end of a tensor before anything is enqueued.

Measured on an MI355X, worst figure over the case list against its bound min(cap, max(4 x fp32 reference, floor)):
  loss terms            1.0e-7 relative (loss of n1025-no_outside-a1600)     bound 5.0e-7
  loss gradients        1.7e-7 per element (d_sg of r2-n4096-smooth)         bound 6.7e-7; every exact zero exact
  prepare_hits          1.4e-7 absolute (view, n 2100 F 512)                  bound 2.0e-7 (the cap)
  camera directions     1.4e-7 absolute (B 2 S 270000)                        bound 3.0e-7 (the cap)
  material head         4.9e-8 of max(1, |ref|max) (roughness at 5)           bound 5.0e-7
                        per element, relative: 4.6e-4 at 10 (bound 4.4e-3), 1.3e-5 at 5 (5.3e-5), 2.4e-7 at -30 (7.0e-7),
                        at 30 exactly 0 as the fp32 reference; never above a third of its bound
  rows                  every output and every gradient bit-exact; two runs of the loss give the same bits
The kernel figures equal the fp32 reference's to two digits almost everywhere: no case found a kernel wrong.  What the cases
did find is in the wrappers: the ragged patch tail the fused loss dropped, and camera_rays without a ray, which was refused as
a bad argument.  The file (46 tests) runs in 2.8 s; the slowest test takes 0.5 s, the first launch of the process."""
import ctypes
import importlib

import pytest
import torch

import tail64
from nefii_amd import _lib, ops
from nefii_amd.model.loss import IDRLoss
from tail64 import Judge

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


# ---- loss ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in tail64.LOSS_CASES])
def test_fused_idr_loss_vs_fp64(name):
    case = tail64.LOSS_BY_NAME[name]
    inp = tail64.loss_inputs(case)
    r64, r32 = tail64.run_loss(case, inp, torch.float64), tail64.run_loss(case, inp, torch.float32)
    got = tail64.run_loss(case, inp, torch.float32, device=DEV, fused=True)
    again = tail64.run_loss(case, inp, torch.float32, device=DEV, fused=True)
    j = Judge('idr_loss %s' % name)
    tail64.judge_loss(j, name, got, r64, r32)
    same = all(torch.equal(got['terms'][k], again['terms'][k]) for k in tail64.TERMS) and \
        all((got[k] is None and again[k] is None) or torch.equal(got[k], again[k]) for k in ('d_idr', 'd_sg'))
    j.require('two runs', same, 'the same bits' if same else 'two runs differ')
    j.done()


# ---- prepare_hits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,rows,fcols,order', tail64.HITS_CASES)
def test_prepare_hits_vs_fp64(n, rows, fcols, order):
    a = tail64.hits_inputs(n, rows, fcols, order)
    r64, r32 = tail64.hits_ref(*a, torch.float64), tail64.hits_ref(*a, torch.float32)
    got = ops.prepare_hits(*[None if t is None else t.to(DEV) for t in a])
    j = Judge('prepare_hits n%d rows%d F%d %s' % (n, rows, fcols, order))
    tail64.judge_hits(j, 'hits', [None if t is None else t.cpu() for t in got], r64, r32)
    j.done()


# ---- rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c['name'] for c in tail64.ROW_CASES])
def test_assemble_and_gather_rows_are_bit_exact(name):
    assert tail64.MAX_ROW_BLOCKS == _lib.MAX_ROW_BLOCKS
    case = [c for c in tail64.ROW_CASES if c['name'] == name][0]
    where, srcs, fills, wts = tail64.rows_inputs(case)
    want, want_grads = tail64.rows_ref(case, where, srcs, fills, wts)
    rows = case['rows']
    total = rows + (1 if case['pad'] else 0)
    leaves = [s.to(DEV).requires_grad_(k != case['const']) for k, s in enumerate(srcs)]
    outs = ops.assemble_rows(where.to(DEV), total, fills, case['cols'], leaves)
    j = Judge('rows %s' % name)
    for k, (o, w) in enumerate(zip(outs, want)):
        j.same_bits('out %d [%s %d]' % (k, case['forms'][k], case['cols'][k]), o.detach()[:rows], w[:rows])   # (without the scratch row)
        j.require('out %d requires_grad' % k, o.requires_grad == (k != case['const']), str(o.requires_grad))
    used = [k for k in range(len(srcs)) if k != case['unused'] and k != case['const']]
    sum((outs[k][:rows] * wts[k].to(DEV)).sum() for k in used).backward()
    for k, (leaf, w) in enumerate(zip(leaves, want_grads)):
        if w is None:
            j.require('grad %d' % k, leaf.grad is None, 'None expected (the output takes no part in the loss)')
        else:
            j.require('grad %d exists' % k, leaf.grad is not None, str(leaf.grad is not None))
            if leaf.grad is not None:
                j.same_bits('grad %d [%s %d]' % (k, case['forms'][k], case['cols'][k]), leaf.grad, w)
    j.done()


# ---- material head ---------------------------------------------------------------------------------------------------
def test_material_head_vs_fp64():
    j = Judge('material head')
    for p, n_spec, fr, fs, drop in tail64.HEAD_CASES:
        rp, sp, w_r, w_s = tail64.head_inputs(p, n_spec)
        r64 = tail64.head_ref(rp, sp, w_r, w_s, fr, fs, drop, torch.float64)
        r32 = tail64.head_ref(rp, sp, w_r, w_s, fr, fs, drop, torch.float32)
        a, b = rp.detach().to(DEV).requires_grad_(True), sp.detach().to(DEV).requires_grad_(True)
        rough, spec = ops.MaterialHeadGlobalFn.apply(a, b, fr, fs)
        loss = 0
        if drop != 'rough':
            loss = loss + (rough * w_r.to(DEV)).sum()
        if drop != 'spec':
            loss = loss + (spec * w_s.to(DEV)).sum()
        loss.backward()
        got = (rough.detach(), spec.detach(), a.grad, b.grad)
        tail64.judge_head(j, 'p%g s%d %d%d %s' % (p, n_spec, fr, fs, drop), p, n_spec, got, r64, r32)
    j.done()


# ---- camera ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,S,kind', tail64.CAMERA_CASES)
def test_camera_rays_vs_fp64(B, S, kind):
    uv, pose, K = tail64.camera_inputs(B, S)
    sel = tail64.camera_subset(S, kind)
    d64, _ = tail64.camera_ref(uv[:, sel], pose, K, torch.float64)
    d32, _ = tail64.camera_ref(uv[:, sel], pose, K, torch.float32)
    dirs, orig = ops.camera_rays(uv.to(DEV), pose.to(DEV), K.to(DEV))
    j = Judge('camera B%d S%d' % (B, S))
    j.absolute('dirs', dirs.cpu()[:, sel], d64, d32, cap=tail64.CAP_CAMERA)
    ok = torch.equal(orig.cpu(), pose[:, None, :3, 3].expand(B, S, 3))
    j.require('origins', ok, 'the pose translation of every ray, bit for bit' if ok else 'differ from the pose translation')
    ok = bool(torch.isfinite(dirs).all()) and (dirs.double().norm(dim=-1) - 1).abs().max().item() < 3e-7
    j.require('every ray', ok, 'unit length' if ok else 'a ray is not of unit length')
    j.done()


# ---- argument checks -------------------------------------------------------------------------------------------------
class Launches:
    """counts the launches the wrappers of ops.loss / ops.shading / ops.tracer make"""

    def __init__(self, monkeypatch):
        self.names = []
        for mod in (importlib.import_module('nefii_amd.ops.' + m) for m in ('loss', 'shading', 'tracer')):
            real = mod.call

            def counted(name, *a, _real=real, **kw):
                self.names.append(name)
                return _real(name, *a, **kw)
            monkeypatch.setattr(mod, 'call', counted)


def _refused(launches, fn):
    before = list(launches.names)
    with pytest.raises(ValueError):
        fn()
    assert launches.names == before, launches.names[len(before):]


def test_idr_loss_refuses_mismatched_rays_before_anything_is_enqueued(monkeypatch):
    n = 64
    case = dict(tail64.LOSS_BY_NAME['r1-n1024-smooth'], n=n)
    inp = {k: v.to(DEV) for k, v in tail64.loss_inputs(case).items()}
    kw = tail64.loss_kwargs(case)
    kinds = {'L1': 0, 'L2': 1, 'L1_smooth': 2}
    p = _lib.LossParams(kw['idr_rgb_weight'], kw['sg_rgb_weight'], kw['mask_weight'], kw['alpha'], kw['normalsmooth_weight'],
                        kw['background_rgb_weight'], kinds[kw['loss_type']], kinds[kw['env_loss_type']], 1, 0)
    # the entry point itself: n = 62 is no whole number of 4-ray patches -> NEFII_E_SHAPE, the canaries stay
    losses, d_idr, d_sg = (torch.full(s, 7.0, device=DEV) for s in ((6,), (n, 3), (n, 3)))
    net, obj = inp['network_object_mask'].to(torch.uint8), inp['object_mask'].to(torch.uint8)
    ptr = lambda t: t.data_ptr()                                                                # noqa: E731
    args = lambda n_: (ctypes.byref(p), ptr(inp['idr_rgb_values']), ptr(inp['sg_rgb_values']), ptr(inp['rgb']), ptr(net), ptr(obj),   # noqa: E731
                       ptr(inp['sdf_output']), ptr(inp['normal_values']), n_, ptr(losses), ptr(d_idr), ptr(d_sg),
                       torch.cuda.current_stream().cuda_stream)
    lib = _lib.lib()
    for bad_n in (62, 63, 1, 0):
        assert lib.nefii_idr_loss(*args(bad_n)) == -2, bad_n
    torch.cuda.synchronize()
    for t in (losses, d_idr, d_sg):
        assert bool((t == 7.0).all())
    assert lib.nefii_idr_loss(*args(60)) == 0                               # whole patches: served, and only 60 rows written
    torch.cuda.synchronize()
    assert bool((losses != 7.0).all()) and bool((d_sg[60:] == 7.0).all()) and bool((d_sg[:60] != 7.0).all())
    # the wrapper
    launches = Launches(monkeypatch)
    a = [inp['idr_rgb_values'].requires_grad_(True), inp['sg_rgb_values'].requires_grad_(True), inp['rgb'], inp['network_object_mask'],
         inp['object_mask'], inp['sdf_output'], inp['normal_values'], p]
    short = lambda i, m=n - 2: [t[:, :m] if (k == i and k == 2) else t[:m] if k == i else t for k, t in enumerate(a)]   # noqa: E731
    for i in range(7):
        _refused(launches, lambda: ops.IdrLossFn.apply(*short(i)))
    _refused(launches, lambda: ops.IdrLossFn.apply(*[t[:, :n - 2] if k == 2 else t[:n - 2] if k < 7 else t for k, t in enumerate(a)]))
    L = IDRLoss(**kw)
    out = {'idr_rgb_values': a[0][:62], 'sg_rgb_values': a[1][:62], 'network_object_mask': a[3][:62], 'object_mask': a[4][:62],
           'sdf_output': a[5][:62], 'normal_values': a[6][:62], 'grad_theta': None}
    _refused(launches, lambda: L(out, {'rgb': a[2][:, :62]}))               # as the torch formulation it replaces raises
    assert launches.names == []
    lo = ops.IdrLossFn.apply(*a)                                            # the next valid call is served
    lo[0].backward()
    assert launches.names == ['nefii_idr_loss'] and bool(torch.isfinite(lo).all()) and a[1].grad.shape == (n, 3)
    p.normalsmooth_weight = 0.                                              # no patch term: any n is served
    assert bool(torch.isfinite(ops.IdrLossFn.apply(*[t[:, :62] if k == 2 else t[:62] if k < 7 else t for k, t in enumerate(a)])).all())


def test_prepare_hits_and_assemble_rows_refuse_before_anything_is_enqueued(monkeypatch):
    launches = Launches(monkeypatch)
    rows, n, F = 40, 16, 5
    g = torch.Generator().manual_seed(2)
    pts, dirs, grad = (torch.randn(rows, 3, generator=g).to(DEV) for _ in range(3))
    feat = torch.randn(rows, F, generator=g).to(DEV)
    idx = torch.randint(0, rows, (n,), generator=g).to(DEV)
    for bad in ((pts, dirs, grad, feat, idx.int()),                         # 4-byte entries read as 8-byte ones
                (pts, dirs, grad, feat, idx.cpu()),
                (pts, dirs, grad, feat, idx.reshape(4, 4)),
                (pts, dirs, grad, feat, idx.repeat(2)[::2]),                # not contiguous
                (pts, dirs, grad, feat, idx.float()),
                (pts[:rows - 1], dirs, grad, feat, idx),
                (pts, dirs[:rows - 1], grad, feat, idx),
                (pts, dirs, grad[:rows - 1], feat, idx),
                (pts, dirs, grad, feat[:rows - 1], idx),
                (pts, dirs, grad[:, :2], feat, idx),
                (pts[:0], dirs[:0], grad[:0], None, idx)):
        _refused(launches, lambda: ops.prepare_hits(*bad))
    p, v, nrm, f = ops.prepare_hits(pts, dirs, grad, feat, idx)            # the next valid call is served
    assert launches.names == ['nefii_prepare_hits'] and torch.equal(p, pts[idx]) and torch.equal(f, feat[idx])
    assert ops.prepare_hits(pts, dirs, grad, None, idx[:0])[0].shape == (0, 3) and launches.names == ['nefii_prepare_hits']

    launches.names.clear()
    full, one = torch.randn(n, 3, generator=g).to(DEV), torch.randn(1, 1, generator=g).to(DEV)
    where = torch.randperm(rows, generator=g)[:n].to(DEV)
    for bad in ((where.int(), rows, [0.], [3], [full]),
                (where.cpu(), rows, [0.], [3], [full]),
                (where.reshape(1, n), rows, [0.], [3], [full]),
                (where, rows, [0.], [3], [full[:n - 1]]),                   # neither n rows nor one
                (where, rows, [0., 0.], [3, 3], [full, full[:2]]),          # the second source: nothing of the first is written
                (where, rows, [0.], [4], [full]),                           # neither cols columns nor one
                (where, rows, [0.], [3], [full.reshape(-1)]),
                (where, rows, [0.], [3, 1], [full, one]),                   # a fill or a column count missing
                (where, rows, [0., 0.], [3], [full, one]),
                (where, 0, [0.], [3], [full]),
                (where, rows, [0.] * 13, [1] * 13, [one] * 13)):
        _refused(launches, lambda: ops.assemble_rows(*bad))
    assert launches.names == []
    out, = ops.assemble_rows(where, rows, [2.], [3], [full.requires_grad_(True)])
    rest = torch.ones(rows, dtype=torch.bool, device=DEV).index_fill(0, where, False)
    assert launches.names == ['nefii_assemble_rows'] and torch.equal(out[where], full) and bool((out[rest] == 2.).all())
    out.sum().backward()
    assert launches.names[-1] == 'nefii_gather_rows' and bool((full.grad == 1).all())


def test_camera_rays_refuses_mismatched_batches_before_anything_is_enqueued(monkeypatch):
    launches = Launches(monkeypatch)
    uv, pose, K = (t.to(DEV) for t in tail64.camera_inputs(3, 17))
    for bad in ((uv, pose[:2], K), (uv, pose, K[:1]), (uv, pose[:, :3], K), (uv, pose, K[:, :3, :3]), (uv[0], pose[0], K[0]),
                (uv[:, :, :1], pose, K), (uv, pose.reshape(3, 16), K)):
        _refused(launches, lambda: ops.camera_rays(*bad))
    assert launches.names == []
    d, o = ops.camera_rays(uv, pose, K)
    assert launches.names == ['nefii_camera_rays'] and d.shape == (3, 17, 3) and bool(torch.isfinite(d).all())
    assert ops.camera_rays(uv[:, :0], pose, K)[0].shape == (3, 0, 3) and launches.names == ['nefii_camera_rays']     # no ray, no launch
