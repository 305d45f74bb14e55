"""The MLP training kernels after their memory round trips were batched (profiles/mlp_round_trips):
the streamed backward kernel issues a layer's stash loads and the seed's two loads unconditionally on CLAMPED rows and turns
rows past n into zeros by selection; the blocked weight gradient keeps two point slabs in flight; the gradient scale reduces
large inputs over many blocks.  What can go wrong with that is a wrong clamp, a clamped row leaking into a live one, a store
past n, a slab staged out of order, a maximum lost between blocks - so:

* backward and forward on the radiance-shaped (4 x 512, ReLU) and the material-shaped (8 x 512, ELU) streamed nets, fp16 and
  fp32 stash, n around the 64-row tile and 16385 (256 workgroups x 64 rows + 1: one workgroup gets a second, ragged tile):
  outputs, parameter gradients (test_gpu_mlp_shapes.judge, its bounds) and every layer's dz (rel-L2 against fp64 within the
  gradients' bound: dz is what the gradients are contracted from), and the first n rows of outputs, stash and dz equal BIT FOR
  BIT those of a call on the inputs zero-padded to the next multiple of 64 (layer l + 1's rows follow layer l's in dz: a store
  past n lands in them);
* weight and bias gradients through both weight-gradient kernels: the issue's point counts around 32 (scalar-load kernel) and
  4097, and counts whose last point slice holds 1, 2 or 3 slabs of the blocked kernel;
* the gradient scale against a float32 restatement of its rule on the CPU, exactly, on both sides of the many-block threshold,
  with the maximum at the first element, the last, and the last one of a block's first sweep (aligned, unaligned and head
  kernels); inf / NaN entries, zeros, the
  exponent clamps; the head form on both sides of 2 |pre| = 8; two calls in flight on two streams and back to back on one."""
import types

import numpy as np
import pytest
import torch

import mlp64
import test_gpu_mlp_shapes as shapes
from mlp64 import CAP_GRAD, Judge, Reference, make_inputs
from nefii_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
NETS = {'rad': 'conf-h512-rad', 'mat': 'conf-h512-mat'}
_built, _refs = {}, {}


def _net(which):
    if which not in _built:
        _built[which] = [c for c in mlp64.SHAPE_CASES if c.id == NETS[which]][0].build()
    return _built[which]


def _reference(which, n):
    """fp64 / fp32 runs of mlp64.forward with the parameter gradients AND every layer's dz = d loss / d pre-activation; shaped
    like mlp64.Reference (kink rows un-seeded the same way) so that test_gpu_mlp_shapes.judge takes it.  Computed once per
    (net, n) and left unchanged."""
    if (which, n) in _refs:
        return _refs[which, n]
    net = _net(which)
    ins, feat, w1 = make_inputs(net, n, 11 + n)
    fwd = Reference(net, ins, feat, w1, grads=False)            # kink rows, d_out
    ref = types.SimpleNamespace(ins=ins, feat=feat, d_out=fwd.d_out, unseeded=fwd.unseeded)
    for name, dt in (('r64', torch.float64), ('r32', torch.float32)):
        sd = {k: v.detach().to(dt).requires_grad_(True) for k, v in net.sd.items()}
        cast = lambda t: None if t is None else t.to(dt)
        out, pre, hidden, Ws = mlp64.forward(net, sd, tuple(cast(t) for t in ins), cast(feat))
        leaves = list(sd.values()) + (Ws if net.weight_norm else [])
        got = torch.autograd.grad((out * ref.d_out.to(dt)).sum(), leaves + pre)
        g = dict(zip(list(sd.keys()) + (['dW%d' % l for l in range(len(Ws))] if net.weight_norm else []), got))
        if not net.weight_norm:
            g.update({'dW%d' % l: g[k + '.weight'] for l, k in enumerate(net.keys)})
        setattr(ref, name, dict(out=out.detach(), hidden=hidden.detach(), grads=g, dz=list(got[len(leaves):])))
    _refs[which, n] = ref
    return ref


def _pad_rows(t, rows):
    if t is None or t.shape[0] == rows:
        return t
    out = torch.zeros((rows,) + tuple(t.shape[1:]), device=t.device, dtype=t.dtype)
    out[:t.shape[0]] = t
    return out


def _state(pm, args, d, gscale):
    """forward with the stash kept + backward -> (out, the stash tensors, dz); gscale None: the scale training derives"""
    out, _, stash = ops.mlp_forward(pm, *args, want_stash=True)
    if gscale is None:
        gscale = ops.mlp_backward_scale(pm, d, stash)
    dz = ops.mlp_backward(pm, d, stash, gscale)
    torch.cuda.synchronize()
    return out, stash, dz, gscale


@pytest.mark.parametrize('n', [1, 63, 64, 65, 129, 16385])
@pytest.mark.parametrize('which', ['rad', 'mat'])
def test_backward_forward_tiles(which, n, monkeypatch):
    net, ref = _net(which), _reference(which, n)
    assert ref.unseeded <= mlp64.MAX_UNSEEDED, ref.unseeded
    lib, L, judges = _lib.lib(), len(net.specs), []
    for arith in ('f16x3-fp32stash', 'f16x3'):
        gs = 1e-6               # gradients as small as training's: the gradient scale is exercised (test_gpu_mlp_shapes)
        pm, family = shapes.build_packed(net, arith, monkeypatch)
        assert family == ('stream+h16' if arith == 'f16x3' else 'stream')
        out, hidden, grads, args = shapes.run_gpu(net, pm, ref.ins, ref.feat, ref.d_out * gs)
        J = Judge('%s n=%d %s family=%s un-seeded %.3f' % (NETS[which], n, arith, family, ref.unseeded))
        shapes.judge(J, net, ref, arith, out, hidden, {k: g.double() / gs for k, g in grads.items()})
        d = (ref.d_out * gs).to(DEV).contiguous()
        out1, stash, dz, S = _state(pm, args, d, None)
        h16 = isinstance(stash, ops.HalfStash)
        assert h16 == (arith == 'f16x3') and dz.dtype == (torch.float16 if h16 else torch.float32)
        assert torch.equal(out1, out)
        unscale = gs * (S.item() if h16 else 1.0)
        for l in range(L):
            J.close('dz%d' % l, dz[l, :, :net.specs[l].n_out].double() / unscale, ref.r64['dz'][l], ref.r32['dz'][l],
                    floor=CAP_GRAD[arith], cap=CAP_GRAD[arith])
        # the same rows inside whole tiles: zero rows appended up to the next multiple of 64, the same scale
        rows = -(-n // 64) * 64
        out_p, stash_p, dz_p, _ = _state(pm, tuple(_pad_rows(t, rows) for t in args), _pad_rows(d, rows), S)
        J.require('padded: out', torch.equal(out_p[:n], out1), 'rows [0, %d) of %d' % (n, rows))
        if h16:
            same = (torch.equal(stash_p.h[:, :n], stash.h) and torch.equal(stash_p.x0[:n], stash.x0)
                    and torch.equal(stash_p.z_last[:n, :net.n_out], stash.z_last[:, :net.n_out]))
        else:
            same = all(torch.equal(stash_p[l, :n, :net.specs[l].n_out], stash[l, :, :net.specs[l].n_out]) for l in range(L))
        J.require('padded: stash', same, 'h16=%s' % h16)
        for l in range(L):
            w = lib.nefii_padded_width(net.specs[l].n_out)          # (the columns the kernel writes)
            a, b = dz_p[l, :n, :w], dz[l, :, :w]
            J.require('padded: dz%d' % l, torch.equal(a, b), '%d of %d elements differ' % ((a != b).sum().item(), b.numel()))
        judges.append(J)
    bad = []
    for J in judges:
        try:
            J.done()
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('P', [1, 31, 32, 33, 95, 1025, 1121, 1153, 4097])
def test_weight_gradients_both_kernels(P, monkeypatch):
    """every dW, its single rows and columns, and every bias gradient against fp64 (test_gpu_mlp_shapes.judge).  Below 1024
    points the scalar-load kernel runs (untouched, kept as the issue's cases around its 16- and 32-point batches); from 1024 on
    the blocked one, whose point slices are walked in 32-row slabs, two in flight: 4097 gives slices of 17 slabs and a ragged
    one of 10 (the backward test's 16385: 65 and 58), and 1025 / 1153 / 1121 end in a slice of 3 ragged / 2 ragged / 1 slab
    (8 slices of 160 rows: 65, 33 and 1 rows are left for the last) - the lengths at which the loop's prologue already holds
    every slab there is."""
    net, ref = _net('rad'), _reference('rad', P)
    pm, family = shapes.build_packed(net, 'f16x3', monkeypatch)
    assert family == 'stream+h16'
    gs = 1e-6
    out, hidden, grads, _ = shapes.run_gpu(net, pm, ref.ins, ref.feat, ref.d_out * gs)
    J = Judge('%s P=%d weight gradients' % (NETS['rad'], P))
    shapes.judge(J, net, ref, 'f16x3', out, hidden, {k: g.double() / gs for k, g in grads.items()})
    assert any(k.endswith('.bias') for k in ref.r64['grads'])
    J.done()


# ---- the gradient scale ---------------------------------------------------------------------------------------------------
THRESHOLD = 65536           # nefii_mlp_grad_scale*: more elements than this are reduced over many blocks
COUNTS = [1, 1023, 1024, 1025, THRESHOLD, THRESHOLD + 1, 3 * 70001]


def _rule(cands):
    """the rule restated in float32: the largest finite candidate m = f 2^e (f in [0.5, 1)) gives 2^clamp(8 - e, -40, 60); 1
    without a positive one"""
    c = np.abs(np.asarray(cands, dtype=np.float32))
    c = c[c < np.float32(3.0e38)]               # (drops NaN and inf)
    m = c.max() if c.size else np.float32(0)
    if not m > 0:
        return 1.0
    e = int(np.frexp(m)[1])
    return float(np.ldexp(np.float32(1), min(max(8 - e, -40), 60)))


def _positions(count):
    """the first element, the last, and the last one of block 0's first sweep: 256 threads x 16 bytes in the aligned kernel
    (1023), 256 x 4 bytes in the unaligned one and in the head form (255)"""
    return sorted({0, count - 1, min(count, 1024) - 1, min(count, 256) - 1})


def _scale(d):
    s = ops.mlp_grad_scale(d)
    assert s.numel() == 1
    return s


def _background(count, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(count, generator=g) - 0.5) * 2e-6         # |d| < 1e-6


@pytest.mark.parametrize('count', COUNTS)
def test_grad_scale_counts_and_positions(count):
    base = _background(count, count)
    for k, pos in enumerate(_positions(count)):
        d = base.clone()
        d[pos] = (-1.0) ** k * 3.1e-4 * 1.3 ** k                  # the maximum, away from a power of two
        want = _rule(d.numpy())
        got = _scale(d.to(DEV)).item()
        assert got == want, (count, pos, got, want)
        assert 128.0 <= got * d.abs().max().item() < 256.0
        # the same values in a buffer that is not 16-byte aligned: the scalar loads
        buf = torch.zeros(count + 1, device=DEV)
        buf[1:] = d.to(DEV)
        assert buf[1:].data_ptr() % 16 == 4 and _scale(buf[1:]).item() == want, (count, pos, 'unaligned')


@pytest.mark.parametrize('count', [1025, THRESHOLD, THRESHOLD + 1, 3 * 70001])
def test_grad_scale_special_inputs(count):
    base = _background(count, 7)
    d = base.clone()
    d[0], d[count // 2], d[count - 1], d[count - 2] = float('inf'), float('nan'), float('-inf'), 0.7
    want = _rule(d.numpy())
    assert want == 2.0 ** 8 and _scale(d.to(DEV)).item() == want                 # inf and NaN are ignored
    assert _scale(torch.zeros(count, device=DEV)).item() == 1.0                  # all zeros
    assert _scale(torch.full((count,), float('nan'), device=DEV)).item() == 1.0
    for mag, want in ((1.3e-30, 2.0 ** 60), (1.3e30, 2.0 ** -40)):               # the exponent clamps
        d = base.clone() * (mag / 1e-6)
        d[count - 1] = mag
        assert _rule(d.numpy()) == want
        assert _scale(d.to(DEV)).item() == want, mag


def _head_scale(d, pre):
    s = torch.empty(1, device=DEV)
    ops.call('nefii_mlp_grad_scale_head', d.data_ptr(), d.shape[1], pre.data_ptr(), pre.shape[1], d.shape[0], d.shape[1],
             ops.HEAD_POW2, s.data_ptr())
    return s


@pytest.mark.parametrize('count', COUNTS)
def test_grad_scale_head_form(count):
    """POW2 head: max(|d|, |d 2 pre| / 8); the pre-activation of the decisive row on both sides of 2 |pre| = 8, the decisive
    element at the first, the last and a block-boundary position; inf / NaN entries ignored, zeros give 1"""
    n_out = 3 if count % 3 == 0 else 1
    n = count // n_out
    g = torch.Generator().manual_seed(count + 1)
    base_d = _background(count, count + 2).view(n, n_out)
    base_z = (torch.rand(n, n_out, generator=g) - 0.5) * 2.0      # |2 pre| < 2
    for k, pos in enumerate(_positions(count)):
        for z in (3.3, -3.3, 5.9, -5.9, 29.0):                    # 2 |pre| = 6.6 (|d| decides), 11.8, 58 (the head decides)
            d, pre = base_d.clone(), base_z.clone()
            d.view(-1)[pos], pre.view(-1)[pos] = 3.1e-4 * 1.3 ** k, z
            d32, z32 = d.numpy().astype(np.float32), pre.numpy().astype(np.float32)
            want = _rule(np.concatenate([d32.ravel(), (np.abs(d32 * (np.float32(2) * z32)) * np.float32(0.125)).ravel()]))
            got = _head_scale(d.to(DEV), pre.to(DEV)).item()
            assert got == want, (count, pos, z, got, want)
            if abs(z) < 4:
                assert got == _scale(d.to(DEV)).item()
    d, pre = base_d.clone(), base_z.clone()
    d.view(-1)[0], d.view(-1)[count - 1], pre.view(-1)[count // 2] = float('inf'), float('nan'), float('inf')
    d32, z32 = d.numpy().astype(np.float32), pre.numpy().astype(np.float32)
    with np.errstate(all='ignore'):
        want = _rule(np.concatenate([d32.ravel(), (np.abs(d32 * (np.float32(2) * z32)) * np.float32(0.125)).ravel()]))
    assert _head_scale(d.to(DEV), pre.to(DEV)).item() == want
    assert _head_scale(torch.zeros(n, n_out, device=DEV), pre.to(DEV)).item() == 1.0


@pytest.mark.parametrize('count', [THRESHOLD, 3 * 70001])
def test_grad_scale_calls_do_not_meet(count):
    """two calls in flight on two streams, and two back to back on one stream, give what each gives alone"""
    a = (_background(count, 1) * 1.0).to(DEV)
    b = (_background(count, 2) * 4096.0).to(DEV)
    a[count - 1], b[0] = 2.9e-5, -0.37
    alone = [_scale(a).item(), _scale(b).item()]
    assert alone == [_rule(a.cpu().numpy()), _rule(b.cpu().numpy())] and alone[0] != alone[1]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)
    got = []
    for rep in range(4):
        with torch.cuda.stream(s1):
            ra = _scale(a)
        with torch.cuda.stream(s2):
            rb = _scale(b)
        got.append((ra, rb))
    torch.cuda.synchronize()
    assert all([ra.item(), rb.item()] == alone for ra, rb in got)
    back = [_scale(t) for t in (a, b, b, a)]
    torch.cuda.synchronize()
    assert [t.item() for t in back] == [alone[0], alone[1], alone[1], alone[0]]
