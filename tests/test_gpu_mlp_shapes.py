"""The fused-MLP kernels against fp64 over the shapes the C ABI accepts (tests/mlp64.py: yardstick, bounds, kink protocol and
the case lists; tests/test_mlp64_cpu.py proves on the CPU that every bound here is reachable).

Every case first ASSERTS the kernel family that took it (streamed with the state in halves / streamed / generic, against
mlp64.expected_family, the header's rules) and prints it with its Judge table: a sweep that silently ran on the generic kernel
proves nothing about the streamed one.  Three arithmetics per feature net: the f32-input MFMA kernels, 'f16x3' with the fp32
stash (NEFII_MLP_H16=0) and 'f16x3' as training runs it (state in halves on the streamed shapes).

a) the shape matrix (mlp64.SHAPE_CASES): outputs, last hidden activation, every parameter gradient, and every single column and
   row of every dW;  b) activation x head, unscaled and with a head pre-activation of 15 ... 30;  c) conventions at exact zero;
d) refusals;  SDF nets off the shipped shape (mlp64.SDF_CASES) through ops.mlp_forward, ops.sdf_eval and ops.sdf_value_grad.

FINDINGS of the first runs on an MI355X (no kernel computed a wrong value on any shape):
* test_activation_x_head[stream4x512-elu-pow2-scaled] FAILED at first: with the state in halves max |S dz| of that case was
  8188 - exactly 65504 / 8, where LESS is demanded (the ReLU and Softplus nets of the same pair reached 4404 and 4580, every
  other pair at most 502).  nefii_mlp_grad_scale derives S from max |d_out| alone (S max |d_out| in [128, 256)); a POW2 head
  multiplies the seed gradient by 2 |pre|, up to 60 at head pre-activations of 15 ... 30, so S dz of the last layer could reach
  15 360: 4.3 x under fp16's largest number, not the 8 x the project asks for.  Fixed: FusedMLPFn.backward takes the scale of a
  POW2 head from nefii_mlp_grad_scale_head, max(|d_out|, |d_out head'(pre)| / 8); nets whose head derivative stays below 8 -
  every shipped one - get the same S bit for bit.  The case stays as the regression test.
* the per-column / per-row check of dW relative to the slice's OWN norm is not reachable by the fp32 oracle itself (mlp64.Judge.
  slices says why and what is asserted instead).
* nefii_sdf_value_grad keeps nets with ONE hidden layer off its streamed kernel, and streams 256-wide nets with any number of
  output columns: the header now says so.

Per case (largest row count of each; err(gpu) / err(fp32 oracle) / bound; values = worst of outputs and last hidden, max-abs;
gradients = worst parameter, rel-L2; family as asserted for 'f16x3'; unsd = share of rows un-seeded at kinks):

case                                    n family      unsd | f32 values                  | f32 gradients               | f16x3 gradients             | f16x3 dW slices            
physg-h64-rad                         500 generic    0.004 | 1.7e-06 / 1.6e-06 / 6.4e-06 | 1.7e-07 / 2.7e-07 / 3.7e-06 | 4.7e-04 / 1.7e-07 / 2.5e-03 | 1.2e-03 / 2.6e-07 / 1.0e-02
physg-h64-mat                         500 generic    0.000 | 2.8e-06 / 2.8e-06 / 1.1e-05 | 1.6e-07 / 1.8e-07 / 3.7e-06 | 5.2e-04 / 1.8e-07 / 2.5e-03 | 1.2e-03 / 2.5e-07 / 1.0e-02
conf-h64-rad                          301 generic    0.003 | 1.6e-06 / 1.9e-06 / 7.5e-06 | 1.8e-07 / 2.3e-07 / 3.7e-06 | 3.1e-04 / 2.3e-07 / 2.5e-03 | 9.3e-04 / 3.2e-07 / 1.0e-02
conf-h64-mat                          301 generic    0.000 | 3.6e-06 / 3.7e-06 / 1.5e-05 | 3.3e-07 / 3.9e-07 / 3.7e-06 | 5.8e-04 / 2.7e-07 / 2.5e-03 | 2.1e-03 / 3.4e-07 / 1.0e-02
conf-h512-rad                        3000 stream+h16 0.053 | 3.6e-06 / 2.1e-06 / 8.4e-06 | 1.9e-07 / 1.5e-07 / 3.7e-06 | 3.9e-04 / 1.5e-07 / 2.5e-03 | 1.3e-03 / 2.7e-07 / 1.0e-02
conf-h512-mat                        3000 stream+h16 0.000 | 9.6e-06 / 5.3e-06 / 2.0e-05 | 2.9e-07 / 2.0e-07 / 3.7e-06 | 5.0e-04 / 1.8e-07 / 2.5e-03 | 1.6e-03 / 2.3e-07 / 1.0e-02
physg-h512-rad                         64 stream+h16 0.016 | 2.7e-06 / 1.5e-06 / 6.0e-06 | 6.9e-07 / 2.9e-07 / 3.7e-06 | 5.6e-04 / 3.0e-07 / 2.5e-03 | 1.6e-03 / 5.5e-07 / 1.0e-02
physg-h512-mat                         64 stream+h16 0.000 | 4.8e-06 / 2.9e-06 / 1.2e-05 | 6.1e-07 / 3.9e-07 / 3.7e-06 | 4.8e-04 / 3.9e-07 / 2.5e-03 | 1.1e-03 / 6.1e-07 / 1.0e-02
s01-nvd-F32-1x512-o1                20011 stream+h16 0.009 | 2.1e-06 / 2.8e-06 / 1.1e-05 | 3.1e-07 / 1.0e-06 / 4.0e-06 | 2.2e-04 / 1.7e-07 / 2.5e-03 | 4.7e-04 / 3.2e-07 / 1.0e-02
s02-nn-F100-2x512-o8                20011 stream+h16 0.021 | 9.5e-06 / 3.4e-06 / 1.4e-05 | 1.5e-07 / 2.2e-07 / 3.7e-06 | 2.6e-04 / 2.2e-07 / 2.5e-03 | 9.5e-04 / 5.9e-07 / 1.0e-02
s03-idr0-F256-4x512-o4              20011 stream+h16 0.077 | 1.8e-06 / 1.0e-06 / 4.5e-06 | 3.0e-07 / 4.1e-07 / 3.7e-06 | 4.6e-04 / 4.1e-07 / 2.5e-03 | 1.3e-03 / 3.0e-07 / 1.0e-02
s04-m0-F512-8x512-o3                20011 stream+h16 0.000 | 9.4e-06 / 5.2e-06 / 2.0e-05 | 7.0e-07 / 4.5e-07 / 3.7e-06 | 6.7e-04 / 4.5e-07 / 2.5e-03 | 1.8e-03 / 2.0e-07 / 1.0e-02
s05-m10-F100-11x512-o4               1000 stream+h16 0.000 | 1.4e-05 / 1.0e-05 / 2.0e-05 | 9.4e-07 / 6.2e-07 / 3.7e-06 | 7.3e-04 / 6.2e-07 / 2.5e-03 | 2.7e-03 / 9.5e-07 / 1.0e-02
s06-m10-F32-1x512-o3                20011 stream+h16 0.000 | 1.6e-06 / 2.1e-06 / 8.4e-06 | 1.1e-07 / 1.6e-07 / 3.7e-06 | 2.0e-04 / 1.6e-07 / 2.5e-03 | 6.3e-04 / 2.7e-07 / 1.0e-02
s07-radnone-F512-2x512-o3           20011 stream+h16 0.037 | 2.1e-06 / 8.5e-07 / 4.5e-06 | 4.0e-07 / 3.6e-07 / 3.7e-06 | 3.5e-04 / 3.6e-07 / 2.5e-03 | 6.0e-04 / 3.9e-07 / 1.0e-02
s08-idr-F512off-4x512-o3             1000 stream+h16 0.061 | 4.1e-06 / 1.8e-06 / 7.3e-06 | 2.5e-07 / 1.8e-07 / 3.7e-06 | 4.2e-04 / 1.8e-07 / 2.5e-03 | 1.3e-03 / 2.2e-07 / 1.0e-02
s09-m10-F512off-2x512-o4              300 stream+h16 0.000 | 2.7e-06 / 1.2e-06 / 4.9e-06 | 1.9e-07 / 1.8e-07 / 3.7e-06 | 3.3e-04 / 1.8e-07 / 2.5e-03 | 1.1e-03 / 2.7e-07 / 1.0e-02
s10-idr-F0-8x512-o8                  1000 stream+h16 0.067 | 5.4e-06 / 2.7e-06 / 1.1e-05 | 3.6e-07 / 2.6e-07 / 3.7e-06 | 6.2e-04 / 2.6e-07 / 2.5e-03 | 2.1e-03 / 5.4e-07 / 1.0e-02
s11-m0-F0-2x512-o3                  20011 stream+h16 0.000 | 5.4e-06 / 2.0e-06 / 8.0e-06 | 1.1e-07 / 1.6e-07 / 3.7e-06 | 3.0e-04 / 2.1e-06 / 2.5e-03 | 8.8e-04 / 4.9e-06 / 1.0e-02
s12-nvd-F256-11x512-o1                 65 stream+h16 0.138 | 2.4e-06 / 1.5e-06 / 6.0e-06 | 1.2e-06 / 7.8e-07 / 3.7e-06 | 9.8e-04 / 7.8e-07 / 2.5e-03 | 2.5e-03 / 1.3e-06 / 1.0e-02
s13-idr0-F100-8x512-o4                 64 stream+h16 0.109 | 1.8e-06 / 1.1e-06 / 4.6e-06 | 1.3e-06 / 8.2e-07 / 3.7e-06 | 8.4e-04 / 8.2e-07 / 2.5e-03 | 1.9e-03 / 1.7e-06 / 1.0e-02
s14-matnone-F256-4x512-o3           20011 stream+h16 0.000 | 4.6e-06 / 2.6e-06 / 1.1e-05 | 3.3e-07 / 2.5e-07 / 3.7e-06 | 4.5e-04 / 2.5e-07 / 2.5e-03 | 9.8e-04 / 1.8e-07 / 1.0e-02
s15-nn-F0-1x512-o3                     65 stream+h16 0.000 | 1.3e-06 / 1.8e-06 / 7.0e-06 | 2.4e-07 / 1.4e-07 / 3.7e-06 | 2.7e-04 / 1.3e-07 / 2.5e-03 | 1.0e-03 / 2.2e-07 / 1.0e-02
s16-idr-F32-4x512-o9                 1000 generic    0.041 | 3.6e-06 / 1.7e-06 / 6.8e-06 | 2.6e-07 / 2.0e-07 / 3.7e-06 | 4.1e-04 / 2.0e-07 / 2.5e-03 | 1.9e-03 / 4.3e-07 / 1.0e-02
s17-nvd-F512-2x512-o9                1000 generic    0.033 | 1.6e-06 / 9.0e-07 / 4.5e-06 | 1.6e-07 / 3.5e-07 / 3.7e-06 | 3.2e-04 / 1.4e-07 / 2.5e-03 | 9.3e-04 / 2.0e-07 / 1.0e-02
g01-idr-F256-4x256-o3               20011 generic    0.024 | 3.9e-06 / 2.2e-06 / 8.8e-06 | 1.6e-07 / 2.2e-07 / 3.7e-06 | 3.8e-04 / 2.2e-07 / 2.5e-03 | 1.4e-03 / 3.3e-07 / 1.0e-02
g02-m10-F100-3x256-o4               20011 generic    0.000 | 3.7e-06 / 2.5e-06 / 9.9e-06 | 1.1e-07 / 1.6e-07 / 3.7e-06 | 3.5e-04 / 1.5e-07 / 2.5e-03 | 9.7e-04 / 2.6e-07 / 1.0e-02
g03-nvd-F32-2x128-o1                  300 generic    0.007 | 1.3e-06 / 1.2e-06 / 4.8e-06 | 1.6e-07 / 4.5e-07 / 3.7e-06 | 3.1e-04 / 1.4e-07 / 2.5e-03 | 7.4e-04 / 1.9e-07 / 1.0e-02
g04-m0-F0-8x128-o3                   1000 generic    0.000 | 5.4e-06 / 4.1e-06 / 1.7e-05 | 1.5e-07 / 4.6e-07 / 3.7e-06 | 6.1e-04 / 4.6e-07 / 2.5e-03 | 1.4e-03 / 1.2e-06 / 1.0e-02
g05-nn-F100-1x64-o8                    65 generic    0.000 | 9.8e-07 / 8.6e-07 / 4.5e-06 | 1.7e-07 / 2.3e-07 / 3.7e-06 | 2.5e-04 / 2.3e-07 / 2.5e-03 | 4.3e-04 / 3.5e-07 / 1.0e-02
g06-m10-F512-4x64-o4                 1000 generic    0.000 | 2.4e-06 / 1.9e-06 / 7.7e-06 | 1.3e-07 / 1.3e-07 / 3.7e-06 | 3.0e-04 / 1.3e-07 / 2.5e-03 | 7.2e-04 / 1.6e-07 / 1.0e-02
g07-idr0-F0-2x32-o4                    64 generic    0.000 | 3.7e-07 / 3.7e-07 / 4.5e-06 | 2.0e-07 / 2.2e-07 / 3.7e-06 | 5.1e-04 / 2.2e-07 / 2.5e-03 | 8.1e-04 / 2.4e-07 / 1.0e-02
g08-m10-F32-11x32-o3                  300 generic    0.000 | 5.0e-06 / 5.8e-06 / 2.0e-05 | 6.3e-07 / 7.5e-07 / 3.7e-06 | 1.0e-03 / 7.5e-07 / 2.5e-03 | 1.4e-03 / 1.0e-06 / 1.0e-02
g09-idr-F512-mixed-o3                1000 generic    0.027 | 2.0e-06 / 1.1e-06 / 4.5e-06 | 2.3e-07 / 2.2e-07 / 3.7e-06 | 3.7e-04 / 2.2e-07 / 2.5e-03 | 1.6e-03 / 6.2e-07 / 1.0e-02
g10-m0-F256-mixed-o4                  300 generic    0.000 | 1.5e-06 / 1.2e-06 / 4.6e-06 | 5.3e-07 / 4.5e-07 / 3.7e-06 | 5.9e-04 / 4.5e-07 / 2.5e-03 | 1.1e-03 / 5.5e-07 / 1.0e-02
g11-idr-F100-2x320-o4                1000 generic    0.015 | 1.7e-06 / 1.2e-06 / 4.9e-06 | 1.9e-07 / 2.7e-07 / 3.7e-06 | 2.8e-04 / 1.2e-07 / 2.5e-03 | 9.2e-04 / 1.7e-07 / 1.0e-02
g12-m10-F0-4x320-o3                    65 generic    0.000 | 4.2e-06 / 2.8e-06 / 1.1e-05 | 4.5e-07 / 3.8e-07 / 3.7e-06 | 4.7e-04 / 3.8e-07 / 2.5e-03 | 1.2e-03 / 6.7e-07 / 1.0e-02
g13-radnone-F256-2x256-o8             300 generic    0.017 | 9.8e-07 / 5.9e-07 / 4.5e-06 | 5.3e-07 / 4.1e-07 / 3.7e-06 | 4.8e-04 / 4.1e-07 / 2.5e-03 | 6.7e-04 / 5.0e-07 / 1.0e-02
g14-idr-F512off-2x64-o1              1000 generic    0.007 | 1.3e-06 / 8.8e-07 / 4.5e-06 | 1.4e-07 / 1.5e-07 / 3.7e-06 | 3.8e-04 / 1.3e-07 / 2.5e-03 | 1.0e-03 / 1.5e-07 / 1.0e-02
g15-m10-F512off-1x128-o4              300 generic    0.000 | 1.5e-06 / 8.8e-07 / 4.5e-06 | 1.3e-07 / 1.5e-07 / 3.7e-06 | 2.4e-04 / 1.5e-07 / 2.5e-03 | 6.0e-04 / 2.4e-07 / 1.0e-02

Activation x head (42 cases x 3 arithmetics), worst err(gpu) and worst err / bound: f32 values 6.7e-6 (0.43), gradients 2.4e-6
(0.47); f16x3 values 3.3e-6 (0.29), gradients 7.3e-4 (0.29), dW slices 1.6e-3 (0.16); the fp32 stash and the half state agree to
three digits.  SDF variants: f32-input kernels' value 3.0e-6 max-abs (0.89 of the bound: 11 x 512, 20 011 rows), split evaluators
1.1e-6 (0.33), gradient 2.5e-6 rel-L2 (0.46) and 6.4e-6 max-abs on the stream (0.64); Step-1 parameter gradients 5.4e-7 (0.15).
The same figures per quantity: DESIGN.md section 2."""
import ctypes

import pytest
import torch

import mlp64
from mlp64 import CAP_GRAD, CAP_OUT, FLOOR_GRAD, FLOOR_VALUE, Judge, Reference, expected_family, make_inputs
from nefii_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _dev(t):
    return None if t is None else t.to(DEV)


def _misaligned(feat):
    """the same rows at a 4-byte offset into their buffer: contiguous, not 16-byte aligned"""
    buf = torch.empty(feat.numel() + 1, device=DEV, dtype=torch.float32)
    out = buf[1:].view(feat.shape)
    out.copy_(feat)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def build_packed(net, arith, monkeypatch):
    """PackedMLP of the net for one arithmetic, with the family it runs on asserted against the header's rules"""
    monkeypatch.setenv('NEFII_MLP_H16', '0' if arith == 'f16x3-fp32stash' else '1')
    pm = ops.PackedMLP(net.specs, net.act, net.head, net.enc, net.F, DEV, half=False if arith == 'f32' else 'f16x3')
    want = expected_family(net.specs, net.enc, net.F, net.head, net.act)
    if arith == 'f32':
        got = 'generic'
        assert not pm.mlp_stream
    else:
        got = 'stream' if pm.mlp_stream else 'generic'
        if ops.h16_supported(pm):
            assert pm.mlp_stream
            got = 'stream+h16'
        expect = want if arith == 'f16x3' else want.replace('+h16', '')
        assert got == expect, 'library runs this net on %r, the header says %r' % (got, expect)
    return pm, got


def run_gpu(net, pm, ins, feat, d_out, misaligned=False):
    """forward + backward through ops.FusedMLPFn -> (out, hidden, grads by state-dict key and 'dW%d')"""
    n = d_out.shape[0]
    a, b, c = (_dev(t) for t in ins)
    if a is None:
        a = torch.zeros(n, 3, device=DEV)           # (a net without encoders still tells the wrapper its row count)
    f = _dev(feat)
    if misaligned:
        f = _misaligned(f)
    leaves = {k: v.to(DEV).requires_grad_(True) for k, v in net.sd.items()}
    Ws, bs = [], []
    for key in net.keys:
        if net.weight_norm:
            w = torch._weight_norm(leaves[key + '.weight_v'], leaves[key + '.weight_g'], 0)
            w.retain_grad()
        else:
            w = leaves[key + '.weight']
        Ws.append(w)
        bs.append(leaves[key + '.bias'])
    out = ops.FusedMLPFn.apply(pm, a, b, c, f, *Ws, *bs)
    out.backward(d_out.to(DEV))
    grads = {k: v.grad for k, v in leaves.items()}
    grads.update({'dW%d' % l: w.grad for l, w in enumerate(Ws)})
    out2, hidden, _ = ops.mlp_forward(pm, a, b, c, f, want_hidden=True)
    assert torch.equal(out2, out.detach())
    torch.cuda.synchronize()
    return out.detach(), hidden, grads, (a, b, c, f)


def judge(J, net, ref, arith, out, hidden, grads, relative=False):
    r64, r32 = ref.r64, ref.r32
    assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads.values())
    J.maxabs('out', out, r64['out'], r32['out'], floor=FLOOR_VALUE, cap=CAP_OUT, relative=relative)
    J.close('out', out, r64['out'], r32['out'], floor=FLOOR_VALUE, cap=CAP_OUT)
    J.maxabs('last hidden', hidden, r64['hidden'], r32['hidden'], floor=FLOOR_VALUE, cap=CAP_OUT, relative=relative)
    cap = CAP_GRAD[arith]
    floor = FLOOR_GRAD if arith == 'f32' else cap           # (one-pass fp16 quantities: the floor is the cap)
    for k in sorted(r64['grads']):
        J.close(k.split('.', 1)[-1], grads[k], r64['grads'][k], r32['grads'][k], floor=floor, cap=cap)
        if k.startswith('dW'):
            e32 = mlp64.rel_l2_64(r32['grads'][k], r64['grads'][k])
            J.slices(k, grads[k], r64['grads'][k], r32['grads'][k], 4.0 * min(cap, max(4.0 * e32, floor)))


def run_case(net, n, seed, monkeypatch, what, misaligned=False, relative=False, units=(), check_dz=False):
    ins, feat, w1 = make_inputs(net, n, seed)
    ref, judges = Reference(net, ins, feat, w1), []
    assert ref.unseeded <= mlp64.MAX_UNSEEDED, ref.unseeded
    for arith in mlp64.ARITHMETICS:
        # gradients as small as training's on the fp16 paths, so that the gradient scale is exercised; the gradients are linear
        # in the upstream gradient, so one reference serves both (compared in double after dividing by gs)
        gs = 1.0 if arith == 'f32' else 1e-6
        pm, family = build_packed(net, arith, monkeypatch)
        out, hidden, grads, args = run_gpu(net, pm, ins, feat, ref.d_out * gs, misaligned)
        grads = {k: g.double() / gs for k, g in grads.items()}
        J = Judge('%s n=%d %s family=%s un-seeded %.3f' % (what, n, arith, family, ref.unseeded))
        judge(J, net, ref, arith, out, hidden, grads, relative)
        for l, u in units:      # a pre-activation of exactly 0: zero gradient, bit for bit
            J.require('unit (%d, %d) at exact zero' % (l, u),
                      not grads['dW%d' % l][u].any().item() and not grads[net.keys[l] + '.bias'][u].any().item(),
                      'max |dW row| %.3e, |db| %.3e' % (grads['dW%d' % l][u].abs().max().item(),
                                                       grads[net.keys[l] + '.bias'][u].abs().item()))
        if check_dz and family == 'stream+h16':
            _, _, stash = ops.mlp_forward(pm, *args, want_stash=True)
            d = (ref.d_out * gs).to(DEV).contiguous()
            dz16 = ops.mlp_backward(pm, d, stash, ops.mlp_backward_scale(pm, d, stash))     # the scale training uses
            assert dz16.dtype == torch.float16
            peak = max(dz16[l, :, :net.specs[l].n_out].float().abs().max().item() for l in range(len(net.specs)))
            J.require('max |S dz|', peak < 65504.0 / 8.0, '%.0f' % peak)
        judges.append(J)
    bad = []
    for J in judges:
        try:
            J.done()
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('case', mlp64.SHAPE_CASES, ids=repr)
def test_shape_matrix(case, monkeypatch):
    net = case.build()
    for n in case.ns:
        run_case(net, n, case.seed + 4 + n, monkeypatch, case.id, misaligned=case.misaligned)


@pytest.mark.parametrize('case', mlp64.HEAD_CASES, ids=repr)
def test_activation_x_head(case, monkeypatch):
    net = case.build()
    run_case(net, case.ns[0], case.seed + 4 + case.ns[0], monkeypatch, case.id, relative=True, check_dz=True)


@pytest.mark.parametrize('cid,build', mlp64.zero_cases(), ids=[c[0] for c in mlp64.zero_cases()])
def test_conventions_at_exact_zero(cid, build, monkeypatch):
    net, units = build()
    run_case(net, 300, 9, monkeypatch, cid, units=units)


def _good_call():
    """a small net the library takes, right after a refusal: the outputs are right and nothing is pending"""
    case = [c for c in mlp64.SHAPE_CASES if c.id == 'g07-idr0-F0-2x32-o4'][0]
    net = case.build()
    ins, feat, w1 = make_inputs(net, 64, 3)
    ref = Reference(net, ins, feat, w1, grads=False)
    pm = ops.PackedMLP(net.specs, net.act, net.head, net.enc, net.F, DEV)
    pm.pack(*[[t.to(DEV) for t in ts] for ts in zip(*[mlp64.nets.linear_params(net.sd, k) for k in net.keys])])
    out, _, _ = ops.mlp_forward(pm, *[_dev(t) for t in ins], _dev(feat))
    torch.cuda.synchronize()
    assert (out.cpu().double() - ref.r64['out']).abs().max().item() < CAP_OUT


def _refused(net, n=10, feat_width=None):
    """the first entry points a net meets (pack, forward) refuse it through _lib.check"""
    ins, feat, _ = make_inputs(net, n, 2)
    with pytest.raises((RuntimeError, AssertionError), match=r'bad shape|bad argument|assert') as e:
        F_ = net.F if feat_width is None else feat_width
        pm = ops.PackedMLP(net.specs, net.act, net.head, net.enc, F_, DEV, half=False)
        pm.pack(*[[t.to(DEV) for t in ts] for ts in zip(*[mlp64.nets.linear_params(net.sd, k) for k in net.keys])])
        f = _dev(feat)
        if feat_width is not None:
            f = torch.zeros(n, feat_width, device=DEV)
        ops.mlp_forward(pm, *[_dev(t) for t in ins], f)
    print('refused:', e.value)
    torch.cuda.synchronize()
    _good_call()


def test_refusals():
    """nets the header says the library cannot take fail with NEFII_E_SHAPE / NEFII_E_ARG (argument checks: nothing is launched)"""
    from nefii_amd import synthetic as syn
    mk = lambda kind, mc: mlp64.Net(kind, mc, syn.make_state_dict(mc, seed=1))
    for what, net in (
            ('105 encoding columns', mk('rad', mlp64.variant('conf', 'rad', mode='idr', multires_xyz=10, multires_view=6))),
            ('hidden width 576', mk('rad', mlp64.variant('conf', 'rad', dims=[576] * 2))),
            ('513 SDF outputs', mk('sdf', mlp64.variant('neus', 'sdf', feature_vector_size=512)))):
        assert expected_family(net.specs, net.enc, net.F, net.head, net.act) == 'refused', what
        _refused(net)
    # feat_width > k_x of layer 0: the forward is the first entry point that reads it
    net = mk('rad', mlp64.variant('conf', 'rad', dims=[64] * 2, feature_vector_size=64))
    _refused(net, feat_width=128)
    # 13 layers (the Python layer's own assertion may come first: either is a clean refusal)
    mc = mlp64.variant('conf', 'rad', dims=[64] * 12, feature_vector_size=64)
    specs, enc, head = ops.radiance_specs(mc['rendering_network'], 64)
    assert len(specs) == 13 and expected_family(specs, enc, 64, head, ops.ACT_RELU) == 'refused'
    with pytest.raises((RuntimeError, AssertionError)):
        ops.PackedMLP(specs, ops.ACT_RELU, head, enc, 64, DEV)
    torch.cuda.synchronize()
    _good_call()


# ---- SDF nets off the shipped shape -------------------------------------------------------------------------------------
def _build_sdf(net, f16x3):
    pm = ops.PackedMLP(net.specs, net.act, net.head, net.enc, 0, DEV, f16x3=f16x3)
    pm.pack(*[[t.to(DEV) for t in ts] for ts in zip(*[mlp64.nets.linear_params(net.sd, k) for k in net.keys])])
    return pm


@pytest.mark.parametrize('case', mlp64.SDF_CASES, ids=repr)
def test_sdf_variants(case):
    net = case.build()
    args = (net.specs, net.enc, net.F, net.head, net.act)
    streamed, vg_streamed = expected_family(*args) == 'stream', mlp64.expected_value_grad_stream(*args)
    judges = []
    for f16x3 in (False, True):
        pm = _build_sdf(net, f16x3)
        assert (pm.w_stream is not None) == (streamed and f16x3), 'fragment stream: library %s, header %s' % (
            pm.w_stream is not None, streamed and f16x3)
        for n in (1, 65, 3000) + ((20011,) if streamed else ()):
            x = mlp64.ball_points(n, 5 + n)
            (o64, h64, g64), (o32, h32, g32) = mlp64.sdf_reference(net, x)
            xd = x.to(DEV)
            # the streamed kernel's workspace: one slot per hidden layer and workgroup (64-row tiles of 128 KiB at 512 wide,
            # 96-row tiles of 96 KiB at 256 wide, at most 256 workgroups); the generic kernels take n rows per hidden layer
            rows, slot = (64, 128 * 1024) if net.specs[0].n_pad == 512 else (96, 96 * 1024)
            ws = _lib.lib().nefii_sdf_value_grad_workspace_bytes(ctypes.byref(pm.struct), n)
            on_stream = ws == min((n + rows - 1) // rows, 256) * (len(net.specs) - 1) * slot
            assert on_stream == (vg_streamed and f16x3), 'nefii_sdf_value_grad on the stream: library %s, header %s' % (
                on_stream, vg_streamed and f16x3)
            J = Judge('sdf %s n=%d f16x3=%s stream=%s value_grad on stream=%s' % (case.id, n, f16x3, pm.w_stream is not None,
                                                                                 on_stream))
            out, hid, _ = ops.mlp_forward(pm, xd, None, None, None, want_hidden=True)          # the f32-input kernels
            J.maxabs('mlp_forward out', out, o64, o32, floor=mlp64.FLOOR_SDF_VALUE, cap=mlp64.CAP_SDF_F32)
            J.maxabs('mlp_forward hidden', hid, h64, h32, floor=mlp64.FLOOR_SDF_VALUE, cap=mlp64.CAP_SDF_F32)
            cap_v = mlp64.CAP_SDF_SPLIT if f16x3 else mlp64.CAP_SDF_F32
            out2, feat, grad = ops.sdf_value_grad(pm, xd, want_feat=True)
            J.maxabs('value_grad value', out2[:, 0], o64[:, 0], o32[:, 0], floor=mlp64.FLOOR_SDF_VALUE, cap=cap_v)
            J.maxabs('value_grad out', out2, o64, o32, floor=mlp64.FLOOR_SDF_VALUE, cap=mlp64.CAP_SDF_F32)
            J.maxabs('value_grad hidden', feat, h64, h32, floor=mlp64.FLOOR_SDF_VALUE, cap=mlp64.CAP_SDF_F32)
            J.close('value_grad gradient', grad, g64, g32, floor=mlp64.FLOOR_SDF_GRAD, cap=mlp64.CAP_SDF_GRAD_L2)
            if on_stream:
                J.maxabs('value_grad gradient', grad, g64, g32, floor=mlp64.CAP_SDF_GRAD_ABS, cap=mlp64.CAP_SDF_GRAD_ABS)
            if f16x3:
                val = ops.sdf_eval(pm, xd)
                J.maxabs('sdf_eval', val, o64[:, 0], o32[:, 0], floor=mlp64.FLOOR_SDF_VALUE, cap=mlp64.CAP_SDF_SPLIT)
            torch.cuda.synchronize()
            assert all(torch.isfinite(t).all() for t in (out, hid, out2, feat, grad))
            judges.append(J)
    bad = []
    for J in judges:
        try:
            J.done()
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('case', [c for c in mlp64.SDF_CASES if c.wgrad], ids=repr)
def test_sdf_step1_weight_gradients(case):
    """Step-1 parameter gradients of an SDF net off the shipped shape through IDRNetwork.implicit_network (the f32-input
    kernels, skip layers included) for the L1 fit's upstream gradient sign(sdf - target) / n, the sign taken from the fp64 run
    on every side (the L1 kink is the loss's, not the network's)."""
    from nefii_amd import conf
    from nefii_amd.model.implicit_differentiable_renderer import IDRNetwork
    net = case.build()
    n = 2000
    g = torch.Generator().manual_seed(8)
    x = torch.randn(n, 3, generator=g) * 0.5
    target = torch.randn(n, 1, generator=g) * 0.3
    runs = {}
    for dt in (torch.float64, torch.float32):
        sd = {k: v.to(dt).requires_grad_(True) for k, v in net.sd.items()}
        out = mlp64.forward(net, sd, (x.to(dt), None, None), None)[0]
        if dt == torch.float64:
            d = (torch.sign(out[:, :1].detach() - target.double()) / n).float()
        runs[dt] = (out.detach(), dict(zip(sd, torch.autograd.grad((out[:, :1] * d.to(dt)).sum(), list(sd.values())))))
    m = IDRNetwork(conf.from_dict(case.mc))
    m.load_state_dict(case.sd, strict=True)
    inet = m.to(DEV).implicit_network
    inet.train()
    pred = inet(x.to(DEV))
    assert pred.requires_grad
    pred[:, :1].backward(d.to(DEV))
    J = Judge('sdf step-1 %s n=%d' % (case.id, n))
    J.maxabs('value', pred[:, 0], runs[torch.float64][0][:, 0], runs[torch.float32][0][:, 0], floor=mlp64.FLOOR_SDF_VALUE,
             cap=mlp64.CAP_SDF_F32)
    for k, p in inet.named_parameters():
        key = 'implicit_network.' + k
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        J.close(k, p.grad, runs[torch.float64][1][key], runs[torch.float32][1][key], floor=FLOOR_GRAD, cap=mlp64.CAP_SDF_WGRAD)
    J.done()


@pytest.mark.parametrize('precision', ['f32', 'f16x3w'])
@pytest.mark.parametrize('case', [c for c in mlp64.SDF_CASES if c.trace], ids=repr)
def test_tracer_on_variant_nets(case, precision):
    """the tracer on SDF nets off the shipped shape (no skip layer, a skip at layer 1, three hidden layers), eval and training,
    against oracle/tracer.py as test_tracer_vs_oracle_and_counts does, evaluation counts within 1 %"""
    from oracle import nets, tracer
    from trace_cmp import argmin_set, compare_trace, run_gpu_trace
    case.build()
    mc, sd = case.mc, case.sd
    sdf = lambda x: nets.sdf_forward(sd, mc['implicit_network'], x)[:, 0]
    n = 2000
    g = torch.Generator().manual_seed(11)
    o = torch.randn(n, 3, generator=g)
    o = o / o.norm(dim=-1, keepdim=True) * (1.5 + torch.rand(n, 1, generator=g))
    d = torch.randn(n, 3, generator=g) * 0.45 - o
    d = d / d.norm(dim=-1, keepdim=True)
    om = torch.rand(n, generator=g) < 0.8
    steps = torch.rand(100, generator=g)
    for training in (False, True):
        ref = tracer.trace(sdf, o, d, om, mc['ray_tracer'], training, steps)
        got = run_gpu_trace(mc, sd, o, d, om, training, steps, precision)
        print('[tracer %s %s training=%s] hits %d of %d' % (case.id, precision, training, int(ref['hit'].sum()), n))
        compare_trace(sdf, o, d, got, ref['hit'], ref['dists'], (case.id, training, precision), argmin_set(ref['hit'], om, training))
        gpu_evals = ops.algorithmic_evals(got[3].cpu().long(), 100).sum().item()
        c = ref['counters']
        cpu_evals = sum(c.get(k, 0) for k in ('sphere_trace', 'sampler', 'bisect', 'min_sdf'))
        assert abs(gpu_evals - cpu_evals) <= 0.01 * cpu_evals, (gpu_evals, cpu_evals)
