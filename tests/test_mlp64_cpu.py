"""The fp64 yardstick of the MLP tests (tests/mlp64.py) checked on the CPU: its forward equals oracle/nets.py bit for bit, and
for EVERY case of the GPU matrix (tests/test_gpu_mlp_shapes.py iterates over the same lists) the fp32 oracle, with the same
rows un-seeded at kinks, agrees with fp64 far inside the bounds the kernels are held to - which is what guarantees that a
correct kernel can meet them."""
import pytest
import torch

import mlp64
from mlp64 import Net, Reference, expected_family, expected_value_grad_stream, make_inputs, rel_l2_64
from nefii_amd import ops, synthetic as syn
from oracle import nets

ROWS = 4000


@pytest.mark.parametrize('name', ['physg', 'conf', 'neus'])
def test_forward_equals_the_oracle_bit_for_bit(name):
    mc = syn.model_conf(name)
    sd = {k: v.double() for k, v in syn.make_state_dict(mc, seed=1).items()}
    n = 257
    rad, mat, sdf = Net('rad', mc, sd), Net('mat', mc, sd), Net('sdf', mc, sd)
    (x, v, nrm), feat, _ = make_inputs(rad, n, 5)
    x, v, nrm = x.double(), v.double(), nrm.double()
    feat = None if feat is None else feat.double()
    out, pre, hidden, _ = mlp64.forward(rad, sd, (x, v, nrm), feat)
    assert torch.equal(out, nets.radiance_forward(sd, mc['rendering_network'], x, nrm, v, feat))
    assert len(pre) == len(rad.specs) and torch.equal(mlp64.head_fwd(pre[-1], rad.head), out)
    out, pre, _, _ = mlp64.forward(mat, sd, (x, None, None), feat)
    ref = nets.material_forward(sd, mc['envmap_material_network'], x, feat)
    # (the oracle applies the sigmoid to column slices, whose strided kernel rounds the last bit differently from the
    # contiguous one: the pre-activations are what is bit-identical, the head applied the oracle's way proves it)
    assert torch.equal(torch.sigmoid(pre[-1][..., :3]), ref['sg_diffuse_albedo'])
    assert (out[:, :3] - ref['sg_diffuse_albedo']).abs().max().item() < 3e-16
    if out.shape[1] == 4:
        assert torch.equal((1 - nets.TINY_ROUGHNESS) * torch.sigmoid(pre[-1][..., 3:4]) + nets.TINY_ROUGHNESS,
                           ref['sg_roughness'])
    out, pre, hidden, _ = mlp64.forward(sdf, sd, (x, None, None), None)
    ref = nets.sdf_forward(sd, mc['implicit_network'], x)
    if sdf.last_as_f:
        assert torch.equal(torch.cat([out, hidden], dim=-1), ref)
    else:
        assert torch.equal(out, ref)
    (r64, _) = mlp64.sdf_reference(sdf, x.float())
    assert torch.equal(r64[2], nets.sdf_gradient(sd, mc['implicit_network'], x))


def test_kink_rows_rule():
    z = torch.tensor([[1., -1.], [1e-5, 3.], [0., 2.], [-1.9e-5, 0.], [2e-5, 1.]], dtype=torch.float64)
    big = torch.ones(5, 1, dtype=torch.float64)
    assert mlp64.kink_rows([z], big, ops.ACT_RELU, ops.HEAD_NONE).tolist() == [False, True, False, True, False]
    assert not mlp64.kink_rows([z], big, ops.ACT_ELU, ops.HEAD_POW2).any()          # only ReLU nets have hidden kinks
    assert mlp64.kink_rows([big], z[:, :1], ops.ACT_ELU, ops.HEAD_ABS).tolist() == [False, True, False, True, False]
    assert not mlp64.kink_rows([big], z[:, :1], ops.ACT_ELU, ops.HEAD_TANH01).any()


def _check(case):
    """ROWS rows for every case: the fp32 oracle's rounding error of a gradient SUM does fall with the number of rows (measured:
    Softplus-100 on the 4 x 512 shape 1.2e-6 at 300 rows and 4.1e-7 at 4000; the scaled last layer's weight_g 5.2e-6 at 300 and
    8.5e-7 at 4000), so the bounds below - figures for the population - are asserted where they were measured, at 4000 rows,
    also for the cases the GPU runs at fewer; the share of un-seeded rows is a condition on the rows the GPU test really
    uses and is asserted at every row count of the case."""
    net = case.build()
    for n in case.ns:
        ins, feat, w1 = make_inputs(net, n, case.seed + 4 + n)
        share = Reference(net, ins, feat, w1, grads=False).unseeded
        assert share <= mlp64.MAX_UNSEEDED, 'n = %d: un-seeded share %.3f' % (n, share)
    n = ROWS
    ins, feat, w1 = make_inputs(net, n, case.seed + 4)
    ref = Reference(net, ins, feat, w1)
    assert ref.unseeded <= mlp64.MAX_UNSEEDED, 'un-seeded share %.3f' % ref.unseeded
    worst = max(rel_l2_64(ref.r32['grads'][k], ref.r64['grads'][k]) for k in ref.r64['grads'])
    e_out = rel_l2_64(ref.r32['out'], ref.r64['out'])
    e_pre = max([(a.double() - b).abs().max().item() for a, b in zip(ref.r32['pre'][:-1], ref.r64['pre'][:-1])] or [0.])
    print('[%s] n %d un-seeded %.3f  fp32 oracle: gradients %.2e  outputs %.2e  hidden pre-activations %.2e' % (
        case.id, n, ref.unseeded, worst, e_out, e_pre))
    assert torch.isfinite(ref.r64['out']).all() and all(torch.isfinite(g).all() for g in ref.r64['grads'].values())
    assert worst <= (4e-6 if case.scaled else 1e-6), worst
    assert e_out <= (4e-6 if case.scaled else 2e-6), e_out
    if case.scaled:
        assert 15.0 * 0.95 <= ref.peak_head_pre < 30.0 * 1.3, ref.peak_head_pre    # (another batch than the one that chose the scale)


@pytest.mark.parametrize('case', mlp64.SHAPE_CASES, ids=repr)
def test_shape_case_is_reachable(case):
    _check(case)
    net = case.build()
    fam = expected_family(net.specs, net.enc, net.F, net.head, net.act)
    assert fam == ('stream+h16' if case.id.startswith(('s0', 's10', 's11', 's12', 's13', 's14', 's15', 'conf-h512',
                                                       'physg-h512')) else 'generic'), fam


@pytest.mark.parametrize('case', mlp64.HEAD_CASES, ids=repr)
def test_head_case_is_reachable(case):
    _check(case)


@pytest.mark.parametrize('cid,build', mlp64.zero_cases(), ids=[c[0] for c in mlp64.zero_cases()])
def test_zero_case_is_not_a_kink(cid, build):
    net, units = build()
    ins, feat, w1 = make_inputs(net, 300, 9)
    ref = Reference(net, ins, feat, w1)
    assert ref.unseeded <= mlp64.MAX_UNSEEDED
    for l, u in units:      # exactly 0 in both arithmetics, zero gradient rows by torch's convention
        for r in (ref.r64, ref.r32):
            assert not r['pre'][l][:, u].any()
            assert not r['grads']['dW%d' % l][u].any() and not r['grads'][net.keys[l] + '.bias'][u].any()
    worst = max(rel_l2_64(ref.r32['grads'][k], ref.r64['grads'][k]) for k in ref.r64['grads'])
    assert worst <= 1e-6, worst


@pytest.mark.parametrize('case', mlp64.SDF_CASES, ids=repr)
def test_sdf_case_builds_and_crosses_zero(case):
    net = case.build()
    x = mlp64.ball_points(ROWS, 5)
    (o64, h64, g64), (o32, h32, g32) = mlp64.sdf_reference(net, x)
    assert o64[:, 0].min().item() < 0 < o64[:, 0].max().item(), (o64[:, 0].min().item(), o64[:, 0].max().item())
    e = (o32[:, 0].double() - o64[:, 0]).abs().max().item()
    print('[sdf %s] value range %.3f ... %.3f, fp32 oracle: value %.2e max-abs, gradient %.2e rel-L2' % (
        case.id, o64[:, 0].min().item(), o64[:, 0].max().item(), e, rel_l2_64(g32, g64)))
    assert e <= 5e-6 / 4 and rel_l2_64(g32, g64) <= 2e-5 / 4


def test_expected_family_on_the_shipped_nets():
    for name, rad, mat, sdf in (('physg', 'stream+h16', 'stream+h16', 'stream'), ('conf', 'stream+h16', 'stream+h16', 'stream'),
                                ('neus', 'stream+h16', 'stream+h16', 'stream')):
        mc = syn.model_conf(name)
        sd = syn.make_state_dict(mc, seed=0)
        for kind, want in (('rad', rad), ('mat', mat), ('sdf', sdf)):
            net = Net(kind, mc, sd)
            assert expected_family(net.specs, net.enc, net.F, net.head, net.act) == want, (name, kind)
            if kind == 'sdf':
                assert expected_value_grad_stream(net.specs, net.enc, net.F, net.head, net.act)
        small = syn.model_conf(name, hidden=64)
        for kind in ('rad', 'mat', 'sdf'):
            net = Net(kind, small, syn.make_state_dict(small, seed=0))
            assert expected_family(net.specs, net.enc, net.F, net.head, net.act) == 'generic', (name, kind)
    want = {'8x512-noskip': (1, 1), '8x512-skip1': (1, 1), '8x512-skip7': (1, 1), '8x512-skip2-5': (1, 1), '2x512-skip1': (1, 1),
            '1x512': (1, 0), '3x512-pe10-lastf': (1, 1), '11x512-skip4': (1, 1), '8x512-pe5': (1, 1), '8x512-pe4': (0, 0),
            '8x512-pe0': (0, 0), '8x256-F256': (1, 1), '4x256-skip2-pe10-F100': (1, 1), '8x128': (0, 0),
            '8x512-skip8-output': (0, 0)}
    for case in mlp64.SDF_CASES:
        net = case.build()
        args = (net.specs, net.enc, net.F, net.head, net.act)
        assert (expected_family(*args) == 'stream', expected_value_grad_stream(*args)) == tuple(bool(v) for v in want[case.id]), case.id
    # refusals of the header
    specs, enc, head = ops.radiance_specs(mlp64.variant('conf', 'rad', multires_xyz=10, multires_view=6)['rendering_network'], 512)
    assert expected_family(specs, enc, 512, head, ops.ACT_RELU) == 'refused'
    specs, enc, head = ops.radiance_specs(mlp64.variant('conf', 'rad', dims=[576] * 2)['rendering_network'], 512)
    assert expected_family(specs, enc, 512, head, ops.ACT_RELU) == 'refused'
    specs, enc, head = ops.radiance_specs(mlp64.variant('conf', 'rad', dims=[64] * 12)['rendering_network'], 512)
    assert expected_family(specs, enc, 512, head, ops.ACT_RELU) == 'refused'
