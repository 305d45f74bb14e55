"""fp64 yardstick of the fused-MLP tests (tests/test_mlp64_cpu.py, tests/test_gpu_mlp_shapes.py).

The reference of every kernel output is the plain torch loop below (posenc, nets.linear_params, F.linear - the loop of
oracle/nets.py, which it equals bit for bit on the shipped confs, returning EVERY layer's pre-activation as well) run in
float64 on the fp32 weights and inputs the kernel saw; the same loop in float32 measures the conditioning and sets the bound
as tests/sg64.py does:

    err(gpu, fp64) <= min(cap, max(4 * err(fp32 oracle, fp64), floor))

`cap` is the bound the suite already asserts for that quantity on the shipped shapes (test_gpu_kernels.py) and is never widened.

Kinks.  A ReLU unit (or a RELU / ABS / RELU_INIT head) whose pre-activation lies within DELTA of 0 in fp64 may come out on the
other side in another arithmetic; its gradient then differs by O(1) and that is no error of the kernel.  kink_rows() finds the
rows with such a unit; they get a ZERO upstream gradient on every side (kernel, fp32 oracle, fp64): nothing is dropped from a
comparison and every forward value is still compared.  DELTA = 2e-5 is the suite's own forward bound (6-8 x the fp32 oracle's
pre-activation error).  A case may lose at most MAX_UNSEEDED of its rows this way.  A pre-activation that is EXACTLY 0 (zero
weights and bias) is 0 in every arithmetic and is not a kink: what the kernel does there is compared.

Also here: the case lists both test files iterate over, and expected_family(): the dispatch rules of include/nefii_amd.h
restated."""
import copy
import math

import torch
import torch.nn.functional as F

from nefii_amd import ops, synthetic as syn
from oracle import nets
from sg64 import Judge as _Judge, rel_l2_64

DELTA, MAX_UNSEEDED = 2e-5, 0.20
# floors: 4 x the worst error of the fp32 ORACLE against fp64 over the whole case matrix at 4000 rows (test_mlp64_cpu.py prints
# them: outputs 1.12e-6 rel-L2, parameter gradients 9.3e-7, SDF value 8.4e-7 max-abs, SDF gradient 1.16e-6 rel-L2) - never
# from what a kernel gives, never above the cap.  (sg64's starting values were 2e-6 / 2e-5: the first would have been tighter
# than the fp32 oracle allows, the second above the f32 kernels' cap.)
FLOOR_VALUE, FLOOR_GRAD = 4.5e-6, 3.7e-6
FLOOR_SDF_VALUE, FLOOR_SDF_GRAD = 3.4e-6, 4.6e-6
# caps: what test_gpu_kernels.py asserts on the shipped shapes
CAP_OUT, CAP_STASH = 2e-5, 3e-5
CAP_GRAD = {'f32': 5e-6, 'f16x3-fp32stash': 2.5e-3, 'f16x3': 2.5e-3}
CAP_SDF_SPLIT, CAP_SDF_F32, CAP_SDF_GRAD_L2, CAP_SDF_GRAD_ABS, CAP_SDF_WGRAD = 5e-6, 2e-5, 2e-5, 1e-5, 1e-3
ARITHMETICS = ('f32', 'f16x3-fp32stash', 'f16x3')

ACTS = {'relu': ops.ACT_RELU, 'elu': ops.ACT_ELU, 'softplus100': ops.ACT_SOFTPLUS100}
HEADS = {'none': ops.HEAD_NONE, 'tanh01': ops.HEAD_TANH01, 'pow2': ops.HEAD_POW2, 'sigmoid': ops.HEAD_SIGMOID,
         'relu': ops.HEAD_RELU, 'abs': ops.HEAD_ABS, 'relu_init': ops.HEAD_RELU_INIT}
KINK_HEADS = (ops.HEAD_RELU, ops.HEAD_ABS, ops.HEAD_RELU_INIT)


class Judge(_Judge):
    def maxabs(self, name, got, ref64, ref32, floor=FLOOR_VALUE, cap=CAP_OUT, relative=False):
        """max |got - ref64| (relative=True: over max(1, max |ref64|)) against min(cap, max(4 x the fp32 oracle's, floor))"""
        r = ref64.detach().double().cpu()
        s = max(1.0, r.abs().max().item()) if relative and r.numel() else 1.0
        e = ((got.detach().double().cpu() - r).abs().max().item() / s) if r.numel() else 0.0
        e32 = ((ref32.detach().double().cpu() - r).abs().max().item() / s) if r.numel() else 0.0
        self._row(name, 'max_abs', e, e32, min(cap, max(4.0 * e32, floor)))

    def slices(self, name, got, ref64, ref32, bound):
        """every single column and every single row of a weight gradient against `bound`: a dropped, shifted or mis-ordered
        column is O(1) there and can hide in the whole matrix's norm.  The error of a slice is taken relative to
        max(|slice|, rms |slice| of the matrix): relative to its OWN norm alone the measure is ill-conditioned for the slices
        of nearly dead units (norm 1e-3 ... 1e-5 of the typical one: the fp32 ORACLE is then off by up to 1.6e-4 of such
        a slice where it is within 4e-7 in this measure, and a one-pass fp16 GEMM loses a
        Softplus unit's activation of 1e-9 altogether: 16 h underflows in fp16)."""
        g, r, r32 = (t.detach().double().cpu() for t in (got, ref64, ref32))
        for dim, what in ((0, 'col'), (1, 'row')):
            nrm = r.norm(dim=dim)
            den = torch.maximum(nrm, nrm.pow(2).mean().sqrt()) + 1e-300
            e, e32 = ((g - r).norm(dim=dim) / den).max().item(), ((r32 - r).norm(dim=dim) / den).max().item()
            self._row('%s worst %s' % (name, what), 'rel_l2', e, e32, bound)


def ball_points(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, generator=g)
    return x / x.norm(dim=-1, keepdim=True) * torch.rand(n, 1, generator=g) ** (1 / 3)


# ---- model confs -----------------------------------------------------------------------------------------------------
def variant(name, net='rad', out=None, **changes):
    """syn.model_conf(name) with the block of one net ('rad' rendering_network, 'mat' envmap_material_network, 'sdf'
    implicit_network) overridden: dims, skip_in, multires*, mode (sets d_in: 9 for idr, 6 otherwise; no_view_dir takes
    multires_view = 0 so that syn.make_state_dict sizes layer 0 right), head options, use_last_as_f; feature_vector_size at
    the top level; `out`: the net's output count (material nets: 3 or 4, through roughness_mlp)."""
    mc = syn.model_conf(name)
    if 'feature_vector_size' in changes:
        mc['feature_vector_size'] = int(changes.pop('feature_vector_size'))
    blk = mc[{'rad': 'rendering_network', 'mat': 'envmap_material_network', 'sdf': 'implicit_network'}[net]]
    blk.update(copy.deepcopy(changes))
    if net == 'rad':
        mode = blk.get('mode', 'idr')
        blk['d_in'] = 9 if mode == 'idr' else 6
        if mode == 'no_view_dir':
            blk['multires_view'] = 0
        if out is not None:
            blk['d_out'] = out
    elif net == 'mat' and out is not None:
        assert out in (3, 4)
        blk['roughness_mlp'] = blk['specular_mlp'] = blk['same_mlp'] = out == 4
    elif net == 'sdf' and out is not None:
        blk['d_out'] = out
    return mc


class Net:
    """One MLP as the kernels see it: LayerSpecs, encoders, activation and head ids, and its slice of the state dict."""

    def __init__(self, kind, mc, sd, no_encoder=False, act=None, head=None):
        self.kind, self.mc, self.F = kind, mc, int(mc['feature_vector_size'])
        self.skip, self.last_as_f = (), False
        if kind == 'rad':
            self.cfg, prefix = mc['rendering_network'], 'rendering_network'
            self.specs, self.enc, self.head = ops.radiance_specs(self.cfg, self.F)
            self.act, self.keys = ops.ACT_RELU, ['%s.lin%d' % (prefix, l) for l in range(len(self.specs))]
        elif kind == 'mat':
            self.cfg, prefix = mc['envmap_material_network'], 'envmap_material_network'
            dim_out = 4 if (self.cfg.get('roughness_mlp') and self.cfg.get('same_mlp')) else 3
            self.specs, self.enc = ops.material_specs(self.cfg, self.F, dim_out)
            self.act, self.head = ops.ACT_ELU, ops.HEAD_SIGMOID
            self.keys = ['%s.diffuse_albedo_layers.%d' % (prefix, 2 * l) for l in range(len(self.specs))]
        else:
            self.cfg, prefix = mc['implicit_network'], 'implicit_network'
            self.specs, self.enc = ops.sdf_specs(self.cfg, self.F)
            self.act, self.head = ops.ACT_SOFTPLUS100, ops.HEAD_NONE
            self.keys = ['%s.lin%d' % (prefix, l) for l in range(len(self.specs))]
            self.skip, self.last_as_f = tuple(self.cfg.get('skip_in', ())), bool(self.cfg.get('use_last_as_f', False))
            self.F = 0          # (an SDF net takes no feature block; feature_vector_size sizes its OUTPUT)
        self.act = self.act if act is None else ACTS[act]
        self.head = self.head if head is None else HEADS[head]
        self.sd = {k: v.detach().clone() for k, v in sd.items() if k.startswith(prefix + '.') and any(
            k.startswith(key + '.') for key in self.keys)}
        if no_encoder:       # features only: layer 0 keeps its feature columns (a net ops.PackedMLP takes, no conf describes)
            s0 = self.specs[0]
            for k in list(self.sd):
                if k.startswith(self.keys[0] + '.weight'):
                    w = self.sd[k]
                    self.sd[k] = w[:, s0.x_src0:s0.x_src0 + s0.x_len].contiguous() if w.shape[1] == s0.k_in else w
            self.specs = [ops.LayerSpec(s0.n_out, s0.x_len, x_src0=0, x_len=s0.x_len)] + self.specs[1:]
            self.enc = [-1, -1, -1]
        self.weight_norm = (self.keys[0] + '.weight_g') in self.sd
        self.n_out = self.specs[-1].n_out

    def names(self, l):
        return [self.keys[l] + s for s in (('.weight_v', '.weight_g', '.bias') if self.weight_norm else ('.weight', '.bias'))]

    def scale_last(self, s):
        """last layer's effective weights and bias times s (a power of two: exact)"""
        k = self.keys[-1]
        self.sd[k + ('.weight_g' if self.weight_norm else '.weight')] *= s
        self.sd[k + '.bias'] *= s

    def zero_unit(self, l, u):
        """unit u of layer l gets zero incoming weights and bias (plain weights only: a zero row has no weight-norm)"""
        assert not self.weight_norm
        self.sd[self.keys[l] + '.weight'][u] = 0.
        self.sd[self.keys[l] + '.bias'][u] = 0.

    def plain(self):
        """the same net with plain (effective) weights instead of weight-norm pairs"""
        if self.weight_norm:
            sd = {}
            for k in self.keys:
                w, b = nets.linear_params(self.sd, k)
                sd[k + '.weight'], sd[k + '.bias'] = w.clone(), b.clone()
            self.sd, self.weight_norm = sd, False
        return self


def act_fwd(h, act):
    if act == ops.ACT_RELU:
        return torch.relu(h)
    if act == ops.ACT_ELU:
        return F.elu(h)
    return F.softplus(h, beta=100)


def head_fwd(h, head):
    if head == ops.HEAD_TANH01:
        return (torch.tanh(h) + 1.) / 2.
    if head == ops.HEAD_POW2:
        return h ** 2
    if head == ops.HEAD_SIGMOID:
        return torch.sigmoid(h)
    if head == ops.HEAD_RELU:
        return torch.relu(h)
    if head == ops.HEAD_ABS:
        return torch.abs(h)
    if head == ops.HEAD_RELU_INIT:
        return torch.relu(h) + 0.5
    return h


def forward(net, sd, ins, feat):
    """-> (out [n, n_out], pre: every layer's pre-activation, hidden: the activation entering the last layer, W: the
    effective weights).  sd / ins / feat in ONE dtype; ins = (a, b, c) raw [n, 3] inputs (None where enc < 0)."""
    enc = torch.cat([nets.posenc(x, e) for x, e in zip(ins, net.enc) if e >= 0], dim=-1) if any(
        e >= 0 for e in net.enc) else None
    h = enc if feat is None else (feat if enc is None else torch.cat([enc, feat], dim=-1))
    pre, Ws, hidden = [], [], None
    L = len(net.keys)
    for l, key in enumerate(net.keys):
        if l == L - 1:
            hidden = h
        if l in net.skip:
            h = torch.cat([h, enc], dim=1) / math.sqrt(2)
        w, b = nets.linear_params(sd, key)
        Ws.append(w)
        h = F.linear(h, w, b)
        pre.append(h)
        if l < L - 1:
            h = act_fwd(h, net.act)
    return head_fwd(h, net.head), pre, hidden, Ws


def kink_rows(pre_acts, head_pre, act, head, delta=DELTA):
    """bool [n]: rows with a hidden pre-activation of a ReLU net, or the head pre-activation of a RELU / ABS / RELU_INIT
    head, at 0 < |pre| < delta (fp64 values)"""
    bad = torch.zeros(head_pre.shape[0], dtype=torch.bool)
    near = lambda z: ((z.abs() < delta) & (z != 0)).any(dim=1)
    if act == ops.ACT_RELU:
        for z in pre_acts:
            bad |= near(z)
    if head in KINK_HEADS:
        bad |= near(head_pre)
    return bad


def make_inputs(net, n, seed):
    """(a, b, c) with None where the net has no such input, feat or None, w1 [n, n_out] - fp32, as the existing tests draw them"""
    g = torch.Generator().manual_seed(seed)
    x = ball_points(n, seed + 2)
    u = [F.normalize(torch.randn(n, 3, generator=g), dim=-1) for _ in range(2)]
    feat = torch.randn(n, net.F, generator=g) * 0.3 if net.F > 0 else None
    w1 = torch.rand(n, net.n_out, generator=g)
    raw = [x, u[0], u[1]]
    return tuple(raw[i] if net.enc[i] >= 0 else None for i in range(3)), feat, w1


class Reference:
    """fp64 and fp32 runs of one net on one batch: outputs, pre-activations, the rows un-seeded at kinks, and the parameter
    gradients (by state-dict key, plus 'dW%d' = the gradient of layer l's EFFECTIVE weight) for the upstream gradient
    w1 * gs with those rows zeroed."""

    def __init__(self, net, ins, feat, w1, gs=1.0, grads=True):
        self.runs = {}
        for dt in (torch.float64, torch.float32):
            sd = {k: v.detach().to(dt).requires_grad_(grads) for k, v in net.sd.items()}
            cast = lambda t: None if t is None else t.to(dt)
            out, pre, hidden, Ws = forward(net, sd, tuple(cast(t) for t in ins), cast(feat))
            if dt == torch.float64:
                self.kink = kink_rows([p.detach() for p in pre[:-1]], pre[-1].detach(), net.act, net.head)
                self.d_out = (w1 * gs).masked_fill(self.kink.unsqueeze(1), 0.)        # fp32: what the kernel gets
                self.peak_head_pre = pre[-1].detach().abs().max().item()
            g = {}
            if grads:
                leaves = list(sd.values()) + (Ws if net.weight_norm else [])
                got = torch.autograd.grad((out * self.d_out.to(dt)).sum(), leaves)
                g = dict(zip(list(sd.keys()) + (['dW%d' % l for l in range(len(Ws))] if net.weight_norm else []), got))
                if not net.weight_norm:
                    g.update({'dW%d' % l: g[k + '.weight'] for l, k in enumerate(net.keys)})
            self.runs[dt] = dict(out=out.detach(), pre=[p.detach() for p in pre], hidden=hidden.detach(), grads=g)
        self.r64, self.r32 = self.runs[torch.float64], self.runs[torch.float32]
        self.unseeded = self.kink.float().mean().item()


# ---- dispatch, restated from include/nefii_amd.h --------------------------------------------------------------------------
def expected_family(specs, enc, F_, head, act):
    """'refused' | 'generic' | 'stream' | 'stream+h16': what the header promises for a net of these LayerSpecs.
    refused: more than 12 layers, a padded width above 512, encodings above 96 padded columns, a feature block wider than
    layer 0's.  Feature nets (nefii_mlp_stream_bytes / nefii_mlp_h16_supported): every hidden layer 512 wide, no skip layer,
    at most 8 outputs, at least one hidden layer -> the streamed kernels forward and, with transposed fragments (which
    ops.PackedMLP always packs for a trainable net), backward with the state in halves.  SDF nets (Softplus, one encoder, no
    features; nefii_sdf_stream_bytes): every hidden layer 512 or 256 wide, layer inputs of 0 or W previous features plus 0 or
    64 encoding columns, a W-deep last layer without encoding columns -> 'stream'."""
    if len(specs) > 12 or any(max(s.k_x, s.n_pad) > 512 or s.k_e > 96 for s in specs):
        return 'refused'
    if sum(3 + 6 * e for e in enc if e >= 0) > 96 or F_ > specs[0].k_x:
        return 'refused'
    hid, last = specs[:-1], specs[-1]
    if not hid:
        return 'generic'
    if act == ops.ACT_SOFTPLUS100 and F_ == 0 and enc[0] >= 0 and enc[1] < 0 and enc[2] < 0 and head == ops.HEAD_NONE:
        W = hid[0].n_pad
        ok = W in (512, 256) and all(s.n_pad == W and s.k_x in (0, W) and s.k_e in (0, 64) for s in hid)
        return 'stream' if ok and last.k_x == W and last.k_e == 0 else 'generic'
    ok = all(s.n_pad == 512 for s in hid) and all(s.k_e == 0 and s.k_x == 512 for s in specs[1:]) and last.n_out <= 8
    return 'stream+h16' if ok else 'generic'


def expected_value_grad_stream(specs, enc, F_, head, act):
    """nefii_sdf_value_grad runs on the stream: a streamed SDF net with at least TWO hidden layers whose layer 0 reads 64
    encoding columns"""
    return expected_family(specs, enc, F_, head, act) == 'stream' and len(specs) >= 3 and specs[0].k_e == 64


# ---- the cases -------------------------------------------------------------------------------------------------------------
ENCODINGS = {     # name -> (net, conf changes, no_encoder)
    'idr': ('rad', dict(mode='idr', multires_xyz=10, multires_view=4), False),                # 93 columns
    'nvd': ('rad', dict(mode='no_view_dir', multires_xyz=10), False),                         # 66
    'nn': ('rad', dict(mode='no_normal', multires_xyz=10, multires_view=4), False),           # 90
    'idr0': ('rad', dict(mode='idr', multires_xyz=0, multires_view=0), False),                # 9
    'radnone': ('rad', dict(mode='idr', multires_xyz=0, multires_view=0), True),              # no encoder at all
    'm10': ('mat', dict(multires=10), False),                                                 # 63
    'm0': ('mat', dict(multires=0), False),                                                   # 3
    'matnone': ('mat', dict(multires=0), True),
}


class Case:
    def __init__(self, cid, base, encoding, F_, dims, out, ns, misaligned=False, act=None, head=None, scaled=False,
                 shipped_hidden=None, seed=1):
        self.id, self.base, self.encoding, self.F, self.dims, self.out, self.ns = cid, base, encoding, F_, dims, out, ns
        self.misaligned, self.act, self.head, self.scaled, self.shipped_hidden, self.seed = (
            misaligned, act, head, scaled, shipped_hidden, seed)

    def build(self):
        kind, changes, no_enc = ENCODINGS[self.encoding]
        if self.shipped_hidden is not None:          # a shipped conf as it stands (test_radiance_and_material_mlp's cases)
            mc = syn.model_conf(self.base, hidden=self.shipped_hidden if self.shipped_hidden != 512 else None)
        else:
            mc = variant(self.base, kind, out=self.out, dims=list(self.dims), feature_vector_size=self.F, **changes)
        net = Net(kind, mc, syn.make_state_dict(mc, seed=self.seed), no_encoder=no_enc, act=self.act, head=self.head)
        if self.scaled:         # the power of two that brings the largest head pre-activation of the fp64 run into 15 ... 30
            ins, feat, w1 = make_inputs(net, 4000, self.seed + 4)
            peak = Reference(net, ins, feat, w1, grads=False).peak_head_pre
            net.scale_last(2.0 ** math.ceil(math.log2(15.0 / peak)))
        return net

    def __repr__(self):
        return self.id


def _c(cid, base, encoding, F_, dims, out, ns, **kw):
    return Case(cid, base, encoding, F_, dims, out, ns, **kw)


# 3a - the shape matrix: a covering list.  Streamed: every hidden layer 512 wide and at most 8 outputs.
SHAPE_CASES = [
    # the five cases of test_radiance_and_material_mlp, radiance and material net each
    _c('physg-h64-rad', 'physg', 'idr', 0, [64] * 4, 3, (500,), shipped_hidden=64),
    _c('physg-h64-mat', 'physg', 'm10', 0, [64] * 4, 3, (500,), shipped_hidden=64),
    _c('conf-h64-rad', 'conf', 'idr', 64, [64] * 4, 3, (301,), shipped_hidden=64),
    _c('conf-h64-mat', 'conf', 'm10', 64, [64] * 8, 4, (301,), shipped_hidden=64),
    _c('conf-h512-rad', 'conf', 'idr', 512, [512] * 4, 3, (200, 3000), shipped_hidden=512),
    _c('conf-h512-mat', 'conf', 'm10', 512, [512] * 8, 4, (200, 3000), shipped_hidden=512),
    _c('physg-h512-rad', 'physg', 'idr', 0, [512] * 4, 3, (64,), shipped_hidden=512),
    _c('physg-h512-mat', 'physg', 'm10', 0, [512] * 4, 3, (64,), shipped_hidden=512),
    # streamed variants (k = k_x + k_e of layer 0)
    _c('s01-nvd-F32-1x512-o1', 'physg', 'nvd', 32, [512] * 1, 1, (1, 20011)),              # k 128
    _c('s02-nn-F100-2x512-o8', 'conf', 'nn', 100, [512] * 2, 8, (63, 20011)),              # k 224, scalar staging, zero fill
    _c('s03-idr0-F256-4x512-o4', 'physg', 'idr0', 256, [512] * 4, 4, (64, 20011)),         # k 288
    _c('s04-m0-F512-8x512-o3', 'physg', 'm0', 512, [512] * 8, 3, (65, 20011)),             # k 544
    _c('s05-m10-F100-11x512-o4', 'conf', 'm10', 100, [512] * 11, 4, (300, 1000)),          # k 192, the deepest net
    _c('s06-m10-F32-1x512-o3', 'physg', 'm10', 32, [512] * 1, 3, (1, 20011)),              # k 96
    _c('s07-radnone-F512-2x512-o3', 'conf', 'radnone', 512, [512] * 2, 3, (63, 20011)),    # k 512, no encoder
    _c('s08-idr-F512off-4x512-o3', 'conf', 'idr', 512, [512] * 4, 3, (64, 1000), misaligned=True),
    _c('s09-m10-F512off-2x512-o4', 'conf', 'm10', 512, [512] * 2, 4, (65, 300), misaligned=True),
    _c('s10-idr-F0-8x512-o8', 'physg', 'idr', 0, [512] * 8, 8, (300, 1000)),               # k 96
    _c('s11-m0-F0-2x512-o3', 'physg', 'm0', 0, [512] * 2, 3, (1000, 20011)),               # k 32
    _c('s12-nvd-F256-11x512-o1', 'conf', 'nvd', 256, [512] * 11, 1, (63, 65)),             # k 352
    _c('s13-idr0-F100-8x512-o4', 'conf', 'idr0', 100, [512] * 8, 4, (1, 64)),              # k 160
    _c('s14-matnone-F256-4x512-o3', 'physg', 'matnone', 256, [512] * 4, 3, (300, 20011)),  # k 256, no encoder
    _c('s15-nn-F0-1x512-o3', 'physg', 'nn', 0, [512] * 1, 3, (64, 65)),                    # k 96
    # 9 outputs at 512 wide: must leave the streamed family and still be right
    _c('s16-idr-F32-4x512-o9', 'conf', 'idr', 32, [512] * 4, 9, (300, 1000)),
    _c('s17-nvd-F512-2x512-o9', 'physg', 'nvd', 512, [512] * 2, 9, (63, 1000)),
    # generic widths
    _c('g01-idr-F256-4x256-o3', 'conf', 'idr', 256, [256] * 4, 3, (1, 20011)),
    _c('g02-m10-F100-3x256-o4', 'conf', 'm10', 100, [256] * 3, 4, (63, 20011)),            # the reference's own material default
    _c('g03-nvd-F32-2x128-o1', 'physg', 'nvd', 32, [128] * 2, 1, (64, 300)),
    _c('g04-m0-F0-8x128-o3', 'physg', 'm0', 0, [128] * 8, 3, (65, 1000)),
    _c('g05-nn-F100-1x64-o8', 'conf', 'nn', 100, [64] * 1, 8, (1, 65)),
    _c('g06-m10-F512-4x64-o4', 'conf', 'm10', 512, [64] * 4, 4, (300, 1000)),
    _c('g07-idr0-F0-2x32-o4', 'physg', 'idr0', 0, [32] * 2, 4, (63, 64)),
    _c('g08-m10-F32-11x32-o3', 'physg', 'm10', 32, [32] * 11, 3, (65, 300)),
    _c('g09-idr-F512-mixed-o3', 'conf', 'idr', 512, [512, 256, 128], 3, (1, 1000)),
    _c('g10-m0-F256-mixed-o4', 'conf', 'm0', 256, [512, 256, 128], 4, (64, 300)),
    _c('g11-idr-F100-2x320-o4', 'physg', 'idr', 100, [320] * 2, 4, (63, 1000)),
    _c('g12-m10-F0-4x320-o3', 'physg', 'm10', 0, [320] * 4, 3, (1, 65)),
    _c('g13-radnone-F256-2x256-o8', 'conf', 'radnone', 256, [256] * 2, 8, (64, 300)),
    _c('g14-idr-F512off-2x64-o1', 'conf', 'idr', 512, [64] * 2, 1, (65, 1000), misaligned=True),
    _c('g15-m10-F512off-1x128-o4', 'conf', 'm10', 512, [128] * 1, 4, (63, 300), misaligned=True),
]

# 3b - every activation x head pair on one streamed and one generic shape, unscaled and with the last layer scaled up
HEAD_CASES = [
    _c('%s-%s-%s%s' % (tag, act, head, '-scaled' if scaled else ''), 'conf', 'idr', F_, dims, 3, (300,), act=act, head=head,
       scaled=scaled)
    for tag, F_, dims in (('stream4x512', 512, [512] * 4), ('generic2x64', 64, [64] * 2))
    for act in ACTS for head in HEADS for scaled in (False, True)]


def zero_cases():
    """3c - (id, net builder): conventions at exact zero.  Plain weights (a zero row has no weight-norm)."""
    out = []
    for tag, F_, dims in (('stream4x512', 512, [512] * 4), ('generic2x64', 64, [64] * 2)):
        for head in ('relu', 'relu_init', 'abs', 'pow2'):
            def build(F_=F_, dims=dims, head=head):
                net = _c('', 'conf', 'idr', F_, dims, 3, (300,), head=head).build().plain()
                net.zero_unit(len(dims), 1)             # output column 1: pre-activation exactly 0
                return net, [(len(dims), 1)]
            out.append(('%s-head-%s' % (tag, head), build))

        def build_hidden(F_=F_, dims=dims):
            net = _c('', 'conf', 'idr', F_, dims, 3, (300,)).build().plain()
            units = [(0, 5), (len(dims) - 1, dims[-1] - 1)]
            for l, u in units:
                net.zero_unit(l, u)
            return net, units
        out.append(('%s-hidden-unit' % tag, build_hidden))
    return out


class SdfCase:
    def __init__(self, cid, base, changes, F_=None, trace=False, wgrad=False):
        self.id, self.base, self.changes, self.F, self.trace, self.wgrad = cid, base, changes, F_, trace, wgrad

    def build(self, seed=3):
        kw = dict(self.changes)
        if self.F is not None:
            kw['feature_vector_size'] = self.F
        mc = variant(self.base, 'sdf', **kw)
        L = mc['implicit_network'].get('multires', 0)
        # (weights on the sin / cos columns as the existing tests draw them for 6 octaves, scaled down for more so that the
        # field's slope stays what it is there: the last octave's frequency doubles with each)
        damp = min(1.0, 2.0 ** (6 - L))
        sd = syn.make_state_dict(mc, seed=seed, bumpy=0.004 * damp)
        g = torch.Generator().manual_seed(11)
        d0 = 3 + 6 * L
        for l in mc['implicit_network']['skip_in']:       # live sin / cos columns at every skip layer, as after training
            if d0 > 3:
                w = sd['implicit_network.lin%d.weight_v' % l]
                w[:, -(d0 - 3):] = torch.randn(w.shape[0], d0 - 3, generator=g) * 0.02 * damp
        net = Net('sdf', mc, sd)
        # (the live columns lift the whole field above zero: the output bias is shifted so that 30 % of the unit ball lies
        # inside the surface again - a tracer has something to hit, and values near zero are where absolute bounds bite)
        with torch.no_grad():
            val = forward(net, {k: v.double() for k, v in net.sd.items()}, (ball_points(2000, 1).double(), None, None), None)[0]
            net.sd[net.keys[-1] + '.bias'][0] -= val[:, 0].quantile(0.3).float()
            sd[net.keys[-1] + '.bias'] = net.sd[net.keys[-1] + '.bias'].clone()
        self.mc, self.sd = mc, sd
        return net

    def __repr__(self):
        return self.id


SDF_CASES = [
    SdfCase('8x512-noskip', 'physg', dict(skip_in=[]), trace=True, wgrad=True),
    SdfCase('8x512-skip1', 'physg', dict(skip_in=[1]), trace=True, wgrad=True),
    SdfCase('8x512-skip7', 'physg', dict(skip_in=[7])),
    SdfCase('8x512-skip2-5', 'physg', dict(skip_in=[2, 5]), wgrad=True),
    SdfCase('2x512-skip1', 'physg', dict(dims=[512] * 2, skip_in=[1])),
    SdfCase('1x512', 'physg', dict(dims=[512], skip_in=[])),
    SdfCase('3x512-pe10-lastf', 'conf', dict(dims=[512] * 3, skip_in=[], multires=10, use_last_as_f=True), trace=True),
    SdfCase('11x512-skip4', 'physg', dict(dims=[512] * 11, skip_in=[4])),
    SdfCase('8x512-pe5', 'physg', dict(multires=5)),
    SdfCase('8x512-pe4', 'physg', dict(multires=4)),
    SdfCase('8x512-pe0', 'physg', dict(multires=0)),
    SdfCase('8x256-F256', 'neus', dict(dims=[256] * 8), F_=256),
    SdfCase('4x256-skip2-pe10-F100', 'neus', dict(dims=[256] * 4, skip_in=[2], multires=10), F_=100),
    SdfCase('8x128', 'physg', dict(dims=[128] * 8)),
    SdfCase('8x512-skip8-output', 'physg', dict(skip_in=[8])),
]


def sdf_reference(net, x):
    """fp64 / fp32: (out [n, 1 + F or 1], last hidden, d out[:, 0] / dx)"""
    res = {}
    for dt in (torch.float64, torch.float32):
        sd = {k: v.to(dt) for k, v in net.sd.items()}
        xr = x.to(dt).requires_grad_(True)
        out, _, hidden, _ = forward(net, sd, (xr, None, None), None)
        grad = torch.autograd.grad(out[:, 0].sum(), xr)[0]
        res[dt] = (out.detach(), hidden.detach(), grad)
    return res[torch.float64], res[torch.float32]
