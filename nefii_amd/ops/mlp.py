"""The fused MLP - packing, forward, backward, weight gradients, autograd - and SDF evaluation and calibration."""
import ctypes
import math
import os

import torch

from .. import _lib
from .._lib import HEAD_ABS, HEAD_NONE, HEAD_POW2, HEAD_RELU, HEAD_RELU_INIT, HEAD_TANH01, Mlp
from ._call import _f32, _pad_hidden, _ptr, _round32, call


class LayerSpec:
    """How one nn.Linear [n_out, k_in] maps onto the kernel's [X | E] input blocks."""

    def __init__(self, n_out, k_in, x_src0=0, x_len=0, e_src0=0, e_len=0, scale=1.0):
        self.n_out, self.k_in = n_out, k_in
        self.x_src0, self.x_len, self.e_src0, self.e_len, self.scale = x_src0, x_len, e_src0, e_len, scale
        self.k_x, self.k_e, self.n_pad = _pad_hidden(x_len), _round32(e_len), _pad_hidden(n_out)


class PackedMLP:
    """Device-resident packed weights + the nefii_mlp descriptor of one fused MLP."""

    def __init__(self, specs, act, head, enc_freqs, feat_width, device, need_bwd=True, f16x3=False, half=False):
        """half: the MLP runs on the fp16-MFMA kernels (nefii_mlp_forward_f16 / _backward_f16 / _wgrad_f16; radiance and
        material networks, never the SDF network) - implies the fp16 fragment sets.  True / 'f16x3': split-precision
        forward, single-pass backward and weight gradients; 'f16': everything in one fp16 pass."""
        assert 1 <= len(specs) <= _lib.MAX_LAYERS
        self.half = half if half in ('f16', 'f16x3') else ('f16x3' if half else False)
        f16x3 = f16x3 or bool(self.half)
        self.specs = specs
        self.act, self.head = act, head
        self.enc_freqs = list(enc_freqs)
        self.feat_width = feat_width
        self.device = device
        self.need_bwd = need_bwd
        self.w_fwd, self.w_bwd, self.bias, self.w_f16, self.w_f16b = [], [], [], [], []
        self.f16x3 = f16x3
        m = Mlp()
        m.n_layers, m.act, m.head, m.feat_width = len(specs), act, head, feat_width
        for i in range(3):
            m.enc_freqs[i] = self.enc_freqs[i]
        for l, s in enumerate(specs):
            k = s.k_x + s.k_e
            # nets on the fp16-MFMA kernels never get their f32 fragments packed (pack(): skip_f32) - they are not allocated
            # and the descriptor carries NULL, so that an f32 entry point called on such a net returns NEFII_E_ARG instead of
            # computing with zero weights
            self.w_fwd.append(None if self.half else torch.zeros(k * s.n_pad, device=device, dtype=torch.float32))
            self.w_bwd.append(torch.zeros(k * s.n_pad, device=device, dtype=torch.float32)
                              if need_bwd and not self.half else None)
            self.bias.append(torch.zeros(s.n_pad, device=device, dtype=torch.float32))
            self.w_f16.append(torch.zeros(2 * k * s.n_pad, device=device, dtype=torch.float16) if f16x3 else None)
            self.w_f16b.append(torch.zeros(2 * k * s.n_pad, device=device, dtype=torch.float16)
                               if f16x3 and need_bwd else None)
            L = m.layer[l]
            L.k_x, L.k_e, L.n_out, L.n_pad = s.k_x, s.k_e, s.n_out, s.n_pad
            L.w_fwd = self.w_fwd[l].data_ptr() if self.w_fwd[l] is not None else None
            L.w_bwd = self.w_bwd[l].data_ptr() if self.w_bwd[l] is not None else None
            L.bias = self.bias[l].data_ptr()
            L.w_f16x3 = self.w_f16[l].data_ptr() if f16x3 else None
            L.w_bwd_f16x3 = self.w_f16b[l].data_ptr() if self.w_f16b[l] is not None else None
        self.struct = m
        # SDF nets of the qualifying shape also keep their hidden layers as one fragment stream per wave (the
        # pipelined tile evaluator of the tracer); other nets leave w_stream NULL and run on the generic kernel
        self.w_stream = None
        if f16x3 and not self.half and torch.device(device).type == 'cuda':
            # stream layout / matrix instruction of the pipelined evaluator: 0 = 32x32x16 (512-wide nets only),
            # 1 = 16x16x32 (512- and 256-wide nets)
            m.reserved = int(os.environ.get('NEFII_STREAM_LAYOUT', '1'))
            nbytes = _lib.lib().nefii_sdf_stream_bytes(ctypes.byref(m))
            if nbytes and feat_width == 0 and self.enc_freqs[1] < 0 and self.enc_freqs[2] < 0:
                self.w_stream = torch.zeros(nbytes // 2, device=device, dtype=torch.float16)
                m.w_stream = self.w_stream.data_ptr()
            else:
                m.reserved = 0
        # radiance / material nets with 512-wide hidden layers: the split-precision forward reads the hidden layers as a
        # fragment stream too (nefii_mlp_forward_f16 on 48- / 64-row tiles); re-packed with the weights every pack()
        self.mlp_stream = False
        if self.half == 'f16x3' and torch.device(device).type == 'cuda':
            nbytes = _lib.lib().nefii_mlp_stream_bytes(ctypes.byref(m))
            if nbytes:
                self.w_stream = torch.zeros(nbytes // 2, device=device, dtype=torch.float16)
                m.w_stream = self.w_stream.data_ptr()
                self.mlp_stream = True
        self.hidden_stride = max(s.n_pad for s in specs)
        self.packed_version = None

    @property
    def n_layers(self):
        return len(self.specs)

    @property
    def in_width(self):
        return self.specs[0].k_in

    def pack(self, weights, biases):
        """weights[l]: effective [n_out, k_in] fp32 GPU tensors (after weight-norm), biases[l]: [n_out]."""
        # every layer and every form in ONE launch (nefii_pack_mlp); the fp16-MFMA kernels (self.half) never read the
        # f32 fragments, so those are skipped there
        src = (_lib.PackSource * len(self.specs))()
        keep = []                               # converted copies must outlive the launch call
        for l, s in enumerate(self.specs):
            w = _f32(weights[l])
            b = _f32(biases[l])
            keep += [w, b]
            assert tuple(w.shape) == (s.n_out, s.k_in), (tuple(w.shape), s.n_out, s.k_in)
            e = src[l]
            e.W, e.bias = _ptr(w), _ptr(b)
            e.n_out, e.k_in, e.x_src0, e.x_len, e.e_src0, e.e_len = s.n_out, s.k_in, s.x_src0, s.x_len, s.e_src0, s.e_len
            e.scale, e.skip_f32 = s.scale, 1 if self.half else 0
        call('nefii_pack_mlp', ctypes.byref(self.struct), src)
        if self.w_stream is not None:
            call('nefii_pack_mlp_stream' if self.mlp_stream else 'nefii_pack_sdf_stream', ctypes.byref(self.struct),
                 _ptr(self.w_stream))


def mlp_precision():
    """Arithmetic of the radiance / material MLPs (NEFII_MLP_PRECISION): 'f16x3' (default) - fp16 MFMA tiles: forward in
    split precision (hi/lo pairs, fp32-class accuracy), backward and weight gradients in one fp16 pass with a
    power-of-two gradient scale; 'f16' - the forward in one fp16 pass too (measured 1.3e-3 relative L2 on config 3's RGB:
    above the north-star bar, for measurement only); 'f32' - the f32-input MFMA kernels (bit-exact fp32 fma chains)."""
    return os.environ.get('NEFII_MLP_PRECISION', 'f16x3')


def h16_supported(pm):
    """The net trains with its stash and dz kept in halves (nefii_mlp_*_f16h: streamed kernels forward and backward).
    NEFII_MLP_H16=0 keeps the fp32 stash (A/B measurements)."""
    if pm.half != 'f16x3' or os.environ.get('NEFII_MLP_H16', '1') == '0':
        return False
    if getattr(pm, '_h16', None) is None:        # a property of the net's shape and buffers, not of its weights
        pm._h16 = bool(_lib.lib().nefii_mlp_h16_supported(ctypes.byref(pm.struct)))
    return pm._h16


def param_list(module):
    """list(module.parameters()), gathered once per module: the Parameter OBJECTS of the networks here are fixed at
    construction (weight_norm included; load_state_dict / .to() / optimizers write in place), and Module.parameters() walks
    the module tree on every call - the per-step version / requires_grad checks cost 0.09 ms of config 1's 0.81-ms host step."""
    plist = module.__dict__.get('_nefii_plist')
    if plist is not None:
        # ... but nothing stops a caller from REPLACING them (load_state_dict(assign=True), remove_weight_norm, to_empty):
        # the version / requires_grad checks would then watch dead objects and serve stale packed weights.  Cheap guard on
        # every call - the first parameter is still the first (next() stops at the first leaf) - and a full identity
        # check every 256th.
        n = module.__dict__['_nefii_plist_calls'] = module.__dict__.get('_nefii_plist_calls', 0) + 1
        first = next(module.parameters(), None)
        if (plist[0] if plist else None) is not first:
            plist = None
        elif n % 256 == 0:
            cur = list(module.parameters())
            if len(cur) != len(plist) or any(a is not b for a, b in zip(cur, plist)):
                plist = None
    if plist is None:
        plist = module.__dict__['_nefii_plist'] = list(module.parameters())
    return plist


class HalfStash:
    """What nefii_mlp_forward_f16h leaves for the backward pass: h [n_layers - 1, n, stride] halves (16 x the hidden
    activations), z_last [n, 8] floats (pre-activations of the head), x0 [n, nefii_mlp_x0_width] halves (16 x layer 0's
    input in the kernel's column order: padded features, then the encodings)."""

    def __init__(self, h, z_last, x0):
        self.h, self.z_last, self.x0 = h, z_last, x0


def mlp_forward(pm, in_a, in_b, in_c, feat, want_hidden=False, want_stash=False, h16=None):
    """(out, last hidden or None, stash or None).  The stash is a HalfStash where the net supports it (h16=False: the fp32
    [n_layers, n, stride] tensor regardless), else fp32."""
    lib = _lib.lib()
    n = in_a.shape[0]
    dev = in_a.device
    n_out = pm.specs[-1].n_out
    out = torch.empty(n, n_out, device=dev, dtype=torch.float32)
    hidden = None
    if want_hidden:
        hidden = torch.empty(n, pm.specs[-2].n_out, device=dev, dtype=torch.float32)
    stash = None
    if want_stash and n > 0 and h16 is not False and h16_supported(pm):
        stash = HalfStash(torch.empty(pm.n_layers - 1, n, pm.hidden_stride, device=dev, dtype=torch.float16),
                          torch.empty(n, 8, device=dev, dtype=torch.float32),
                          torch.empty(n, lib.nefii_mlp_x0_width(ctypes.byref(pm.struct)), device=dev, dtype=torch.float16))
        call('nefii_mlp_forward_f16h', ctypes.byref(pm.struct), _ptr(in_a), _ptr(in_b), _ptr(in_c), _ptr(feat), n, _ptr(out),
             n_out, _ptr(hidden), hidden.shape[1] if hidden is not None else 0, _ptr(stash.h), pm.hidden_stride,
             _ptr(stash.z_last), _ptr(stash.x0))
        return out, hidden, stash
    if want_stash:
        stash = torch.empty(pm.n_layers, n, pm.hidden_stride, device=dev, dtype=torch.float32)
    if n > 0:
        args = (ctypes.byref(pm.struct), _ptr(in_a), _ptr(in_b), _ptr(in_c), _ptr(feat), n, _ptr(out), n_out, _ptr(hidden),
                hidden.shape[1] if hidden is not None else 0, _ptr(stash), pm.hidden_stride)
        if pm.half:
            call('nefii_mlp_forward_f16', *args, 1 if pm.half == 'f16' else 0)
        else:
            call('nefii_mlp_forward', *args)
    return out, hidden, stash


def mlp_backward(pm, d_out, stash, gscale=None):
    """gscale (pm.half): device scalar from mlp_grad_scale(d_out)"""
    n = d_out.shape[0]
    if isinstance(stash, HalfStash):        # dz comes back in halves too: gscale x dz_l
        dz = torch.empty(pm.n_layers, n, pm.hidden_stride, device=d_out.device, dtype=torch.float16)
        call('nefii_mlp_backward_f16h', ctypes.byref(pm.struct), _ptr(d_out), d_out.shape[1], _ptr(stash.h), pm.hidden_stride,
             _ptr(stash.z_last), n, _ptr(dz), pm.hidden_stride, _ptr(gscale))
        return dz
    dz = torch.empty(pm.n_layers, n, pm.hidden_stride, device=d_out.device, dtype=torch.float32)
    if n > 0:
        args = (ctypes.byref(pm.struct), _ptr(d_out), d_out.shape[1], _ptr(stash), pm.hidden_stride, n, _ptr(dz), pm.hidden_stride)
        if pm.half:
            call('nefii_mlp_backward_f16', *args, _ptr(gscale))
        else:
            call('nefii_mlp_backward', *args)
    return dz


def mlp_grad_scale(d_out):
    """power-of-two scale that brings max |d_out| to ~256 (device scalar; the fp16 backward GEMMs carry dz x scale)"""
    s = torch.empty(1, device=d_out.device, dtype=torch.float32)
    call('nefii_mlp_grad_scale', _ptr(d_out), d_out.numel(), _ptr(s))
    return s


def mlp_backward_scale(pm, d_out, stash):
    """the gradient scale FusedMLPFn.backward uses: mlp_grad_scale(d_out), and for a POW2 head - whose derivative 2 |pre| is
    unbounded - nefii_mlp_grad_scale_head on the head's pre-activations the forward left (identical while |2 pre| < 8)"""
    if pm.head != HEAD_POW2 or d_out.shape[0] == 0:
        return mlp_grad_scale(d_out)
    pre = stash.z_last if isinstance(stash, HalfStash) else stash[pm.n_layers - 1]
    s = torch.empty(1, device=d_out.device, dtype=torch.float32)
    call('nefii_mlp_grad_scale_head', _ptr(d_out), d_out.shape[1], _ptr(pre), pre.shape[1], d_out.shape[0], d_out.shape[1],
         pm.head, _ptr(s))
    return s


def encode_inputs(pm, in_a, in_b, in_c, feat):
    n = in_a.shape[0]
    out = torch.empty(n, pm.in_width, device=in_a.device, dtype=torch.float32)
    if n > 0:
        call('nefii_encode_inputs', ctypes.byref(pm.struct), _ptr(in_a), _ptr(in_b), _ptr(in_c), _ptr(feat), n, _ptr(out),
             pm.in_width)
    return out


def _stash_tensors(stash, like):
    if stash is None:
        return (like.new_empty(0),)
    return (stash.h, stash.z_last, stash.x0) if isinstance(stash, HalfStash) else (stash,)


def _image_to_linear_columns(lib, s0, g_img):
    """layer 0's weight gradient in the h16 input image's column order (features | encodings, each padded) -> the Linear's"""
    kx = lib.nefii_padded_width(s0.x_len)
    parts = sorted([(s0.x_src0, g_img[:, :s0.x_len]), (s0.e_src0, g_img[:, kx:kx + s0.e_len])], key=lambda t: t[0])
    return torch.cat([t[1] for t in parts if t[1].shape[1]], dim=1)


class FusedMLPFn(torch.autograd.Function):
    """y = MLP(PE(a), PE(b), PE(c), feat); differentiable wrt the layer weights and biases only
    (the raw inputs come from frozen geometry: IDRNetwork.freeze_geometry, Step-2; in the Step-1 geometry fit the inputs
    are sample positions)."""

    @staticmethod
    def forward(ctx, pm, in_a, in_b, in_c, feat, *wb):
        L = pm.n_layers
        ws, bs = wb[:L], wb[L:]
        pm.pack(ws, bs)
        need = any(t.requires_grad for t in wb)
        out, _, stash = mlp_forward(pm, in_a, in_b, in_c, feat, want_stash=need)
        ctx.pm = pm
        ctx.save_for_backward(in_a, in_b if in_b is not None else in_a.new_empty(0),
                              in_c if in_c is not None else in_a.new_empty(0),
                              feat if feat is not None else in_a.new_empty(0), *_stash_tensors(stash, in_a))
        ctx.has = (in_b is not None, in_c is not None, feat is not None)
        # an output that nothing differentiable reads (physg.conf weights the radiance colour with 0 and the loss detaches it)
        # may still be reachable in the autograd graph through a node it shares with other outputs (AssembleRowsFn): its
        # backward then arrives with None and must not run on materialised zeros
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, d_out):
        pm = ctx.pm
        if d_out is None:
            return (None,) * (5 + 2 * pm.n_layers)
        in_a, in_b, in_c, feat, *st = ctx.saved_tensors
        stash = HalfStash(*st) if len(st) == 3 else st[0]
        h16 = isinstance(stash, HalfStash)
        in_b = in_b if ctx.has[0] else None
        in_c = in_c if ctx.has[1] else None
        feat = feat if ctx.has[2] else None
        L = pm.n_layers
        d_out = d_out.contiguous()
        gscale = mlp_backward_scale(pm, d_out, stash) if pm.half else None
        dz = mlp_backward(pm, d_out, stash, gscale)
        lib = _lib.lib()
        n = d_out.shape[0]
        # layer 0's input: the image the h16 forward left (no encoded matrix to rebuild), else the Linear's own columns
        x0 = stash.x0 if h16 else encode_inputs(pm, in_a, in_b, in_c, feat)

        def operands():
            """per layer (spec, dz_l, x_l, x_l's row stride, k, dW_l [n_out, k], db_l) of dW_l = scale * dz_l^T x_l"""
            for l, s in enumerate(pm.specs):
                if l == 0:
                    xin, xs = x0, x0.shape[1]
                elif not h16 and s.e_len:
                    # skip layer: its input is [previous activations | encoded network input] (the 1/sqrt(2) is s.scale)
                    # in the Linear's column order (x_src0 / e_src0 are column offsets into its weight)
                    blocks = [stash[l - 1][:, :s.x_len], x0[:, :s.e_len]]
                    xin = torch.cat(blocks if s.x_src0 < s.e_src0 else blocks[::-1], dim=1).contiguous()
                    xs = xin.shape[1]
                else:
                    xin, xs = (stash.h if h16 else stash)[l - 1], pm.hidden_stride
                k = xs if l == 0 and h16 else s.k_in
                yield (s, dz[l], xin, xs, k, torch.empty(s.n_out, k, device=d_out.device, dtype=torch.float32),
                       torch.empty(s.n_out, device=d_out.device, dtype=torch.float32))

        ops = operands()        # (lazily: the per-layer calls build a skip layer's input right before they read it)
        batch = h16 and n > 0 and os.environ.get('NEFII_WGRAD_BATCH', '1') != '0'
        if batch:
            # every layer's weight gradient in one zero-fill + one launch per kernel form: the per-layer calls below are 2 L
            # dependent launches in the step's tail
            ops = list(ops)
            items = (_lib.WgradItem * L)(*[_lib.WgradItem(_ptr(dz_l), _ptr(xin), _ptr(g), _ptr(b), pm.hidden_stride, xs, 1,
                                                         s.n_out, k, s.scale) for s, dz_l, xin, xs, k, g, b in ops])
            call('nefii_mlp_wgrad_f16h_batch', items, L, n, _ptr(gscale))
        gw, gb = [], []
        for s, dz_l, xin, xs, k, g, b in ops:
            if not batch:
                gemm = (_ptr(dz_l), pm.hidden_stride, _ptr(xin), xs) + ((1,) if h16 else ()) + (n, s.n_out, k, s.scale)
                if pm.half:
                    call('nefii_mlp_wgrad_f16h' if h16 else 'nefii_mlp_wgrad_f16', *gemm, _ptr(gscale), _ptr(g), _ptr(b))
                else:
                    call('nefii_mlp_wgrad', *gemm, _ptr(g), _ptr(b))
            gw.append(_image_to_linear_columns(lib, s, g) if h16 and s is pm.specs[0] else g)
            gb.append(b)
        return (None, None, None, None, None) + tuple(gw) + tuple(gb)


class FusedMLPHiddenFn(torch.autograd.Function):
    """FusedMLPFn that also returns the last hidden activation (ImplicitNetwork with use_last_as_f) as a
    non-differentiable output: the Step-1 fit consumes the SDF column only."""

    @staticmethod
    def forward(ctx, pm, in_a, *wb):
        L = pm.n_layers
        pm.pack(wb[:L], wb[L:])
        need = any(t.requires_grad for t in wb)
        out, hidden, stash = mlp_forward(pm, in_a, None, None, None, want_hidden=True, want_stash=need)
        ctx.pm = pm
        empty = in_a.new_empty(0)
        ctx.save_for_backward(in_a, empty, empty, empty, *_stash_tensors(stash, in_a))
        ctx.has = (False, False, False)
        ctx.mark_non_differentiable(hidden)
        ctx.set_materialize_grads(False)
        return out, hidden

    @staticmethod
    def backward(ctx, d_out, _d_hidden):
        g = FusedMLPFn.backward(ctx, d_out)
        return g[:2] + g[5:]


def sdf_value_grad(pm, x, want_feat=False):
    """(sdf_out [n, n_out_last], feature [n, hidden] or None, d sdf/dx [n,3])."""
    lib = _lib.lib()
    n = x.shape[0]
    dev = x.device
    n_out = pm.specs[-1].n_out
    out = torch.empty(n, n_out, device=dev, dtype=torch.float32)
    grad = torch.empty(n, 3, device=dev, dtype=torch.float32)
    feat = torch.empty(n, pm.specs[-2].n_out, device=dev, dtype=torch.float32) if want_feat else None
    if n > 0:
        nbytes = lib.nefii_sdf_value_grad_workspace_bytes(ctypes.byref(pm.struct), n)
        ws = torch.empty(nbytes // 4, device=dev, dtype=torch.float32)
        call('nefii_sdf_value_grad', ctypes.byref(pm.struct), _ptr(x), n, _ptr(out), n_out, _ptr(feat),
             feat.shape[1] if feat is not None else 0, _ptr(grad), _ptr(ws))
    return out, feat, grad


def sdf_eval(pm, x, coarse=False, fp8=False):
    """implicit_network(x)[:, 0] with the tracer's split-precision tile evaluator (needs PackedMLP(f16x3=True));
    coarse=True: with its single-pass (one fp16 MFMA per product) evaluator instead; fp8=True: with the "16f" evaluator
    (correction products on block-scaled fp8, nefii_tracer_params.split_fp8)."""
    x = x.contiguous()
    n = x.shape[0]
    out = torch.empty(n, device=x.device, dtype=torch.float32)
    if n > 0:
        name = 'nefii_sdf_eval_fp8corr' if fp8 else 'nefii_sdf_eval_coarse' if coarse else 'nefii_sdf_eval'
        call(name, ctypes.byref(pm.struct), _ptr(x), n, _ptr(out))
    return out


def fp8corr_supported(pm):
    return bool(pm.f16x3 and pm.w_stream is not None and _lib.lib().nefii_sdf_fp8corr_supported(ctypes.byref(pm.struct)))


def coarse_supported(pm):
    return bool(pm.f16x3 and pm.w_stream is not None and _lib.lib().nefii_sdf_coarse_supported(ctypes.byref(pm.struct)))


COARSE_TAU_SAFETY = 3.0


def calibrate_coarse_tau(pm, radius=1.0, n=65536, safety=COARSE_TAU_SAFETY, seed=0):
    """Error bound of the tracer's coarse pass for THIS network: `safety` x the largest |single-pass - split| SDF value
    over n points drawn uniformly in the bounding sphere (where the tracer samples), at least 1e-4.  0.0 when the net
    has no single-pass stream.  One host sync; callers cache it per packed weight version (geometry is frozen)."""
    if not coarse_supported(pm):
        return 0.0
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, generator=g)
    x = x / x.norm(dim=1, keepdim=True) * (torch.rand(n, 1, generator=g) ** (1.0 / 3.0)) * (radius * 1.02)
    x = x.to(pm.device)
    err = (sdf_eval(pm, x, coarse=True) - sdf_eval(pm, x)).abs().max().item()
    if not math.isfinite(err):
        return 0.0
    return max(1e-4, safety * err)


LIPSCHITZ_SAFETY = 1.5


def calibrate_lipschitz(grad_fn, device, radius=1.0, n=65536, safety=LIPSCHITZ_SAFETY, seed=1, search_rounds=4):
    """Bound on |sdf(p) - sdf(q)| / |p - q| inside the bounding sphere for THIS network, for the tracer's staged searches
    (nefii_tracer_params.minsdf_lipschitz): `safety` x the largest |grad sdf| found, at least 1.  Found by n points drawn
    uniformly in the sphere, then `search_rounds` rounds of local search around the 256 steepest points so far (255 Gaussian
    perturbations each, radius shrinking from 0.04: the steep spots of a softplus-100 network are small - the search typically
    raises the random sample's maximum by a few percent).  grad_fn: points [n, 3] -> gradients [n, 3] (ImplicitNetwork.gradient).
    Like coarse_tau a MEASURED bound, not a proven one; the tracer audits it (_lib.CNT_LIP_AUDIT).  One host sync; cached per
    packed weight version."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, generator=g)
    x = x / x.norm(dim=1, keepdim=True) * (torch.rand(n, 1, generator=g) ** (1.0 / 3.0)) * (radius * 1.02)
    x = x.to(device)
    gn = grad_fn(x).reshape(-1, 3).norm(dim=1)
    sigma = 0.04 * radius
    for _ in range(search_rounds):
        top = torch.topk(gn, min(256, gn.numel())).indices
        seeds, best = x[top], gn[top]
        pert = torch.randn(seeds.shape[0], 255, 3, generator=g).to(device) * sigma
        cand = (seeds.unsqueeze(1) + pert).reshape(-1, 3)
        rn = cand.norm(dim=1, keepdim=True)
        cand = torch.where(rn > radius * 1.02, cand * (radius * 1.02 / rn), cand)        # stay inside the sphere
        x = torch.cat([seeds, cand])
        gn = torch.cat([best, grad_fn(cand).reshape(-1, 3).norm(dim=1)])
        sigma *= 0.5
    gmax = gn.max().item()
    if not math.isfinite(gmax):
        return 0.0
    return max(1.0, safety * gmax)


# ---- descriptors of the reference's three networks ------------------------------------------------
def sdf_specs(cfg, feature_vector_size):
    """LayerSpec list for ImplicitNetwork (implicit_differentiable_renderer.py:18-83)."""
    dims = list(cfg['dims'])
    L = int(cfg.get('multires', 0))
    d0 = 3 + 6 * L
    if cfg.get('use_last_as_f', False):
        full = [d0] + dims + [cfg['d_out']]
    else:
        full = [d0] + dims + [cfg['d_out'] + feature_vector_size]
    skip = tuple(cfg.get('skip_in', ()))
    specs = []
    prev_out = None
    for l in range(len(full) - 1):
        n_out = full[l + 1] - d0 if (l + 1) in skip else full[l + 1]
        if l == 0:
            specs.append(LayerSpec(n_out, d0, e_src0=0, e_len=d0))
        elif l in skip:
            specs.append(LayerSpec(n_out, prev_out + d0, x_src0=0, x_len=prev_out, e_src0=prev_out, e_len=d0,
                                   scale=1.0 / math.sqrt(2)))
        else:
            specs.append(LayerSpec(n_out, prev_out, x_src0=0, x_len=prev_out))
        prev_out = n_out
    return specs, [L, -1, -1]


def radiance_specs(cfg, feature_vector_size):
    """RenderingNetwork (implicit_differentiable_renderer.py:126-241): layer 0 eats cat[PE(x), PE(v), n, feat]."""
    mode = cfg.get('mode', 'idr')
    Lv, Lx = int(cfg.get('multires_view', 0)), int(cfg.get('multires_xyz', 0))
    if mode == 'idr':
        enc = [Lx, Lv, 0]
    elif mode == 'no_view_dir':
        enc = [Lx, 0, -1]
    elif mode == 'no_normal':
        enc = [Lx, Lv, -1]
    else:
        raise ValueError(mode)
    ew = sum(3 + 6 * e for e in enc if e >= 0)
    dims = [ew + feature_vector_size] + list(cfg['dims']) + [cfg['d_out']]
    specs = [LayerSpec(dims[1], dims[0], x_src0=ew, x_len=feature_vector_size, e_src0=0, e_len=ew)]
    for l in range(1, len(dims) - 1):
        specs.append(LayerSpec(dims[l + 1], dims[l], x_src0=0, x_len=dims[l]))
    if cfg.get('normalize_output', True):
        head = HEAD_TANH01
    elif not cfg.get('clip_output', False):
        head = HEAD_NONE
    else:
        head = {'relu': HEAD_RELU, 'abs': HEAD_ABS, 'relu_init': HEAD_RELU_INIT, 'pow2': HEAD_POW2}[
            cfg.get('clip_method', 'relu')]
    return specs, enc, head


def material_specs(cfg, feature_vector_size, dim_out):
    """EnvmapMaterialNetwork.diffuse_albedo_layers (sg_envmap_material.py:92-103): cat[PE(x), feat] -> ELU MLP."""
    Lx = int(cfg.get('multires', 0))
    ew = 3 + 6 * Lx
    dims = [ew + feature_vector_size] + list(cfg['dims']) + [dim_out]
    specs = [LayerSpec(dims[1], dims[0], x_src0=ew, x_len=feature_vector_size, e_src0=0, e_len=ew)]
    for l in range(1, len(dims) - 1):
        specs.append(LayerSpec(dims[l + 1], dims[l], x_src0=0, x_len=dims[l]))
    return specs, [Lx, -1, -1]
