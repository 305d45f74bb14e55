"""fp64 yardstick of the kernels that open and close the training step (tests/test_tail64_cpu.py, tests/test_gpu_step_tail.py):
nefii_idr_loss, nefii_prepare_hits, nefii_assemble_rows / nefii_gather_rows, nefii_material_head_global and nefii_camera_rays.

Every reference is plain torch on the CPU in float64, run on the fp32 values the kernel saw:
  loss           IDRLoss with fused = False (pinned to the reference's loss by tests/test_loss_cpu.py): six terms, two gradients
  prepare_hits   x / (|x| + 1e-6) and the gathers
  rows           fill + index_put, and autograd through them; copies and sums of lattice values, so bit-exact in any order
  material head  sigmoid, the 0.089 blend, 0.16 s^2 and the warm-up flags, autograd for the backward
  camera         oracle.renderer.camera_rays
The same reference in float32 measures the conditioning, and the bound is the project's rule (sg64.Judge prints every figure)

    err(gpu, fp64) <= min(cap, max(4 * err(fp32 reference, fp64), floor))

cap: what the suite asserted for the quantity before this file (loss terms 2e-5, loss gradients 1e-5, prepare_hits 2e-7
absolute, camera directions 3e-7 absolute, material head 1e-6 of max(1, |ref|max)).  Floors, from the arithmetic:
  loss terms       sums of non-negative fp32 terms accumulated in double, divided once in fp32: 5e-7 relative
  loss gradients   PER ELEMENT, max |got - ref| / |ref| over ref != 0 (weight * slope / denominator: three roundings);
                   where ref == 0 the result must be exactly 0: 5e-7
  unit vectors     at most 8 roundings of numbers <= 1: 5e-7 absolute (moot under the tighter caps, kept for the record)
  material head    at most 8 roundings (expf included) of numbers <= 1: 5e-7 of max(1, |ref|max).  That measure sees nothing of
                   a gradient near saturation (4.5e-5 at 10, 1e-13 at 30), so every output is ALSO judged per element,
                   relatively, with no cap and the floor 5e-7 + 2e-7 / (1 - sigmoid(p)) for the gradients: s = 1 / (1 + e)
                   carries at most 1.5 ulp(1) ~ 1e-7 of absolute error, 1 - s is then exact, so its relative error is that
                   over 1 - s (3e-3 at 10); the rest is the usual 8 roundings.  At 30 fp32 has sigmoid = 1 and the gradient
                   exactly 0 against 1e-13: the fp32 reference is wrong by all of it, and a kernel passes with 0 or with
                   whatever one ulp(1) of 1 - s gives (6e-8 times the weights) - not with 1e-6.  Zeros of the reference
                   (warm-up flags, an output that takes no part) must be exact zeros.
No comparison leaves a row or an element out: fp32 subtraction is sign-exact and both SmoothL1 branches agree at |d| = 1,
so there is no kink allowance.

fp32 reference against fp64 over the case lists below (tests/test_tail64_cpu.py prints the table; worst per quantity):
  loss terms 1.5e-7 (mask_loss of n1024-none_in; bound 6.2e-7 there) | loss gradients per element 1.7e-7 (d_sg of
  r2-n4096-smooth; bound 6.7e-7 there), exact zeros exact in every case | prepare_hits 1.4e-7 | camera directions 1.4e-7
  | material head 4.9e-8
so the floors decide for the loss (4 x the fp32 figure passes 5e-7 in four rows of the table, by a third at the most) and
the caps for the unit vectors.  No floor was raised.

The module also holds the case lists both test files iterate over."""
import math

import torch

import sg64
from nefii_amd.model.loss import IDRLoss
from oracle import renderer as orr

FLOOR, FACTOR = 5e-7, 4.0
CAP_TERM, CAP_GRAD, CAP_HITS, CAP_CAMERA, CAP_HEAD = 2e-5, 1e-5, 2e-7, 3e-7, 1e-6
TERMS = ('loss', 'idr_rgb_loss', 'sg_rgb_loss', 'mask_loss', 'normalsmooth_loss', 'background_rgb_loss')


def _d(t):
    return t.detach().double().cpu()


def per_element(got, ref):
    """(max |got - ref| / |ref| over ref != 0, elements with ref == 0 and got != 0)"""
    got, ref = _d(got).reshape(-1), _d(ref).reshape(-1)
    nz = ref != 0
    rel = ((got[nz] - ref[nz]).abs() / ref[nz].abs()).max().item() if bool(nz.any()) else 0.0
    return rel, int((got[~nz] != 0).sum().item())


class Judge(sg64.Judge):
    """sg64.Judge with the three error measures of this file"""

    def term(self, name, got, ref64, ref32, floor=FLOOR, cap=CAP_TERM):
        got, ref64, ref32 = float(got), float(ref64), float(ref32)
        if ref64 == 0.0:
            self.require(name, got == 0.0, 'exact zero expected, got %r' % got)
            return
        e, e32 = abs(got - ref64) / abs(ref64), abs(ref32 - ref64) / abs(ref64)
        self._row(name, 'rel', e, e32, min(cap, max(FACTOR * e32, floor)))

    def elements(self, name, got, ref64, ref32, floor=FLOOR, cap=CAP_GRAD):
        assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
        (e, wrong), (e32, _) = per_element(got, ref64), per_element(ref32, ref64)
        self._row(name, 'elem', e, e32, min(cap, max(FACTOR * e32, floor)))
        self.require(name + ' zeros', wrong == 0, '%d elements are not 0 where the reference is exactly 0' % wrong)

    def absolute(self, name, got, ref64, ref32, floor=FLOOR, cap=CAP_HITS, scaled=False):
        assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
        s = max(1.0, _d(ref64).abs().max().item()) if scaled and ref64.numel() else 1.0
        e = (_d(got) - _d(ref64)).abs().max().item() / s if ref64.numel() else 0.0
        e32 = (_d(ref32) - _d(ref64)).abs().max().item() / s if ref64.numel() else 0.0
        self._row(name, 'abs', e, e32, min(cap, max(FACTOR * e32, floor)))

    def same_bits(self, name, got, ref):
        ok = got.shape == ref.shape and got.dtype == ref.dtype and torch.equal(got.cpu(), ref.cpu())
        self.require(name, ok, 'bit-exact' if ok else 'differs from the reference (shape %s / %s)' % (tuple(got.shape), tuple(ref.shape)))


# ---- loss ------------------------------------------------------------------------------------------------------------
def _lc(name, n, r_patch, loss_type, env, masks, bg_w=0.0, idr_w=1.0, ns_w=0.0, alpha=50.0, sdf_scale=0.05, normals='random',
        form='plain'):
    return dict(name=name, n=n, r_patch=r_patch, loss_type=loss_type, env_loss_type=env, masks=masks, bg_w=bg_w, idr_w=idr_w,
                ns_w=ns_w, alpha=alpha, sdf_scale=sdf_scale, normals=normals, form=form)


# masks: random | none_in (no ray in both masks) | all_in | no_outside (no ray outside both) | all_outside |
# no_whole_patch (r_patch >= 1: every patch has a ray that is not in both)
LOSS_CASES = [
    _lc('n1-all_in', 1, -1, 'L1', 'L1', 'all_in'),
    _lc('n1-all_outside', 1, -1, 'L2', 'L2', 'all_outside', bg_w=0.5),
    _lc('n3-random', 3, -1, 'L1_smooth', 'L1', 'random', bg_w=0.3),
    _lc('n1023-idr0', 1023, -1, 'L1', 'L2', 'random', bg_w=0.5, idr_w=0.0),
    _lc('n1024-none_in', 1024, -1, 'L2', 'L1', 'none_in', bg_w=1.0),
    _lc('n1025-no_outside-a1600', 1025, -1, 'L1_smooth', 'L2', 'no_outside', bg_w=0.3, alpha=1600.0, sdf_scale=1.0),
    _lc('n4100-a1600-thin', 4100, -1, 'L1', 'L1', 'random', alpha=1600.0, sdf_scale=0.05),
    _lc('n4100-a50-thick', 4100, -1, 'L1', 'L2', 'random', bg_w=0.3, alpha=50.0, sdf_scale=1.0),
    _lc('n4100-all_in', 4100, -1, 'L1_smooth', 'L1', 'all_in', bg_w=0.5),
    _lc('n4100-all_outside', 4100, -1, 'L1_smooth', 'L2', 'all_outside', bg_w=1.0),
    _lc('n4100-f64-strided', 4100, -1, 'L2', 'L2', 'random', bg_w=0.5, form='f64_strided'),
    _lc('r1-n4-all_in', 4, 1, 'L1', 'L1', 'all_in', ns_w=0.1, normals='smooth'),
    _lc('r1-n4-no_whole_patch', 4, 1, 'L2', 'L2', 'no_whole_patch', ns_w=0.1, bg_w=0.5),
    _lc('r1-n1024-smooth', 1024, 1, 'L1_smooth', 'L2', 'random', bg_w=0.3, ns_w=0.2, normals='smooth'),
    _lc('r1-n4100-a1600', 4100, 1, 'L2', 'L1', 'random', bg_w=1.0, ns_w=0.05, alpha=1600.0, sdf_scale=1.0),
    _lc('r1-n4100-no_whole_patch', 4100, 1, 'L1', 'L2', 'no_whole_patch', bg_w=0.5, ns_w=0.1, normals='smooth'),
    _lc('r2-n16-all_in', 16, 2, 'L1', 'L1', 'all_in', ns_w=0.1, normals='smooth'),
    _lc('r2-n4096-smooth', 4096, 2, 'L1_smooth', 'L2', 'random', bg_w=0.3, idr_w=0.7, ns_w=0.05, normals='smooth'),
    _lc('r2-n4096-ns0', 4096, 2, 'L2', 'L2', 'random', bg_w=0.5, ns_w=0.0),
    _lc('r1-n80000', 80000, 1, 'L1_smooth', 'L1', 'random', bg_w=0.5, ns_w=0.1, alpha=1600.0, sdf_scale=1.0, normals='smooth'),
]
LOSS_BY_NAME = {c['name']: c for c in LOSS_CASES}

# offsets (idr - gt, sg - gt) of the planted rows, on the 2^-10 lattice the planted gt sits on: d == 0 and |d| == 1 exactly
PLANTED = ((0., 1.), (1., 0.), (-1., 0.), (0., -1.), (0., 0.), (1., -1.))
PLANT_EVERY = 7


def planted_rows(n):
    return torch.arange(0, n, PLANT_EVERY)


def loss_kwargs(case):
    return dict(idr_rgb_weight=case['idr_w'], sg_rgb_weight=1.0, eikonal_weight=0.1, mask_weight=100.0, alpha=case['alpha'],
                r_patch=case['r_patch'], normalsmooth_weight=case['ns_w'], loss_type=case['loss_type'],
                env_loss_type=case['env_loss_type'], background_rgb_weight=case['bg_w'])


def loss_inputs(case):
    """the fp32 tensors of one case on the CPU, as the model hands them over: bool masks, gt [1, n, 3], sdf [n, 1]"""
    n, r = case['n'], case['r_patch']
    g = torch.Generator().manual_seed(1000 + 7 * n + 3 * max(r, 0) + len(case['name']))
    idr, sg, gt = torch.rand(n, 3, generator=g) * 1.6, torch.rand(n, 3, generator=g) * 2.5, torch.rand(n, 3, generator=g)
    rows = planted_rows(n)
    lattice = torch.randint(0, 1025, (rows.numel(), 3), generator=g).float() / 1024.
    off = torch.tensor(PLANTED)[torch.arange(rows.numel()) % len(PLANTED)]
    gt[rows] = lattice
    idr[rows] = lattice + off[:, 0:1]
    sg[rows] = lattice + off[:, 1:2]
    net, obj = torch.rand(n, generator=g) < 0.4, torch.rand(n, generator=g) < 0.7
    k = 4 * r * r if r >= 1 else 1
    kind = case['masks']
    if kind == 'random' and r >= 1:             # some whole patches inside both masks
        net.view(-1, k)[::3] = True
        obj.view(-1, k)[::3] = True
    elif kind == 'none_in':
        obj = ~net & (torch.rand(n, generator=g) < 0.5)
    elif kind == 'all_in':
        net[:], obj[:] = True, True
    elif kind == 'no_outside':
        obj = obj | ~net
    elif kind == 'all_outside':
        net[:], obj[:] = False, False
    elif kind == 'no_whole_patch':
        p = torch.arange(n // k)
        net[:] = True
        obj.view(-1, k)[p, p % k] = False
        net.view(-1, k)[p[::2], (p[::2] + 1) % k] = False
    if case['normals'] == 'smooth':             # what a trained surface gives: unit normals that move by 1e-3 inside a patch
        base = torch.nn.functional.normalize(torch.randn(n // k, 1, 3, generator=g), dim=-1)
        nrm = (base + 1e-3 * torch.randn(n // k, k, 3, generator=g)).reshape(n, 3)
    else:
        nrm = torch.randn(n, 3, generator=g)
    return {'idr_rgb_values': idr, 'sg_rgb_values': sg, 'rgb': gt.reshape(1, n, 3), 'network_object_mask': net, 'object_mask': obj,
            'sdf_output': torch.randn(n, 1, generator=g) * case['sdf_scale'], 'normal_values': nrm}


def run_loss(case, inp, dtype, device='cpu', fused=False, kwargs=None, loss_cls=IDRLoss):
    """-> {'terms': {name: 0-d tensor}, 'd_idr': [n, 3] or None, 'd_sg': [n, 3]} of IDRLoss on `device` in `dtype`.
    form 'f64_strided' hands the colours over as every second column of a float64 [n, 6] leaf (whatever `dtype` is: it is the
    form the wrapper has to convert), otherwise as contiguous leaves of `dtype`."""
    def leaf(t):
        if case['form'] == 'f64_strided' and fused:
            wide = torch.zeros(t.shape[0], 6, dtype=torch.float64)
            wide[:, ::2] = t.double()
            wide = wide.to(device).requires_grad_(True)
            return wide, wide[:, ::2]
        x = t.detach().clone().to(device=device, dtype=dtype).requires_grad_(True)      # (a leaf of its own: .to() may return t)
        return x, x
    (idr_leaf, idr), (sg_leaf, sg) = leaf(inp['idr_rgb_values']), leaf(inp['sg_rgb_values'])
    out = {'idr_rgb_values': idr, 'sg_rgb_values': sg, 'network_object_mask': inp['network_object_mask'].to(device),
           'object_mask': inp['object_mask'].to(device), 'sdf_output': inp['sdf_output'].to(device=device, dtype=dtype),
           'normal_values': inp['normal_values'].to(device=device, dtype=dtype), 'grad_theta': None}
    L = loss_cls(**(kwargs or loss_kwargs(case)))
    L.fused = fused
    lo = L(out, {'rgb': inp['rgb'].to(device=device, dtype=dtype)})
    lo['loss'].backward()

    def grad(leaf_, view):
        if leaf_.grad is None:
            return None
        return leaf_.grad[:, ::2].contiguous() if leaf_ is not view else leaf_.grad
    return {'terms': {k: lo[k].detach() for k in TERMS}, 'd_idr': grad(idr_leaf, idr), 'd_sg': grad(sg_leaf, sg)}


def judge_loss(j, tag, got, ref64, ref32):
    for k in TERMS:
        j.term('%s %s' % (tag, k), got['terms'][k], ref64['terms'][k], ref32['terms'][k])
    for k in ('d_idr', 'd_sg'):
        if ref64[k] is None:
            j.require('%s %s' % (tag, k), got[k] is None, 'None on both sides' if got[k] is None else 'a gradient where the reference has none')
        elif got[k] is None:
            j.require('%s %s' % (tag, k), False, 'no gradient')
        else:
            j.elements('%s %s' % (tag, k), got[k], ref64[k], ref32[k])


# ---- prepare_hits ----------------------------------------------------------------------------------------------------
# (n, rows, feat_cols, order of idx)
HITS_CASES = [(1, 5, 0, 'repeats'), (255, 300, 1, 'ascending'), (256, 300, 3, 'shuffled'), (257, 300, 5, 'repeats'),
              (255, 64, 256, 'shuffled'), (257, 300, 257, 'ascending'), (256, 512, 512, 'repeats'), (2100, 2500, 512, 'shuffled')]


def hits_inputs(n, rows, fcols, order):
    """points, ray_dirs, grad [rows, 3], feat [rows, fcols] or None, idx [n] int64; vector norms 1e-3 .. 1e3, gradient row
    idx[0] exactly zero"""
    g = torch.Generator().manual_seed(41 + n + fcols)
    scale = lambda: 10 ** (torch.rand(rows, 1, generator=g) * 6 - 3)                           # noqa: E731
    pts = torch.randn(rows, 3, generator=g)
    dirs = torch.nn.functional.normalize(torch.randn(rows, 3, generator=g), dim=-1) * scale()
    grad = torch.nn.functional.normalize(torch.randn(rows, 3, generator=g), dim=-1) * scale()
    feat = torch.randn(rows, fcols, generator=g) if fcols else None
    if order == 'repeats':
        idx = torch.randint(0, rows, (n,), generator=g)
    else:
        idx = torch.randperm(rows, generator=g)[:n] if n <= rows else torch.randint(0, rows, (n,), generator=g)
        idx = idx.sort().values if order == 'ascending' else idx
    grad[idx[0]] = 0.
    return pts, dirs, grad, feat, idx


def hits_ref(pts, dirs, grad, feat, idx, dtype, negate=True):
    v = dirs.to(dtype).index_select(0, idx)
    v = -v if negate else v
    gg = grad.to(dtype).index_select(0, idx)
    return (pts.index_select(0, idx), v / (v.norm(dim=-1, keepdim=True) + 1e-6), gg / (gg.norm(dim=-1, keepdim=True) + 1e-6),
            None if feat is None else feat.index_select(0, idx))


def judge_hits(j, tag, got, ref64, ref32, zero_row=0):
    j.same_bits(tag + ' points', got[0], ref64[0])
    j.absolute(tag + ' view', got[1], ref64[1], ref32[1])
    j.absolute(tag + ' normals', got[2], ref64[2], ref32[2])
    j.require(tag + ' zero gradient row', bool((got[2][zero_row] == 0).all()), 'normal of the zero gradient: %s' % got[2][zero_row].tolist())
    if ref64[3] is None:
        j.require(tag + ' feat', got[3] is None, 'None expected')
    else:
        j.same_bits(tag + ' feat', got[3], ref64[3])


# ---- rows ------------------------------------------------------------------------------------------------------------
MAX_ROW_BLOCKS = 12          # NEFII_MAX_ROW_BLOCKS (tests assert it against _lib.MAX_ROW_BLOCKS)
_COLS12 = (1, 3, 7, 2, 5, 3, 1, 4, 3, 6, 2, 16)
_FORMS = ('full', 'row', 'col', 'one')          # [n, C], [1, C], [n, 1], [1, 1]


def _rc(name, rows, n, cols, forms, pad=0, unused=None, const=None):
    return dict(name=name, rows=rows, n=n, cols=tuple(cols), forms=tuple(forms), pad=pad, unused=unused, const=const)


ROW_CASES = [
    _rc('rows1', 1, 1, (3, 1, 3, 2), _FORMS),
    _rc('rows2-n1', 2, 1, (3, 1, 3, 2), _FORMS, unused=1),
    _rc('rows2-n2', 2, 2, (3, 2, 3, 4), _FORMS),
    _rc('rows1001-n0', 1001, 0, (3, 1, 3, 2), _FORMS),
    _rc('rows1001-pad', 1001, 300, (3, 1, 3, 3), _FORMS, pad=20, unused=1, const=3),
    _rc('rows1001-12-widest-last', 1001, 300, _COLS12, [_FORMS[i % 4] for i in range(12)], pad=7, unused=5),
    _rc('rows1001-12-widest-first', 1001, 300, _COLS12[::-1], [_FORMS[(i + 1) % 4] for i in range(12)], const=2),
    _rc('rows90000', 90000, 89100, (3, 3, 3), ('full', 'row', 'col'), pad=100),
]


def rows_inputs(case):
    """where [n] int64 (the last `pad` entries name the scratch row `rows`), sources (list of [n|1, C|1] float32), fills, the
    weights [rows, C] of the loss sum(out[:rows] * w): multiples of 1/4, so every gradient sum is exact in any order"""
    g = torch.Generator().manual_seed(11 + case['rows'] + len(case['cols']))
    rows, n, pad = case['rows'], case['n'], case['pad']
    hit = torch.randperm(rows, generator=g)[:n - pad].sort().values
    where = torch.cat([hit, torch.full((pad,), rows, dtype=torch.int64)])
    srcs = []
    for c, form in zip(case['cols'], case['forms']):
        shape = {'full': (n, c), 'row': (1, c), 'col': (n, 1), 'one': (1, 1)}[form]
        srcs.append(torch.randn(shape, generator=g))
    fills = [float(k % 3) - 0.5 for k in range(len(srcs))]
    wts = [torch.randint(-8, 9, (rows, c), generator=g).float() / 4. for c in case['cols']]
    return where, srcs, fills, wts


def rows_ref(case, where, srcs, fills, wts):
    """-> outputs [rows (+1 with padding), C] and the gradients of the sources (None for the unused / constant ones)"""
    rows, n = case['rows'], case['n']
    total = rows + (1 if case['pad'] else 0)
    leaves = [s.clone().requires_grad_(k != case['const']) for k, s in enumerate(srcs)]
    outs = [torch.full((total, c), f, dtype=s.dtype).index_put((where,), s.expand(n, c)) for s, c, f in zip(leaves, case['cols'], fills)]
    used = [k for k in range(len(srcs)) if k != case['unused'] and k != case['const']]
    if used:
        sum((outs[k][:rows] * wts[k]).sum() for k in used).backward()
    return [o.detach() for o in outs], [l.grad for l in leaves]


# ---- material head ---------------------------------------------------------------------------------------------------
HEAD_PARAMS = (-30., -5., 0., 0.3, 5., 10., 30.)
HEAD_CASES = [(p, n_spec, fr, fs, drop) for p in HEAD_PARAMS for n_spec in (1, 3)
              for fr, fs, drop in ((False, False, None), (True, False, None), (False, True, None), (True, True, None),
                                   (False, False, 'rough'), (False, False, 'spec'))]


def head_inputs(p, n_spec):
    g = torch.Generator().manual_seed(3 + n_spec)
    rp = torch.full((1, 1), p)
    sp = (torch.full((1, n_spec), p) + (torch.tensor([[0., 0.25, -0.5]]) if n_spec == 3 else 0.)).float()
    return rp, sp, torch.randn(1, 1, generator=g), torch.randn(1, 3, generator=g)


def head_ref(rp, sp, w_r, w_s, fake_rough, fake_spec, drop, dtype):
    """-> (roughness [1,1], specular [1,3], d rough_param, d spec_param); `drop`: the output that takes no part in the loss"""
    rp, sp = rp.detach().clone().to(dtype).requires_grad_(True), sp.detach().clone().to(dtype).requires_grad_(True)
    r = (1 - 0.089) * torch.sigmoid(rp) + 0.089
    s = torch.sigmoid(sp).expand(-1, 3)
    if fake_rough:
        r = 0 * r + 0.5
    if fake_spec:
        s = 0 * s + 0.5
    s = 0.16 * s ** 2
    loss = 0
    if drop != 'rough':
        loss = loss + (r * w_r.to(dtype)).sum()
    if drop != 'spec':
        loss = loss + (s * w_s.to(dtype)).sum()
    loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad                          # noqa: E731
    return r.detach(), s.detach(), zero(rp), zero(sp)



HEAD_OUTPUTS = ('rough', 'spec', 'd_rough_param', 'd_spec_param')


def judge_head(j, tag, p, n_spec, got, ref64, ref32):
    """the four quantities of one head case: the measure the suite had (absolute over max(1, |ref|max), cap 1e-6) and the
    per-element relative one that makes the saturated parameters count (module docstring)"""
    p_max = p + (0.25 if n_spec == 3 else 0.)            # head_inputs: the largest parameter of the case
    one_minus_s = 1. / (1. + math.exp(p_max))
    for name, g, w, w32 in zip(HEAD_OUTPUTS, got, ref64, ref32):
        j.absolute('%s %s' % (tag, name), g, w, w32, cap=CAP_HEAD, scaled=True)
        floor = FLOOR + (2e-7 / one_minus_s if name.startswith('d_') else 0.)
        j.elements('%s %s' % (tag, name), g, w, w32, floor=floor, cap=float('inf'))

# ---- camera ----------------------------------------------------------------------------------------------------------
# (B, S, stride of the judged subset or None for every ray)
CAMERA_CASES = [(1, 1, None), (1, 255, None), (3, 257, None), (3, 1, None), (1, 257, None), (2, 270000, 'subset')]


def _rot(ax, ay, az):
    def r(a, i, j):
        m = torch.eye(3, dtype=torch.float64)
        m[i, i] = m[j, j] = math.cos(a)
        m[i, j], m[j, i] = -math.sin(a), math.sin(a)
        return m
    return r(az, 0, 1) @ r(ay, 0, 2) @ r(ax, 1, 2)


def camera_inputs(B, S):
    """uv [B, S, 2] over a 512 x 384 image, rotated and translated poses, intrinsics with skew, an off-centre principal point
    and fx != fy: float32"""
    g = torch.Generator().manual_seed(9 + B + S)
    uv = torch.rand(B, S, 2, generator=g) * torch.tensor([512., 384.])
    pose, K = torch.zeros(B, 4, 4, dtype=torch.float64), torch.zeros(B, 4, 4, dtype=torch.float64)
    for b in range(B):
        pose[b, :3, :3] = _rot(0.4 + 0.9 * b, -0.7 + 0.5 * b, 1.1 - 0.8 * b)
        pose[b, :3, 3] = torch.tensor([(1.0, 0.5, -2.0), (-0.7, 1.6, 0.9), (0.2, -1.1, 1.7)][b % 3], dtype=torch.float64)
        pose[b, 3, 3] = 1.
        K[b] = torch.eye(4, dtype=torch.float64)
        K[b, 0, 0], K[b, 1, 1], K[b, 0, 1] = 410. + 35. * b, 388. - 20. * b, 2.5 - 4. * b
        K[b, 0, 2], K[b, 1, 2] = 241.3 + 9. * b, 201.7 - 6. * b
    return uv, pose.float(), K.float()


def camera_subset(S, kind):
    if kind is None:
        return torch.arange(S)
    return torch.cat([torch.arange(0, S - 300, (S - 300 + 3999) // 4000)[:4000], torch.arange(S - 300, S)])


def camera_ref(uv, pose, K, dtype):
    dirs, cam = orr.camera_rays(uv.to(dtype), pose.to(dtype), K.to(dtype))
    return dirs, cam
