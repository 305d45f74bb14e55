"""fp64 yardstick of the tracer tests (tests/test_trace64_cpu.py, tests/test_gpu_tracer_rays.py): ray families off the shipped
distribution, a consensus verdict for the hit mask and the surface depths, and a certificate for the argmin depths.

Reference.  oracle/tracer.py follows the dtype of its rays; run in float64 on the fp32 rays, with the SDF evaluated in float64 on
the fp32 EFFECTIVE weights the kernel packs (trace_cmp.build_sdf packs nets.linear_params' fp32 product), it is the yardstick.

Consensus.  A tracer is a chain of decisions (`sdf <= threshold`, `sdf < 0`, `t_s < t_e`, first negative sample); a ray that
sits on one of them may go either way in any arithmetic, and no tolerance on the outcome can tell that from a mistraced ray.
So four reference traces are run per case - fp64, fp64 with the SDF shifted by +EPS and by -EPS, and the fp32 oracle - and a ray
is DECIDABLE when all four agree on `hit` and, where the fp64 ray ends on the surface (hit, not through an argmin), on its
depth within DEPTH_AGREE.  EPS = 1e-5 is twice the 5e-6 the suite asserts for the split evaluator against fp64
(mlp64.CAP_SDF_SPLIT): an evaluator within that bound decides every comparison of a decidable ray as one of the shifted
references does.  On decidable rays the hit mask must be EQUAL and a surface depth within sdf_threshold + EPS_SDF of the fp64
depth.  At most MAX_UNDECIDABLE of a case's rays may be undecidable: a condition on the case, asserted before anything is compared.

The depth bound.  A front may arrive one step earlier or later than the reference's.  The step one tracer takes and the other
does not has `sdf > threshold` for the first and `sdf <= threshold` for the second, two values at most the evaluators' error
apart: the step is at most sdf_threshold + EPS_SDF, not sdf_threshold - which the REFERENCES miss too (the fp32 oracle against
fp64: 5.009e-5 on a ray of `shell`, n_steps 128 / 25 iterations, ray seed 101; 4.99e-5 on the smooth net) and the kernel did
once (f16x3, smooth net, `shell`, eval: 5.024e-5, a front that stopped where fp64 took a step of 5.024e-5).  Second, the
iteration cap: see `knife` below - a front whose last test is within EPS of the threshold either stops (thr / |cos| short of
the root) or goes on to the sampler, which finds the root; the f32 kernel took the first where all four references took the
second (9.2e-5 apart, smooth net, ray 1289 of `shell`).  Such rays are held to whichever outcome the tracer took.

Certificate.  Training-mode rays that hit the bounding sphere, never entered the sampler and are not the masked-out hits whose
t_min moved end at argmin_i sdf(o + c_i d) over the candidates c_i = t_min + steps[i] (t_max - t_min).  Near-ties flip the
winner, so the depth is not compared with the reference's: the depth must BE a candidate, within the fp32 rounding of that
candidate (`cand_rounding`: a first-order bound per ray, dominated by the conditioning of the sphere intersection - 1e-5 on a
grazing ray, where `under` cancels, 2e-7 on a ray from inside), and the fp64 SDF at it may exceed the fp64 minimum over the
candidates by at most 2 EPS_SDF + delta, delta = 2 x the excess the fp32 oracle needs on the same rays.  (Twice the fp32
oracle's own per-case distance from a candidate - the first form of the depth test - is NOT reachable by a correct fp32 tracer:
the oracle's `norm` and the kernel's sum of squares round |o| differently on one ray in nine, and on the worst-conditioned ray
of a case either may be the luckier: kernel 9.5e-6 against oracle 3.8e-6 on `graze`, 1.28e-7 = 2 ulp against 6.4e-8 = 1 ulp on
`inside` at radius 0.7.  In units of the rounding bound the oracle needs at most 0.16 and the kernel 0.17.)  Rays on which the four
references disagree about the path (sphere hit, sampler) are left out of the certificate and counted.

Rays with a constant answer are held to it exactly: no sphere, eval mode: dist 0, no hit, point = origin; no sphere, training
mode: dist = -d.o within 2 ulp of sum_i |d_i o_i| (three products and two sums, each rounded once: at most 3 x 2^-24 of that
sum, in any order); sphere interval collapsed to [0.01, 0.01] (`away`), training mode: dist = 0.01f.

No vacuous pass: a case names the ray classes it is there for, and the judge wants MIN_CLASS decidable rays in each."""
import torch

from nefii_amd import synthetic as syn
from oracle import nets, tracer

EPS, EPS_SDF, DEPTH_AGREE, MAX_UNDECIDABLE, MIN_CLASS = 1e-5, 5e-6, 1e-4, 0.03, 30
ULP = 2.0 ** -23
CLASSES = ('traced_hit', 'bisected_hit', 'sampler_miss', 'argmin', 'moved_tmin', 'no_sphere', 'collapsed')
FAMILIES = ('shell', 'inside', 'graze', 'away', 'miss')

# parameter sets: each overrides only what it names, the rest stays syn.RAY_TRACER
PARAM_SETS = {
    'default': {},
    'oracle_default': dict(line_step_iters=1, n_rootfind_steps=8),
    'n16': dict(n_steps=16),
    'n37_it3': dict(n_steps=37, sphere_tracing_iters=3),
    'n128_it25_k5': dict(n_steps=128, sphere_tracing_iters=25, line_step_iters=5),
    'r0.7': dict(object_bounding_sphere=0.7),
    'r1.5': dict(object_bounding_sphere=1.5),
    'thr1e-3': dict(sdf_threshold=1.0e-3),
    'it0': dict(sphere_tracing_iters=0),
    'root0': dict(n_rootfind_steps=0),
    'ls0.8': dict(line_search_step=0.8),
}

NETS = {     # name -> (model, hidden, bumpy, state-dict seed[, scene])
    'physg64-smooth': ('physg', 64, 0.0, 2),
    # seed 1: with line_search_step 0.8 on `shell` the four REFERENCES leave 2.0 % of the rays undecidable on this net (fronts that
    # overshoot, do not recover within three back-offs of a fifth of the step and end inside the body, at a depth that moves by
    # 1e-4 .. 3e-3 with an SDF shift of 1e-5); on the nets of seeds 0, 2 and 3 they leave 3.3 - 4.9 %, above the 3 % a case may have
    'physg64-bumpy': ('physg', 64, 0.03, 1),
    'physg512-bumpy': ('physg', None, 0.004, 2),
    'neus256-bumpy': ('neus', None, 0.01, 4),
    # the two trained scenes that ship (test_gpu_minsdf_share._net's bowl; the thin bars of assets/scene_frame_sdf512.npz)
    'conf512-bowl-trained': ('conf', None, 0.0, 2, 'bowl_trained'),
    'conf512-frame-trained': ('conf', None, 0.0, 2, 'frame_trained'),
}


def tracer_params(pset):
    p = dict(syn.RAY_TRACER)
    p.update(PARAM_SETS[pset] if isinstance(pset, str) else pset)
    return p


_NETS = {}


def make_net(name):
    """(model conf, state dict, fp32 sdf, fp64 sdf) - the fp64 one on the fp32 effective weights, on the device of its points"""
    if name in _NETS:
        return _NETS[name]
    model, hidden, bumpy, seed = NETS[name][:4]
    scene = NETS[name][4] if len(NETS[name]) > 4 else None
    mc = syn.model_conf(model, hidden=hidden)
    sd = syn.make_state_dict(mc, seed=seed, bumpy=bumpy, scene=scene)
    cfg = mc['implicit_network']
    sd64 = {}
    for l in range(nets.count_layers(sd, 'implicit_network')):
        w, b = nets.linear_params(sd, 'implicit_network.lin%d' % l)
        sd64['implicit_network.lin%d.weight' % l] = w.double()
        sd64['implicit_network.lin%d.bias' % l] = b.double()
    on = {}

    def sdf32(x):
        return nets.sdf_forward(sd, cfg, x)[:, 0]

    def sdf64(x):
        dev = str(x.device)
        if dev not in on:
            on[dev] = {k: v.to(x.device) for k, v in sd64.items()}
        return nets.sdf_forward(on[dev], cfg, x)[:, 0]

    _NETS[name] = (mc, sd, sdf32, sdf64)
    return _NETS[name]


def _unit(g, n):
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return v / v.norm(dim=-1, keepdim=True)


def _perp(g, a):
    """unit vectors perpendicular to the unit vectors a"""
    v = _unit(g, a.shape[0])
    v = v - (v * a).sum(-1, keepdim=True) * a
    return v / v.norm(dim=-1, keepdim=True)


def rays(family, n, seed, R=1.0, n_steps=100):
    """Seeded fp32 rays with unit directions (normalised in fp64, rounded once), scaled with the bounding sphere's radius R.
    Returns (origins, dirs, object_mask, minsdf_steps)."""
    g = torch.Generator().manual_seed(seed)
    if family == 'shell':            # the distribution every other tracer test draws (test_gpu_kernels._trace_batch)
        o = _unit(g, n) * (1.5 + torch.rand(n, 1, generator=g, dtype=torch.float64)) * R
        d = torch.randn(n, 3, generator=g, dtype=torch.float64) * 0.45 * R - o
    elif family == 'inside':         # secondary-ray-like: start clamped to 0.01, many origins inside the object
        o = _unit(g, n) * (torch.rand(n, 1, generator=g, dtype=torch.float64) ** (1.0 / 3.0)) * 0.95 * R
        d = _unit(g, n)
    elif family == 'graze':          # closest approach to the centre at 0.9 - 1.1 R: long tangent chords, and misses beside them
        a = _unit(g, n)
        o = a * 2.0 * R
        sin = (0.9 + 0.2 * torch.rand(n, 1, generator=g, dtype=torch.float64)) / 2.0
        d = -a * torch.sqrt(1 - sin * sin) + _perp(g, a) * sin
    elif family == 'away':           # the line meets the sphere BEHIND the origin: under > 0, both depths clamp to 0.01
        a = _unit(g, n)
        o = a * (1.0 + torch.rand(n, 1, generator=g, dtype=torch.float64)) * R
        d = a + 0.12 * torch.randn(n, 3, generator=g, dtype=torch.float64)
    elif family == 'miss':           # every ray misses the sphere: half at right angles to the origin, half passing 1.05 - 1.45 R off
        a = _unit(g, n)
        rad = 1.5 + torch.rand(n, 1, generator=g, dtype=torch.float64)
        o = a * rad * R
        sin = (1.05 + 0.4 * torch.rand(n, 1, generator=g, dtype=torch.float64)) / rad
        side = _perp(g, a)
        d = torch.where(torch.rand(n, 1, generator=g, dtype=torch.float64) < 0.5, side, -a * torch.sqrt(1 - sin * sin) + side * sin)
    else:
        raise KeyError(family)
    d = d / d.norm(dim=-1, keepdim=True)
    om = torch.rand(n, generator=g) < 0.8
    steps = torch.rand(n_steps, generator=g)
    return o.float().contiguous(), d.float().contiguous(), om, steps


class Case:
    """`given`: (origins, dirs, object_mask, minsdf_steps) instead of a family's rays (hand-made rays, mixed batches)"""

    def __init__(self, net, family, pset, training, n, classes, seed=7, given=None):
        self.net, self.family, self.pset, self.training, self.n, self.classes, self.seed = net, family, pset, training, n, classes, seed
        self.given = given
        assert all(c in CLASSES for c in classes)
        self.id = '%s-%s-%s-%s' % (net, family, pset if isinstance(pset, str) else 'custom', 'train' if training else 'eval')

    def params(self):
        return tracer_params(self.pset)

    def rays(self):
        if self.given is not None:
            return self.given
        p = self.params()
        return rays(self.family, self.n, self.seed, p['object_bounding_sphere'], p['n_steps'])


class References:
    """The four reference traces of a case and what the judge derives from them.  `device`: where the three fp64 traces run
    (the fp32 oracle always runs on the CPU, as the reference does)."""

    def __init__(self, case, device='cpu', trace32=None):
        self.case = case
        mc, sd, sdf32, sdf64 = make_net(case.net)
        p = case.params()
        self.p, self.sdf64 = p, sdf64
        o, d, om, steps = case.rays()
        self.o, self.d, self.om, self.steps = o, d, om, steps
        o64, d64, st64, omd = o.double().to(device), d.double().to(device), steps.double().to(device), om.to(device)
        run = trace32 or tracer.trace
        self.r32 = run(sdf32, o, d, om, p, case.training, steps)
        self.r64 = self._cpu(tracer.trace(sdf64, o64, d64, omd, p, case.training, st64))
        self.rp = self._cpu(tracer.trace(lambda x: sdf64(x) + EPS, o64, d64, omd, p, case.training, st64))
        self.rm = self._cpu(tracer.trace(lambda x: sdf64(x) - EPS, o64, d64, omd, p, case.training, st64))
        refs = (self.r64, self.rp, self.rm, self.r32)
        r = self.r64
        hit, samp, sph = r['hit'], r['sampler_mask'], r['sphere_hit']
        tr = case.training
        self.argmin = (~hit | ~om) if tr else ~hit          # trace_cmp.argmin_set
        self.surface = hit & ~self.argmin
        same_hit = torch.ones_like(hit)
        for q in refs[1:]:
            same_hit &= q['hit'] == hit
        dd = torch.stack([q['dists'].double() for q in refs])
        spread = dd.max(0).values - dd.min(0).values
        self.decidable = same_hit & (~self.surface | (spread <= DEPTH_AGREE))
        # The one knife edge the shifted traces do not see (a shift moves the whole trajectory, not one test): the start front's
        # `sdf <= threshold` test AT THE ITERATION CAP within EPS of the threshold.  One outcome ends on the front - thr / |cos|
        # short of the root, MORE than one threshold at any incidence - the other goes to the sampler and finds the root.  Both
        # are hits; such a ray's surface depth is held to whichever of the two the tracer took (`alt`: the other one, the front
        # if the fp64 trace went on to the sampler, else the root behind the front, bisected in fp64); no root within 20
        # thresholds of the front: undecidable.
        thr = p['sdf_threshold']
        self.knife = r['at_cap_s'] & ((r['last_sdf_s'] - thr).abs() < EPS) & self.surface
        self.alt = r['dists'].clone()
        k = self.knife & ~samp
        if k.any():
            ok, root = self._root_behind(o[k].double(), d[k].double(), r['front_s'][k], 20 * abs(thr))
            self.alt[k] = torch.where(ok, root, torch.full_like(root, float('nan')))
        self.alt[self.knife & samp] = r['front_s'][self.knife & samp]
        self.decidable &= ~torch.isnan(self.alt)
        self.same_path = torch.ones_like(hit)
        for q in refs[1:]:
            self.same_path &= (q['sampler_mask'] == samp) & (q['sphere_hit'] == sph)
        t_io, _ = tracer.sphere_intersection(o.double(), d.double(), p['object_bounding_sphere'])
        self.t_io = t_io
        self.cls = {
            'traced_hit': self.surface & ~samp,
            'bisected_hit': self.surface & samp,
            'sampler_miss': samp & ~hit,
            'argmin': (~hit & ~samp & sph) if tr else torch.zeros_like(hit),
            'moved_tmin': (hit & ~om & ~samp & sph) if tr else torch.zeros_like(hit),
            'no_sphere': ~sph,
            'collapsed': sph & (t_io[:, 0] == t_io[:, 1]),
        }
        self.undecidable_share = 1.0 - self.decidable.float().mean().item()
        # fp32 rounding of a candidate depth, to first order, with u = 2^-24 per rounded operation: b = d.o carries 3 u |o|
        # (three products, two sums, |d| = 1); under = b^2 - (|o|^2 - R^2) carries 2 |b| db + 8 u (b^2 + |o|^2 + R^2) (the norm's
        # three products, two sums, root and square; two more squares, two differences) and enters t = -b -+ sqrt(under) divided by
        # 2 sqrt(under) - the conditioning of a grazing ray; the root, the difference and c = t_min + s (t_max - t_min) add 5 u t_max
        o64, d64 = o.double(), d.double()
        u, R = 2.0 ** -24, p['object_bounding_sphere']
        bb, no = (d64 * o64).sum(-1), o64.norm(dim=-1)
        under = (bb * bb - (no * no - R * R)).clamp_min(1e-30)
        self.cand_rounding = u * (3 * no + (6 * bb.abs() * no + 8 * (bb * bb + no * no + R * R)) / (2 * under.sqrt()) + 5 * t_io[:, 1].clamp_min(0.01))
        # what the fp32 oracle itself needs on the certificate's rays
        self.cert = self.cls['argmin'] & self.decidable & self.same_path
        self.delta_excess, self.delta_depth, self.delta_ratio = self.certificate(self.r32['dists'])

    def _root_behind(self, o, d, front, reach):
        """(found, depth) of the SDF's sign change on [front, front + reach] along the rays, by bisection in fp64"""
        f = lambda t: self.sdf64(o + t.unsqueeze(-1) * d)
        lo, hi = front.clone(), front + reach
        ok = (f(lo) > 0) & (f(hi) < 0)
        for _ in range(40):
            mid = (lo + hi) / 2
            up = f(mid) > 0
            lo, hi = torch.where(up, mid, lo), torch.where(up, hi, mid)
        return ok, (lo + hi) / 2

    @staticmethod
    def _cpu(r):
        return {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in r.items()}

    def certificate(self, dist):
        """(worst excess of the fp64 SDF at `dist` over the fp64 minimum of the candidates, worst distance of `dist` from the
        nearest fp64 candidate) over the certificate's rays"""
        m = self.cert
        if not m.any():
            return 0.0, 0.0, 0.0
        o, d = self.o[m].double(), self.d[m].double()
        cand = self.t_io[m, 0:1] + self.steps.double().view(1, -1) * (self.t_io[m, 1:2] - self.t_io[m, 0:1])      # [m, n]
        vals = self.sdf64((o.unsqueeze(1) + cand.unsqueeze(-1) * d.unsqueeze(1)).reshape(-1, 3)).reshape(cand.shape)
        t = dist[m].double()
        at = self.sdf64(o + t.unsqueeze(-1) * d)
        excess = (at - vals.min(-1).values).max().item()
        off = (cand - t.unsqueeze(-1)).abs().min(-1).values
        return excess, off.max().item(), (off / self.cand_rounding[m]).max().item()


def judge(refs, got, what=None, min_class=MIN_CLASS, hits_only=False):
    """Hold a trace `got` = (points, hit, dists) to the references of its case.  Prints the figures, then asserts.
    hits_only (an eval-mode trace whose misses nobody reads, nefii_tracer_params.unread_misses): the hit mask and the depths and
    points of the hits; of a miss only that it is one and that its outputs are finite."""
    case, p = refs.case, refs.p
    what = what or case.id
    pts, hit, dist = (t.detach().cpu() for t in got[:3])
    hit = hit.bool()
    o, d, om, r = refs.o, refs.d, refs.om, refs.r64
    dec = refs.decidable
    counts = {c: int((refs.cls[c] & dec).sum()) for c in CLASSES}
    flips = int(((hit != r['hit']) & dec).sum())
    s = refs.surface & dec
    per_ray = torch.minimum((dist.double() - r['dists']).abs(), (dist.double() - refs.alt).abs())      # (alt = the fp64 depth but on knife-edge rays)
    depth_err = per_ray[s].max().item() if s.any() else 0.0
    excess, off, ratio = refs.certificate(dist)
    print('[trace64 %s] undecidable %.2f %% | knife-edge %d | decidable per class %s | flips %d | worst surface depth error %.2e (%d rays) | '
          'certificate on %d rays (%d left out: path): excess %.2e (fp32 oracle %.2e), off a candidate %.2e = %.2f of its fp32 rounding (fp32 oracle %.2e = %.2f)'
          % (what, 100.0 * refs.undecidable_share, int(refs.knife.sum()), ' '.join('%s=%d' % (c, counts[c]) for c in CLASSES if counts[c] or c in case.classes),
             flips, depth_err, int(s.sum()), int(refs.cert.sum()), int((refs.cls['argmin'] & dec & ~refs.same_path).sum()),
             excess, refs.delta_excess, off, ratio, refs.delta_depth, refs.delta_ratio))
    assert refs.undecidable_share <= MAX_UNDECIDABLE, (what, 'undecidable share', refs.undecidable_share)
    for c in case.classes:
        assert counts[c] >= min_class, (what, 'class %s has %d decidable rays' % (c, counts[c]))
    assert flips == 0, (what, 'hit mask flips on decidable rays', flips, torch.nonzero((hit != r['hit']) & dec).flatten()[:8].tolist())
    if s.any():          # the worst ray, with what every reference says about it (fp64, +EPS, -EPS, fp32 oracle)
        i = int(torch.nonzero(s).flatten()[per_ray[s].argmax()])
        worst = dict(ray=i, got=dist[i].item(), refs=[q['dists'][i].item() for q in (r, refs.rp, refs.rm, refs.r32)],
                     sampler=[bool(q['sampler_mask'][i]) for q in (r, refs.rp, refs.rm, refs.r32)], knife=bool(refs.knife[i]), alt=refs.alt[i].item())
    assert depth_err <= p['sdf_threshold'] + EPS_SDF, (what, 'surface depth', depth_err, worst)
    if case.training:
        assert excess <= 2 * EPS_SDF + 2 * max(refs.delta_excess, 0.0), (what, 'argmin excess', excess, refs.delta_excess)
        assert ratio <= 1.0, (what, 'argmin depth off the candidates, in units of their fp32 rounding', ratio, off, refs.delta_depth)
    # constants
    nos = ~r['sphere_hit']
    if nos.any():
        assert not hit[nos].any(), (what, 'a ray that misses the sphere hit')
        if case.training:
            terms = (d[nos].double() * o[nos].double())
            err = (dist[nos].double() + terms.sum(-1)).abs()
            assert (err <= 2 * ULP * terms.abs().sum(-1)).all(), (what, 'dist != -d.o', (err / (ULP * terms.abs().sum(-1))).max().item())
        elif not hits_only:
            assert (dist[nos] == 0).all() and torch.equal(pts[nos], o[nos]), (what, 'sphere miss in eval mode')
    col = refs.cls['collapsed']
    if col.any():
        assert not hit[col].any(), (what, 'a ray with a collapsed interval hit')
        if case.training:
            assert (dist[col] == torch.tensor(0.01)).all(), (what, 'collapsed interval: dist != 0.01f')
    assert torch.isfinite(pts).all() and torch.isfinite(dist).all()
    read = hit if hits_only else torch.ones_like(hit)
    off_ray = (pts.double() - (o.double() + dist.double().unsqueeze(-1) * d.double())).abs().max(-1).values
    assert not read.any() or off_ray[read].max().item() < 1e-6 * max(1.0, p['object_bounding_sphere'])
    return dict(flips=flips, depth_err=depth_err, excess=excess, off=off, counts=counts)


def oracle_evals(counters):
    return sum(counters.get(k, 0) for k in ('sphere_trace', 'sampler', 'bisect', 'min_sdf'))


# ---- the case matrix -----------------------------------------------------------------------------------------------------
def classes_of(family, pset, training):
    """the ray classes a case is there for, on the geometric-init nets (a body of radius 0.5 - 0.6)"""
    if family == 'miss':
        return ('no_sphere',)
    if family == 'away':
        return ('collapsed',)
    if family == 'graze':
        return ('argmin', 'no_sphere') if training else ('no_sphere',)
    if pset in ('it0', 'n37_it3'):          # (nearly) no sphere tracing: the bracket search and the bisection decide
        c = ['bisected_hit'] + (['sampler_miss'] if pset == 'it0' or family == 'shell' else [])
        if training and pset == 'n37_it3':
            c.append('argmin')
    else:
        c = ['traced_hit'] + (['argmin', 'moved_tmin'] if training else [])
        if family == 'shell' and pset in ('default', 'n16', 'root0', 'r0.7', 'r1.5'):
            c.append('bisected_hit')
    if family == 'shell':
        c.append('no_sphere')
    return tuple(c)


def matrix(net='physg64-bumpy', n=1500, eval_sets=('default', 'it0', 'root0', 'n37_it3')):
    """every parameter set on `shell` and `inside`, every family on default, for one net: all of it in training mode (the
    longer path: min-SDF search behind everything eval mode does), the sets of `eval_sets` in eval mode as well"""
    out = []
    for training in (True, False):
        for pset in PARAM_SETS:
            if not training and pset not in eval_sets:
                continue
            for fam in (FAMILIES if pset == 'default' else ('shell', 'inside')):
                out.append(Case(net, fam, pset, training, n, classes_of(fam, pset, training)))
    return out
