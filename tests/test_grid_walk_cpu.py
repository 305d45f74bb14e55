"""The two walks over the SDF interval grid, thread-per-ray and by the whole wave, restated in NumPy and held to each other
(csrc/nefii_tracer.hip: begin_grid_bracket / grid_audit against wave_grid_bracket / wave_grid_audit, which
tests/test_gpu_grid_walk.py holds to each other on the GPU).

A row is what the look-ups give for one ray: the cell interval (lo, hi) of every sample, the corner bounds of every sample
(with `ok`: the sample lies inside the cube), the exact values of the samples in front of `from`, and a hash per sample.
`sequential_bracket` is begin_grid_bracket line by line: the cell pass, the corner pass with its `break`, the survivors
with the near-miss probes counted as the loop meets them and the hash probe kept by `hh < probe_h`.  `wave_bracket` is the
restatement the wave runs: 64 lanes per pass, ballots as integers, first index by lowest set bit, the near-miss probes by
prefix popcount across the passes, the hash probe as the least (hash, index).  Both must leave the same marks, the same
count of probes, the same probe and take the whole-row fallback for the same rows.  Likewise grid_audit's choice of the samples
that get corner bounds: the first CREF_CAP evaluated samples inside the cube, in index order."""
import numpy as np
import pytest

F = np.float32
INF = F(np.inf)
TAU = F(2e-3)
NEAR_PROBES = 6          # csrc/nefii_tracer.hip
CREF_CAP = 76
NO_HASH = 0xFFFFFFFF


def kernel_hash(r, i):
    h = ((r * 2654435761) & 0xFFFFFFFF) ^ (((i + 1) * 0x9E3779B1) & 0xFFFFFFFF)
    return ((h ^ (h >> 15)) * 0x85EBCA6B) & 0xFFFFFFFF


class Row:
    def __init__(self, lo, hi, clo, chi, ok, exact, hashes):
        self.lo, self.hi, self.clo, self.chi = (np.asarray(a, dtype=F) for a in (lo, hi, clo, chi))
        self.ok = np.asarray(ok, dtype=bool)
        self.exact = np.asarray(exact, dtype=F)
        self.hashes = [int(h) for h in hashes]
        self.ns = len(self.lo)


def _limits(obj, miss_argmin, ns, j1, lo0, U):
    front_only = obj and j1 < ns and lo0 > 0
    sign_only = front_only or not miss_argmin
    lim = F(0) if sign_only else max(F(0), F(U + TAU))
    return lim, (j1 if front_only else ns - 1)


def sequential_bracket(row, frm, obj, miss_argmin, corners=True):
    """begin_grid_bracket -> (marks as a sorted tuple, n_near, probe, whole-row fallback)"""
    ns = row.ns
    v = np.empty(ns, dtype=F)
    j1, U, lo0 = ns, INF, F(0)
    for i in range(ns):
        lo, hi = (row.exact[i], row.exact[i]) if i < frm else (row.lo[i], row.hi[i])
        if hi < -TAU and j1 == ns:
            j1 = i
        U = min(U, hi)
        if i == 0:
            lo0 = lo
        v[i] = lo
    lim, last = _limits(obj, miss_argmin, ns, j1, lo0, U)
    if corners:
        for i in range(frm, last + 1):
            lb = v[i]
            if F(lb - F(1e-6)) > lim:
                continue
            if not row.ok[i]:
                continue
            v[i] = max(lb, row.clo[i])
            if i == 0:
                lo0 = v[i]
            U = min(U, row.chi[i])
            if row.chi[i] < -TAU and i < j1:
                j1 = i
                if obj and lo0 > 0:
                    break
        lim, last = _limits(obj, miss_argmin, ns, j1, lo0, U)
    marks, n_near, probe, probe_h = [], 0, -1, NO_HASH
    lim2 = F(lim + F(F(2) * TAU))
    for i in range(frm, ns):
        if i > last:
            continue
        x = F(v[i] - F(1e-6))
        if not x > lim:
            marks.append(i)
        elif n_near < NEAR_PROBES and not x > lim2:
            marks.append(i)
            n_near += 1
        elif row.hashes[i] < probe_h:
            probe_h, probe = row.hashes[i], i
    if probe >= 0:
        marks.append(probe)
        n_near += 1
    k = len(marks)
    fallback = not (0 < k <= CREF_CAP)
    return (() if fallback else tuple(sorted(marks))), n_near, probe, fallback


def _ballot(flags):
    return sum(1 << l for l, f in enumerate(flags) if f)


def _first(b0, b1, none):
    if b0:
        return (b0 & -b0).bit_length() - 1
    if b1:
        return 64 + (b1 & -b1).bit_length() - 1
    return none


def _popc(x):
    return bin(x).count('1')


def wave_bracket(row, frm, obj, miss_argmin, corners=True):
    """wave_grid_bracket: lane l of pass p holds sample 64 p + l"""
    ns = row.ns
    passes = 2 if ns > 64 else 1
    idx = [np.arange(64) + 64 * p for p in range(2)]
    inr = [idx[p] < ns if p < passes else np.zeros(64, bool) for p in range(2)]
    at = [np.minimum(idx[p], ns - 1) for p in range(2)]
    lb = [np.full(64, INF, dtype=F) for _ in range(2)]
    neg, U = [0, 0], INF
    for p in range(passes):
        lead = idx[p] < frm
        lo = np.where(lead, row.exact[at[p]], row.lo[at[p]]).astype(F)
        hi = np.where(lead, row.exact[at[p]], row.hi[at[p]]).astype(F)
        hi = np.where(inr[p], hi, INF)
        neg[p] = _ballot(inr[p] & (hi < -TAU))
        U = min(U, F(np.min(hi)))
        lb[p] = np.where(inr[p], lo, INF).astype(F)
    j1 = _first(neg[0], neg[1], ns)
    lo0 = lb[0][0]
    lim, last = _limits(obj, miss_argmin, ns, j1, lo0, U)
    if corners:
        negc = [0, 0]
        for p in range(passes):
            c = inr[p] & (idx[p] >= frm) & (idx[p] <= last) & ~((lb[p] - F(1e-6)).astype(F) > lim) & row.ok[at[p]]
            lb[p] = np.where(c, np.maximum(lb[p], row.clo[at[p]]), lb[p]).astype(F)
            chi = np.where(c, row.chi[at[p]], INF).astype(F)
            negc[p] = _ballot(c & (chi < -TAU))
            U = min(U, F(np.min(chi)))
        j1 = min(j1, _first(negc[0], negc[1], ns))
        lo0 = lb[0][0]
        lim, last = _limits(obj, miss_argmin, ns, j1, lo0, U)
    lim2 = F(lim + F(F(2) * TAU))
    act, surv, near, S, N = [None] * 2, [None] * 2, [None] * 2, [0, 0], [0, 0]
    for p in range(2):
        x = (lb[p] - F(1e-6)).astype(F)
        act[p] = inr[p] & (idx[p] >= frm) & (idx[p] <= last)
        surv[p] = act[p] & ~(x > lim)
        near[p] = act[p] & ~surv[p] & ~(x > lim2)
        S[p], N[p] = _ballot(surv[p]), _ballot(near[p])
    Sel, hh = [0, 0], [np.full(64, NO_HASH, dtype=np.uint64) for _ in range(2)]
    for p in range(2):
        before = np.array([(_popc(N[0]) if p else 0) + _popc(N[p] & ((1 << l) - 1)) for l in range(64)])
        sel = near[p] & (before < NEAR_PROBES)
        Sel[p] = _ballot(sel)
        pool = act[p] & ~surv[p] & ~sel
        for l in range(64):
            if pool[l]:
                hh[p][l] = row.hashes[64 * p + l]
    hmin = int(min(hh[0].min(), hh[1].min()))
    probe = _first(_ballot(hh[0] == hmin), _ballot(hh[1] == hmin), -1) if hmin != NO_HASH else -1
    m0 = S[0] | Sel[0] | ((1 << probe) if 0 <= probe < 64 else 0)
    m1 = S[1] | Sel[1] | ((1 << (probe - 64)) if probe >= 64 else 0)
    k = _popc(m0) + _popc(m1)
    n_near = _popc(Sel[0]) + _popc(Sel[1]) + (1 if probe >= 0 else 0)
    fallback = not (0 < k <= CREF_CAP)
    marks = tuple(i for i in range(128) if ((m0 >> i) & 1 if i < 64 else (m1 >> (i - 64)) & 1))
    return (() if fallback else marks), n_near, probe, fallback


def sequential_audit(evaluated, in_cube):
    """grid_audit: which samples get corner bounds"""
    got, n = [], 0
    for i in range(len(evaluated)):
        if not evaluated[i] or not in_cube[i]:
            continue
        if n < CREF_CAP:
            got.append(i)
            n += 1
    return tuple(got)


def wave_audit(evaluated, in_cube):
    ns = len(evaluated)
    el = [np.zeros(64, bool), np.zeros(64, bool)]
    for i in range(ns):
        el[i // 64][i % 64] = evaluated[i] and in_cube[i]
    E = [_ballot(el[0]), _ballot(el[1])]
    got = []
    for p in range(2):
        for l in range(64):
            before = (_popc(E[0]) if p else 0) + _popc(E[p] & ((1 << l) - 1))
            if el[p][l] and before < CREF_CAP:
                got.append(64 * p + l)
    return tuple(got)


def random_row(rng, ns, frm, kind):
    """bounds as a ray through an object gives them: a smooth profile, cell intervals around it, tighter corner bounds"""
    s = np.linspace(0, 1, ns)
    depth = {'hit': 0.25, 'graze': 0.02, 'miss': -0.05}[kind]
    f = (0.3 * np.abs(s - rng.uniform(0.3, 0.7)) - depth * rng.uniform(0.5, 1.5) + 0.02 * rng.standard_normal(ns) * (kind == 'graze'))
    wc, wk = rng.uniform(0.01, 0.08, ns), rng.uniform(0.0005, 0.02, ns)
    ok = rng.uniform(size=ns) > 0.03
    lo, hi = np.where(ok, f - wc, -np.inf), np.where(ok, f + wc, np.inf)
    r = int(rng.integers(0, 1 << 24))
    return Row(lo, hi, f - wk, f + wk, ok, f, [kernel_hash(r, i) for i in range(ns)])


def _same(row, frm, obj, miss, corners=True):
    a, b = sequential_bracket(row, frm, obj, miss, corners), wave_bracket(row, frm, obj, miss, corners)
    assert a == b, (frm, obj, miss, corners, a, b)
    return a


@pytest.mark.parametrize('ns', [40, 100, 128])
@pytest.mark.parametrize('frm', [0, 6])
def test_random_rows(ns, frm):
    rng = np.random.default_rng(100 * ns + frm)
    seen = {'fallback': 0, 'probe': 0, 'near': 0, 'front': 0}
    for n in range(600):
        row = random_row(rng, ns, frm, ('hit', 'graze', 'miss')[n % 3])
        for obj in (False, True):
            for miss in (False, True):
                for corners in (True, False):
                    marks, n_near, probe, fallback = _same(row, frm, obj, miss, corners)
                    seen['fallback'] += fallback
                    seen['probe'] += probe >= 0
                    seen['near'] += n_near > 1
                    seen['front'] += bool(marks) and max(marks) < ns - 1
    if ns <= CREF_CAP:       # (a row this short always fits the list)
        del seen['fallback']
    assert all(seen.values()), seen


def _flat(ns, lo, hi=None, r=5):
    """a row whose every sample has the cell interval (lo, hi) and corner bounds that change nothing"""
    hi = lo + 1.0 if hi is None else hi
    return Row(np.full(ns, lo), np.full(ns, hi), np.full(ns, -np.inf), np.full(ns, np.inf), np.ones(ns, bool),
               np.full(ns, 1.0), [kernel_hash(r, i) for i in range(ns)])


@pytest.mark.parametrize('ns', [40, 100, 128])
def test_j1_found_only_in_the_corner_pass(ns):
    row = _flat(ns, -0.05, 0.05)
    j = ns // 2 + 2          # (ns 128: in the second pass)
    row.chi[j], row.clo[j] = -0.01, -0.02
    row.lo[0], row.clo[0] = 0.01, 0.02           # sample 0 surely positive: front_only once j1 is known
    marks, _, probe, fallback = _same(row, 0, True, True)
    assert not fallback and max(m for m in marks if m != probe) == j
    assert _same(row, 0, False, True)[0] != marks      # outside the mask the samples behind j1 stay


@pytest.mark.parametrize('ns', [100, 128])
def test_the_break_case(ns):
    """obj and lo0 > 0: the sequential corner pass stops at the first surely negative candidate, the wave bounds them all -
    the candidates behind it lower U and raise bounds, and none of that may show"""
    row = _flat(ns, -0.05, 0.05)
    row.lo[0], row.clo[0] = -0.01, 0.02          # lo0 > 0 only through sample 0's corner bound
    a, b = 20, 70
    row.chi[a], row.clo[a] = -0.01, -0.02
    row.chi[b], row.clo[b] = -0.5, -0.6          # behind the break: a far lower hi, in the other pass
    row.clo[a + 1:] = 0.2                        # ... and bounds that would drop those samples
    marks, _, probe, fallback = _same(row, 0, True, True)
    assert not fallback and all(m <= a for m in marks)
    # leading exact samples: sample 0 holds its exact value, lo0 is fixed before the corner pass
    row.exact[:6] = 0.3
    marks, _, _, _ = _same(row, 6, True, True)
    assert all(6 <= m <= a for m in marks)
    # not inside the mask: no break, U falls to the far sample's
    _same(row, 0, False, True)


def test_more_near_misses_than_probes_over_both_passes():
    ns = 128
    row = _flat(ns, 0.5, 0.6)
    row.lo[3], row.hi[3] = -0.0005, 0.0005       # U ~ 0.0005: lim = U + tau
    lim = F(F(0.0005) + TAU)
    near = [10, 30, 60, 63, 64, 70, 90, 120]
    for i in near:
        row.lo[i] = lim + TAU                     # clears lim, not lim + 2 tau
    marks, n_near, probe, fallback = _same(row, 0, False, True)
    assert not fallback and n_near == NEAR_PROBES + 1
    assert set(marks) == set(near[:NEAR_PROBES]) | {3, probe}       # (the near misses past the sixth only as the hash probe)


@pytest.mark.parametrize('where', [(5, 40), (40, 100), (70, 100), (63, 64)])
def test_equal_hashes_keep_the_lowest_index(where):
    ns = 128
    row = _flat(ns, 0.5, 0.6)
    row.lo[0], row.hi[0] = -0.0005, 0.0005
    row.hashes = [1000 + 7 * ((i * 37) % ns) for i in range(ns)]
    for i in where:
        row.hashes[i] = 3
    marks, n_near, probe, fallback = _same(row, 0, False, True)
    assert probe == where[0] and n_near == 1 and marks == tuple(sorted((0, probe)))
    # a hash of all ones is never taken (hh < probe_h from ~0u)
    row.hashes = [NO_HASH] * ns
    marks, n_near, probe, _ = _same(row, 0, False, True)
    assert probe == -1 and n_near == 0 and marks == (0,)


@pytest.mark.parametrize('ns', [100, 128])
def test_more_survivors_than_the_list_takes(ns):
    row = _flat(ns, -0.05, 0.05)
    assert _same(row, 0, False, True) == ((), 0, -1, True)
    assert _same(row, 6, True, False)[3]
    # exactly CREF_CAP survive: listed
    row.lo[CREF_CAP:] = 0.5
    row.hashes = [NO_HASH] * ns
    marks, _, _, fallback = _same(row, 0, False, True)
    assert not fallback and len(marks) == CREF_CAP


@pytest.mark.parametrize('ns', [40, 100, 128])
def test_no_survivor_at_all(ns):
    """the front decides among the leading exact samples: nothing behind `from` is wanted - no round to wait for, whole row"""
    row = _flat(ns, 0.5, 0.6)
    row.exact[:6] = [0.3, 0.2, 0.1, -0.1, 0.2, 0.2]
    assert _same(row, 6, True, True) == ((), 0, -1, True)
    # every sample cleared, one hash probe only
    row.exact[:6] = 0.3
    marks, n_near, probe, fallback = _same(row, 6, True, False)
    assert not fallback and marks == (probe,) and n_near == 1


@pytest.mark.parametrize('ns', [40, 100, 128])
def test_audit_corner_choice(ns):
    rng = np.random.default_rng(ns)
    for density in (0.1, 0.5, 0.9, 1.0):
        for _ in range(200):
            ev = rng.uniform(size=ns) < density
            inc = rng.uniform(size=ns) < 0.9
            a, b = sequential_audit(ev, inc), wave_audit(ev, inc)
            assert a == b
    ev = np.ones(ns, bool)
    assert len(wave_audit(ev, ev)) == min(ns, CREF_CAP) and wave_audit(ev, ev) == sequential_audit(ev, ev)
