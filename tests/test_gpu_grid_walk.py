"""The walks over the SDF interval grid run by the whole wave (csrc/nefii_tracer.hip: serve_grid_walks, wave_grid_bracket,
wave_grid_audit) against the thread-per-ray form they restate (begin_grid_bracket, grid_audit;
NEFII_GRID_WALK_WAVE=0), on the GPU.  Only min, max, first index and counts are reordered, so EVERYTHING must agree: points,
hit mask and depths bit for bit, every column of the per-round counters, and the list of single samples (crefine) each round
leaves in the workspace - read round by round, since the list is reused.  Eval-mode traces (every bracket search walks) and
training-mode ones that read the grid (the rays inside the object mask walk), both tiers, on batches that end in, on and
behind a wave and a block of advance_kernel, with a searching ray pinned to the first and last lane of a wave and alone in its
wave.  tests/test_grid_walk_cpu.py holds the two selection rules to each other in NumPy."""
import ctypes
import functools

import pytest
import torch

from nefii_amd import _lib, ops
from nefii_amd.ops._call import _ptr, call

import test_gpu_bound_grid as grid
import test_gpu_bound_vertices as vertices
import test_gpu_minsdf_share as share

pytestmark = pytest.mark.gpu

DEV = grid.DEV
CREF_CAP = 76            # csrc/nefii_tracer.hip
SIZES = [1, 63, 64, 65, 255, 256, 257, 4096]


def _align(b):
    return (b + 255) // 256 * 256


def _crefine_offset(n, ns, cap):
    """where carve() puts the crefine list in a trace workspace (csrc/nefii_tracer.hip; a comment there points here).  cap: the
    refine list's entries per ray, coarse_cap()'s default of 64 for the parameters these tests make.  _by_round checks that the
    list ends inside the workspace the library sized; a wrong offset reads other memory and fails the list comparison."""
    off = (_lib.TRACE_WS_FLOAT_ARRAYS + 1) * _align(4 * n)               # the float arrays and the flags
    off += _align(4 * n * ns)                                             # big
    off += _align(8 * n) + 2 * _align(4 * n) + _align(16 * n)             # singles, dense, tri, cdense
    off += _align(4 * n * cap) + _align(8 * n) + _align(4 * ((n + 255) // 256))      # refine, csingles, block_live
    return off


_FROM_ARRAYS = object()


def _by_round(rt_cfg, pm, o, d, om, training, steps, tau, lip, tier, cells, verts, grid_training, descriptor=_FROM_ARRAYS):
    """one trace, enqueued a round at a time -> (points, hit, depths, counters [rounds, columns], crefine list of every round)
    descriptor: the nefii_trace_grid of the calls (None: a NULL pointer) in place of the one made of cells, verts, grid_training"""
    if descriptor is _FROM_ARRAYS:
        descriptor = _lib.TraceGrid(cells=_ptr(cells), vertex_g=_ptr(verts[0]), cell_l=_ptr(verts[1]), G=cells.shape[0],
                                    training=1 if grid_training else 0)
    grid_arg = None if descriptor is None else ctypes.byref(descriptor)
    tp = ops.make_tracer_params(rt_cfg, training, 'f16x3w', coarse_tau=tau, minsdf_lipschitz=lip, trace_tier=tier)
    lib = _lib.lib()
    n, ns = o.shape[0], tp.n_steps
    lin = torch.linspace(0, 1, steps=ns).to(DEV)
    o, d, om, steps = o.to(DEV).contiguous(), d.to(DEV).contiguous(), om.to(DEV).to(torch.uint8).contiguous(), steps.to(DEV)
    rounds = lib.nefii_trace_max_rounds(ctypes.byref(tp))
    nbytes = lib.nefii_trace_workspace_bytes(n, ctypes.byref(tp))
    ws = torch.zeros(nbytes, device=DEV, dtype=torch.uint8)
    pts = torch.empty(n, 3, device=DEV)
    hit = torch.empty(n, device=DEV, dtype=torch.uint8)
    dist = torch.empty(n, device=DEV)
    counters = torch.zeros(rounds, _lib.TRACE_COUNTERS, device=DEV, dtype=torch.int32)
    off = _crefine_offset(n, ns, 64)
    assert off + 4 * n * CREF_CAP <= nbytes
    lists = []
    for r in range(rounds):
        call('nefii_trace_rays_rounds', ctypes.byref(pm.struct), ctypes.byref(tp), _ptr(o), _ptr(d), _ptr(om), n,
             _ptr(lin), _ptr(steps), _ptr(pts), _ptr(hit), _ptr(dist), _ptr(ws), nbytes, _ptr(counters), r, r + 1, grid_arg)
        k = int(counters[r, _lib.CNT_COARSE_SAMPLES])
        lists.append(ws[off:off + 4 * k].view(torch.int32).cpu().clone())
    return pts.cpu(), hit.cpu(), dist.cpu(), counters.cpu().long(), lists


def _bowl():
    return vertices._bowl()


@functools.lru_cache(maxsize=None)
def _rays():
    """4096 rays, secondary-like ones (started on the surface) and primary-like ones alternating, ordered so that rays whose
    bracket search walks the grid and lists samples sit at 0, 63, 64, 255, 256 and 4095, and ray 64 is the only such ray of
    the second wave: found from the lists of an eval-mode trace in the thread-per-ray form"""
    import os
    mc, pm, tau, lip, cells, verts = _bowl()
    so, sd = grid._secondary()
    m = min(so.shape[0], 2048)
    po, pd = share._random(4096 - m, 33, spread=0.35)
    o, d = torch.cat([so[:m], po]), torch.cat([sd[:m], pd])
    perm = torch.randperm(4096, generator=torch.Generator().manual_seed(3))
    o, d = o[perm], d[perm]
    old = os.environ.get('NEFII_GRID_WALK_WAVE')
    os.environ['NEFII_GRID_WALK_WAVE'] = '0'
    try:
        lists = _by_round(mc['ray_tracer'], pm, o, d, torch.ones(4096, dtype=torch.bool), False, torch.rand(100), tau, lip, 0,
                          cells, verts, False)[4]
    finally:
        if old is None:
            del os.environ['NEFII_GRID_WALK_WAVE']
        else:
            os.environ['NEFII_GRID_WALK_WAVE'] = old
    walks = torch.zeros(4096, dtype=torch.bool)
    for entries in lists:
        walks[(entries.long() & 0xFFFFFFFF) >> 7] = True
    yes, no = torch.nonzero(walks).flatten().tolist(), torch.nonzero(~walks).flatten().tolist()
    assert len(yes) >= 64 and len(no) >= 64, (len(yes), len(no))
    order = [None] * 4096
    for pos in (0, 63, 64, 255, 256, 4095):
        order[pos] = yes.pop()
    for pos in range(65, 128):
        order[pos] = no.pop()
    rest = iter(sorted(yes + no))
    order = torch.tensor([next(rest) if x is None else x for x in order])
    g = torch.Generator().manual_seed(8)
    om = torch.rand(4096, generator=g) < 0.88
    om[[0, 63, 64, 255, 256, 4095]] = True
    return o[order], d[order], om, torch.rand(100, generator=g)


def _compare(what, rt_cfg, o, d, om, steps, monkeypatch):
    """wave against thread, eval mode and training mode with the grid, both tiers -> walks seen (rays listed per mode)"""
    mc, pm, tau, lip, cells, verts = _bowl()
    n = o.shape[0]
    seen = {}
    for training in (False, True):
        for tier in (0, 1):
            got = {}
            for wave in ('0', '1'):
                monkeypatch.setenv('NEFII_GRID_WALK_WAVE', wave)
                mask = om if training else torch.ones(n, dtype=torch.bool)
                got[wave] = _by_round(rt_cfg, pm, o, d, mask, training, steps, tau, lip, tier, cells, verts, training)
            a, b = got['0'], got['1']
            tag = (what, 'training' if training else 'eval', 'tier %d' % tier)
            for k, out in enumerate(('points', 'hit mask', 'depths')):
                assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                   b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), (tag, out)
            diff = torch.nonzero(a[3] != b[3])
            assert diff.numel() == 0, (tag, 'counters differ at (round, column)', diff[:8].tolist())
            assert grid._audit(b[3]) == 0.0, tag
            listed = 0
            for r, (la, lb) in enumerate(zip(a[4], b[4])):
                assert la.numel() == lb.numel(), (tag, r)
                # (a block's entries start where its atomicAdd on the round's counter lands: blocks may swap between two runs,
                # a single block may not)
                if n <= 256:
                    assert torch.equal(la, lb), (tag, 'crefine of round', r)
                else:
                    assert torch.equal(la.sort().values, lb.sort().values), (tag, 'crefine of round', r)
                listed += la.numel()
            seen[tag[1:]] = listed
    print('[grid walk %s] %d rays: samples listed over all rounds %s' % (what, n, seen))
    return seen


@pytest.mark.parametrize('n', SIZES)
def test_wave_walk_is_the_thread_walk(n, monkeypatch):
    mc = _bowl()[0]
    o, d, om, steps = _rays()
    seen = _compare('first %d' % n, mc['ray_tracer'], o[:n], d[:n], om[:n], steps, monkeypatch)
    assert all(v > 0 for v in seen.values()), seen      # (ray 0 walks: no case compares nothing)


@pytest.mark.parametrize('ns', [40, 128])
def test_wave_walk_with_one_and_two_passes(ns, monkeypatch):
    """n_steps 40: one pass with idle lanes; 128: two full passes"""
    mc = _bowl()[0]
    o, d, om, _ = _rays()
    cfg = dict(mc['ray_tracer'], n_steps=ns)
    seen = _compare('n_steps %d' % ns, cfg, o[:257], d[:257], om[:257], torch.rand(ns, generator=torch.Generator().manual_seed(ns)),
                    monkeypatch)
    assert all(v > 0 for v in seen.values()), seen


def test_no_grid_is_spelled_three_ways():
    """A NULL descriptor, an all-zero one and one whose cells are NULL are the same trace: no grid.  The third carries what a
    descriptor may carry without cells - the block level, a counter array, G, the training word; the vertex arrays without
    cells are refused (NEFII_E_ARG), as they always were."""
    mc, pm, tau, lip, cells, verts = _bowl()
    o, d, om, steps = _rays()
    blocks = ops.build_bound_grid_blocks(cells)
    counts = torch.zeros(ops.CERTIFY_COUNTS, device=DEV, dtype=torch.int32)
    everything = torch.ones(o.shape[0], dtype=torch.bool)

    def trace(descriptor):
        return _by_round(mc['ray_tracer'], pm, o, d, everything, False, steps, tau, lip, 0, cells, verts, False, descriptor)

    null = trace(None)
    zero = trace(_lib.TraceGrid())
    headless = trace(_lib.TraceGrid(cells=None, blocks=_ptr(blocks), certify_counts=_ptr(counts), G=cells.shape[0], training=1))
    for name, got in (('all-zero descriptor', zero), ('descriptor without cells', headless)):
        for k, out in enumerate(('points', 'hit mask', 'depths')):
            assert torch.equal(null[k].view(torch.int32) if null[k].dtype == torch.float32 else null[k],
                               got[k].view(torch.int32) if got[k].dtype == torch.float32 else got[k]), (name, out)
        assert torch.equal(null[3], got[3]), (name, 'counters')
    assert int(null[1].sum()) > 0 and int(counts.sum()) == 0
    with pytest.raises(RuntimeError, match='bad argument'):
        trace(_lib.TraceGrid(cells=None, vertex_g=_ptr(verts[0]), cell_l=_ptr(verts[1]), G=cells.shape[0]))
