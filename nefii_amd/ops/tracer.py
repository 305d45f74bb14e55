"""The round tracer: its parameters and counters, the stream and round bookkeeping of trace_rays, camera rays."""
import ctypes

import torch

from .. import _lib
from .._lib import TracerParams
from ._call import _f32, _ptr, call, need_gpu
from ._call import nbytes as _nbytes


def algorithmic_evals(counters, n_steps):
    """SDF evaluations the reference's recurrences need for the rounds in `counters` [..., rounds, _lib.TRACE_COUNTERS]
    (columns _lib.CNT_*; what frac_credited credits): singles + tiered singles taken (those not repeated) + n_steps per dense
    search entered + bisection steps consumed."""
    c = counters.long()
    return (c[..., _lib.CNT_SINGLES] + c[..., _lib.CNT_COARSE_SINGLES] - c[..., _lib.CNT_REPEATS]
            + c[..., _lib.CNT_SEARCHES] * n_steps + c[..., _lib.CNT_BISECT_USED])


def executed_evals(counters, n_steps, tri_nodes=None):
    """(split-precision evaluations, coarse single-pass evaluations) actually executed (tri_nodes: unused, the tracer
    counts its speculative bisection evaluations itself)."""
    c = counters.long()
    split = c[..., _lib.CNT_SINGLES] + c[..., _lib.CNT_DENSE_ROWS] * n_steps + c[..., _lib.CNT_BISECT_EVALS] + c[..., _lib.CNT_REFINED]
    coarse = (c[..., _lib.CNT_COARSE_WINDOWS] * ((n_steps + 3) // 4) + c[..., _lib.CNT_COARSE_SINGLES]
              + c[..., _lib.CNT_COARSE_SAMPLES])
    return split, coarse


PRECISIONS = {'f32': 0, 'f16x3': 1, 'f16x3w': 2}


def make_tracer_params(cfg, training, precision='f32', bisect_levels=3, coarse_tau=0.0, coarse_cap=0, minsdf_group=0,
                       small_round=0, trace_tier=0, tier_kappa=0.0, tier_gate=0.0, minsdf_lipschitz=0.0, unread_misses=0,
                       split_fp8=0):
    p = TracerParams()
    p.split_fp8 = 1 if split_fp8 else 0
    p.unread_misses = 1 if unread_misses else 0
    p.minsdf_lipschitz = float(minsdf_lipschitz) if coarse_tau > 0.0 else 0.0
    p.trace_tier = 1 if (trace_tier and coarse_tau > 0.0) else 0
    p.tier_kappa = float(tier_kappa)
    p.tier_gate = float(tier_gate)
    p.minsdf_group = int(minsdf_group)
    p.small_round = int(small_round)
    p.precision = PRECISIONS[precision]
    p.bisect_levels = bisect_levels
    p.coarse_tau = float(coarse_tau)
    p.coarse_cap = int(coarse_cap)
    p.object_bounding_sphere = cfg.get('object_bounding_sphere', 1.0)
    p.sdf_threshold = cfg.get('sdf_threshold', 5.0e-5)
    p.line_search_step = cfg.get('line_search_step', 0.5)
    p.line_step_iters = cfg.get('line_step_iters', 1)
    p.sphere_tracing_iters = cfg.get('sphere_tracing_iters', 10)
    p.n_steps = cfg.get('n_steps', 100)
    p.n_rootfind_steps = cfg.get('n_rootfind_steps', 8)
    p.training = 1 if training else 0
    return p


class TraceRounds:
    """Adaptive prefix of the tracer's rounds.  Every round after the last one that emitted a query is an empty
    launch pair (~12 us); callers that synchronise right after the trace anyway (the renderer compacts the hits)
    run rounds [0, guess), read three counters and continue only if a ray is still waiting - which the guess,
    taken from the previous call, makes rare.  Results never depend on the guess."""

    def __init__(self):
        self.guess = None


_TRACE_STREAMS = {}
_WORK = _lib.CNT_WORK             # counter columns that mean "a ray still waits for an evaluation"


_SIDE_STREAMS = {}


def side_stream(dev):
    """One process-wide side stream per device for work that may run beside the caller's serial chain (a detached radiance
    forward, model/implicit_differentiable_renderer.py:get_rbg_value)."""
    key = torch.device(dev).index if torch.device(dev).index is not None else torch.cuda.current_device()
    st = _SIDE_STREAMS.get(key)
    if st is None:
        st = _SIDE_STREAMS[key] = torch.cuda.Stream(device=key)
    return st


def _trace_streams(dev, n):
    pool = _TRACE_STREAMS.setdefault(dev, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=dev))
    return pool[:n]


def sum_counters(a, b=None):
    """Counters of several stream groups (a: [groups, rounds, C] -> [rounds, C]) or of two traces (a + b, [rounds, C]):
    the counts add, the columns _lib.CNT_MAXIMA - the bits of a non-negative float, the audits' maxima - take the maximum
    (the bit patterns of non-negative floats order like the floats)."""
    if b is None:
        out = a.sum(dim=0)
        for col in _lib.CNT_MAXIMA:
            out[..., col] = a[..., col].max(dim=0).values
        return out
    out = a + b
    for col in _lib.CNT_MAXIMA:
        out[..., col] = torch.maximum(a[..., col], b[..., col])
    return out


def _lip_audit_of(host_counters):
    """Largest amount by which a second-stage depth of a staged min-SDF search fell below the lower bound the claimed
    Lipschitz constant gave it (_lib.CNT_LIP_AUDIT: float bits; 0 = the bound held wherever it was checked)."""
    col = host_counters[..., _lib.CNT_LIP_AUDIT].contiguous().view(torch.float32)
    return float(col.max()) if col.numel() else 0.0


def _audit_of(host_counters):
    """Largest |coarse - split| the tracer saw among the coarse samples it re-evaluated (_lib.CNT_TAU_AUDIT: float bits)."""
    col = host_counters[..., _lib.CNT_TAU_AUDIT].contiguous().view(torch.float32)
    return float(col.max()) if col.numel() else 0.0


def _chunks_with_work(host, guess):
    """Of the counters [groups, rounds, columns] behind rounds [0, guess): the chunks in whose round guess - 1 a ray still
    waited for an evaluation - none when the guess was every round."""
    if guess >= host.shape[1]:
        return []
    return [g for g in range(host.shape[0]) if int(host[g, guess - 1, _WORK].sum()) > 0]


def _next_guess(host):
    """The round prefix to enqueue next time: the last round in which any chunk had work, its consumer and one spare."""
    busy = torch.nonzero(host[:, :, _WORK].sum(dim=(0, 2))).flatten()
    return (int(busy[-1]) if busy.numel() else 0) + 3


BOUND_GRID_SIZE = 256            # cells per edge of the SDF interval grid: 4 G^3 bytes (67 MB); profiles/bound_grid/README.md
BOUND_GRID_L_FLOOR = 1.0         # least slope bound of a cell: a distance function's
BOUND_GRID_SAFETY = 1.5          # finite differences over a grid edge understate the steepest slope along it (LIPSCHITZ_SAFETY)


def build_bound_grid(pm_sdf, radius, tau, G=BOUND_GRID_SIZE, l_floor=BOUND_GRID_L_FLOOR, safety=BOUND_GRID_SAFETY,
                     vertices=False):
    """The SDF interval grid of a frozen network (include/nefii_amd.h: nefii_sdf_bound_grid_build) -> int32 [G, G, G], one word
    per cell of the cube [-radius, radius]^3: fp16 lo | fp16 hi << 16 with lo <= sdf <= hi over the cell.  tau: the network's
    coarse_tau.  Enqueued on the current stream; the workspace ((G+1)^3 floats and a slab of points) is freed behind it.

    vertices: -> (that tensor, (fp16 [G+1, G+1, G+1] single-pass values at the vertices, fp16 [G, G, G] slope bound per cell)),
    the arrays of nefii_sdf_bound_grid_build_vertices: trace_rays(bound_vertices=...) bounds a sample from its cell's corners."""
    dev = pm_sdf.device
    cells = torch.empty(G, G, G, device=dev, dtype=torch.int32)
    ws = torch.empty(_nbytes('nefii_sdf_bound_grid_workspace_bytes', G), device=dev, dtype=torch.uint8)
    if not vertices:
        call('nefii_sdf_bound_grid_build', ctypes.byref(pm_sdf.struct), G, float(radius), float(tau), float(l_floor), float(safety),
             _ptr(cells), _ptr(ws))
        return cells
    vert_g = torch.empty(G + 1, G + 1, G + 1, device=dev, dtype=torch.float16)
    cell_l = torch.empty(G, G, G, device=dev, dtype=torch.float16)
    call('nefii_sdf_bound_grid_build_vertices', ctypes.byref(pm_sdf.struct), G, float(radius), float(tau), float(l_floor),
         float(safety), _ptr(cells), _ptr(vert_g), _ptr(cell_l), _ptr(ws))
    return cells, (vert_g, cell_l)


BOUND_GRID_BLOCK = 4             # cells per edge of a block of the grid's block level (NEFII_BOUND_GRID_BLOCK)
CERTIFY_COUNTS = 4               # NEFII_CERTIFY_COUNTS: crossed rays certified, their block look-ups; rays ended as free, their look-ups


def build_bound_grid_blocks(cells):
    """The block level over an SDF interval grid (nefii_sdf_bound_grid_blocks): cells int32 [G, G, G] -> fp16 [Gb, Gb, Gb],
    Gb = ceil(G / BOUND_GRID_BLOCK), the least lo of each block's cells.  Enqueued on the current stream."""
    G = cells.shape[0]
    gb = _lib.lib().nefii_sdf_bound_grid_block_count(G)
    if gb <= 0 or tuple(cells.shape) != (G, G, G) or cells.dtype != torch.int32:
        raise ValueError('build_bound_grid_blocks: cells must be build_bound_grid\'s int32 [G, G, G]')
    blocks = torch.empty(gb, gb, gb, device=cells.device, dtype=torch.float16)
    call('nefii_sdf_bound_grid_blocks', _ptr(cells), G, _ptr(blocks))
    return blocks


def trace_rays(pm_sdf, params, origins, dirs, object_mask, lin_steps, minsdf_steps=None, want_counters=False,
               rounds_state=None, groups=1, deferred=None, audit=None, keep_workspace=None, bound_grid=None,
               bound_vertices=None, bound_grid_training=False, bound_grid_certify=None, certify_counts=None, certify_parts=3):
    """RayTracing.forward for per-ray origins.  Returns points [n,3], hit (bool [n]), dists [n] (+ counters).

    groups > 1: the rays are cut into that many contiguous chunks that run their rounds on separate HIP streams
    (nefii_trace_rays_groups).  Rays are independent, so the results are bit-identical; the latency-bound rounds of a
    small batch (fewer 64-query tiles than CUs, one tile time per round regardless) of different chunks then overlap
    on the chip.  On MI355X the dense rounds lose as much as that gains (RayTracing.stream_groups), so it is off by
    default.

    audit (a callable, with rounds_state): called with the largest |coarse - split| of this trace's refined samples whenever
    the counters reach the host (the online check of nefii_tracer_params.coarse_tau: ImplicitNetwork.note_coarse_audit).

    bound_grid (build_bound_grid's tensor, of the weights in pm_sdf and of params.object_bounding_sphere): the staged bracket
    searches of an eval-mode trace (params.minsdf_lipschitz > 0) read their first stage from it instead of evaluating one.
    bound_vertices (build_bound_grid(vertices=True)'s pair, with its bound_grid): the samples the cell intervals leave
    undecided are bounded from the corners of their cells before anything is evaluated.
    bound_grid_training: a training-mode trace reads bound_grid too - the bracket searches of its rays inside the object mask
    (nefii_trace_grid.training); without it such a trace ignores the grid.

    bound_grid_certify (build_bound_grid_blocks' tensor of bound_grid): a training-mode trace ends the rays whose two fronts the
    block level proves to cross within sphere_tracing_iters in round 0, before any sphere-tracing query - they go straight to
    their min-SDF search, which audits what it evaluates against the cells (nefii_trace_grid.certify).  Eval-mode traces
    whose misses are read ignore it; one with params.unread_misses ends, at every sphere-tracing iteration, the rays whose
    remaining stretch to the bounding sphere the grid proves free of the surface - as misses, with one ray in 16 probed for the
    audit.  certify_parts: bit 0 the crossing certificate, bit 1 the free-stretch one.  certify_counts (int32 [CERTIFY_COUNTS] on
    the device, zeroed by the caller): added to - crossed rays certified, their block look-ups, rays ended as free, their look-ups.

    keep_workspace (a list): receives (workspace tensor, first ray, rays) per chunk - measurement tools read ray state from it
    (trace_iterations below).

    deferred (a list, with rounds_state): the call enqueues the guessed round prefix and returns WITHOUT reading the
    counters back; it appends a callable that, invoked once the work has completed, tells whether that prefix was the
    whole trace (and refreshes the guess).  For callers that trace ahead of time on a side stream
    (training/step.py:prefetch_traces) and cannot afford a host sync there."""
    lib = _lib.lib()
    n = origins.shape[0]
    dev = origins.device
    pts = torch.empty(n, 3, device=dev, dtype=torch.float32)
    hit = torch.empty(n, device=dev, dtype=torch.uint8)
    dist = torch.empty(n, device=dev, dtype=torch.float32)
    rounds = lib.nefii_trace_max_rounds(ctypes.byref(params))
    # (inside a stream capture nothing may be read back: a capture of the non-adaptive path runs without the audit - its counters
    # would need a host copy - and the caller audits an eager trace of the same weights instead)
    if audit is not None and rounds_state is None and torch.cuda.is_current_stream_capturing():
        audit = None
    need_cnt = want_counters or rounds_state is not None or audit is not None
    groups = max(1, min(int(groups), n // 64)) if n > 0 else 1
    counters = torch.zeros(groups, rounds, _lib.TRACE_COUNTERS, device=dev, dtype=torch.int32) if need_cnt else None
    if n > 0:
        om = object_mask.to(torch.uint8).contiguous()
        per = -(-n // groups)
        per = -(-per // 64) * 64
        bounds = [(g * per, min(n, (g + 1) * per)) for g in range(groups) if g * per < n]
        cur = torch.cuda.current_stream(dev)
        streams = [cur] if len(bounds) == 1 else _trace_streams(dev, len(bounds))
        if len(bounds) > 1:
            start = cur.record_event()
        work = []
        for g, (lo, hi) in enumerate(bounds):
            with torch.cuda.stream(streams[g]):
                if len(bounds) > 1:
                    streams[g].wait_event(start)
                nbytes = lib.nefii_trace_workspace_bytes(hi - lo, ctypes.byref(params))
                work.append((torch.empty(nbytes, device=dev, dtype=torch.uint8), nbytes))

        if keep_workspace is not None:
            keep_workspace.extend((w, lo, hi - lo) for (w, _), (lo, hi) in zip(work, bounds))
        G = len(bounds)
        begin = (ctypes.c_int64 * (G + 1))(*([lo for lo, _ in bounds] + [n]))
        ws_ptrs = (ctypes.c_void_p * G)(*[w.data_ptr() for w, _ in work])
        ws_bytes = (ctypes.c_size_t * G)(*[b for _, b in work])
        st_ptrs = (ctypes.c_void_p * G)(*[st.cuda_stream for st in streams])
        cells, cells_n = (_ptr(bound_grid), bound_grid.shape[0]) if bound_grid is not None else (None, 0)
        vert_g, cell_l = (None, None) if bound_vertices is None else (_ptr(bound_vertices[0]), _ptr(bound_vertices[1]))
        if bound_vertices is not None and (bound_grid is None or bound_vertices[0].shape[0] != cells_n + 1 or
                                           bound_vertices[1].shape[0] != cells_n):
            raise ValueError('bound_vertices: the arrays of build_bound_grid(vertices=True), with their bound_grid')
        blocks, certify = (_ptr(bound_grid_certify), int(certify_parts) & 3) if bound_grid_certify is not None else (None, 0)
        if certify and (bound_grid is None or bound_grid_certify.shape[0] != -(-cells_n // BOUND_GRID_BLOCK)):
            raise ValueError('bound_grid_certify: the tensor of build_bound_grid_blocks(bound_grid), with its bound_grid')
        # one descriptor per call (nefii_trace_grid); without a grid the library gets NULL
        grid = None if bound_grid is None else ctypes.byref(_lib.TraceGrid(
            cells=cells, vertex_g=vert_g, cell_l=cell_l, blocks=blocks, certify_counts=_ptr(certify_counts) if certify else None,
            G=cells_n, training=1 if bound_grid_training else 0, certify=certify))

        def run(sel, r0, r1):
            """rounds [r0, r1) of the chunks in `sel`, enqueued round-major by one library call"""
            if len(sel) == G and G > 1:
                b_, w_, wb_, s_, c_ = begin, ws_ptrs, ws_bytes, st_ptrs, counters
                call('nefii_trace_rays_groups', ctypes.byref(pm_sdf.struct), ctypes.byref(params), _ptr(origins), _ptr(dirs),
                     _ptr(om), G, b_, _ptr(lin_steps), _ptr(minsdf_steps), _ptr(pts), _ptr(hit), _ptr(dist), w_, wb_,
                     _ptr(c_) if c_ is not None else None, r0, r1, grid, stream=s_)
                return
            for g in sel:
                lo, hi = bounds[g]
                ws, nbytes = work[g]
                call('nefii_trace_rays_rounds', ctypes.byref(pm_sdf.struct), ctypes.byref(params), _ptr(origins[lo:hi]),
                     _ptr(dirs[lo:hi]), _ptr(om[lo:hi]), hi - lo, _ptr(lin_steps), _ptr(minsdf_steps), _ptr(pts[lo:hi]),
                     _ptr(hit[lo:hi]), _ptr(dist[lo:hi]), _ptr(ws), nbytes, _ptr(counters[g]) if counters is not None else None,
                     r0, r1, grid, stream=streams[g].cuda_stream)

        def join():
            for st in streams:
                if st is not cur:
                    cur.wait_event(st.record_event())

        def pinned_counters():
            """the counters travel to pinned host memory behind the enqueued rounds, on the stream of the trace: a deferred
            check then reads them without a copy on the CALLER'S stream (which would wait for whatever that stream still has
            to run - the previous step's tail)"""
            ahead = torch.empty(counters.shape, dtype=counters.dtype, pin_memory=True)
            return ahead.copy_(counters, non_blocking=True)

        def tell(host):
            if audit is not None:
                audit(_audit_of(host), _lip_audit_of(host))

        everyone = list(range(G))
        if rounds_state is None:
            run(everyone, 0, 0)
            join()
            if audit is not None:
                # the non-adaptive path has no counter read-back of its own.  A caller that hands in a `deferred` list gets the
                # audit there (run once the work has completed); otherwise one host sync
                if deferred is not None:
                    deferred.append(lambda ahead=pinned_counters(): tell(ahead))
                else:
                    tell(counters.cpu())
        else:
            guess = rounds if rounds_state.guess is None else max(2, min(rounds, rounds_state.guess))
            run(everyone, 0, guess)
            join()

            def settle(host, wait):
                """with the counters of the enqueued prefix on the host: the chunks that still have work run their remaining
                rounds (same streams, same workspaces), the guess is refreshed and the audit told.  Returns those chunks."""
                again = _chunks_with_work(host, guess)
                if again:
                    run(again, guess, 0)
                    wait()
                    host = counters.cpu()
                rounds_state.guess = _next_guess(host)
                tell(host)
                return again

            def sync_streams():
                for st in streams:
                    st.synchronize()

            if deferred is not None:
                ahead = pinned_counters()
                # call once the enqueued prefix has completed: None if it was the whole trace, else the refreshed outputs
                deferred.append(lambda: (pts, hit.bool(), dist) if settle(ahead, sync_streams) else None)
            else:
                settle(counters.cpu(), join)                 # the one host sync (the caller syncs next anyway)
    if want_counters:
        return pts, hit.bool(), dist, sum_counters(counters)
    return pts, hit.bool(), dist


def trace_iterations(kept):
    """Sphere-tracing iterations each ray took, from the workspaces a finished trace_rays(keep_workspace=kept) left: the
    tracer parks the count at bit _lib.TRACE_ITER_SHIFT (4 bits) of a ray's flag word when its sphere tracing ends
    (csrc/nefii_tracer.hip; the flag array follows _lib.TRACE_WS_FLOAT_ARRAYS float arrays of n rays, each padded to 256
    bytes).  Measurement only (tools/tier_parity.py)."""
    out = []
    for ws, _lo, n in kept:
        stride = (4 * n + 255) // 256 * 256
        begin = _lib.TRACE_WS_FLOAT_ARRAYS * stride
        flags = ws[begin:begin + 4 * n].view(torch.int32)
        out.append((flags >> _lib.TRACE_ITER_SHIFT) & 0xF)
    return torch.cat(out)


def camera_rays(uv, pose, intrinsics):
    """uv [B,S,2], pose [B,4,4], K [B,4,4] -> dirs [B,S,3], per-ray origins [B,S,3]."""
    need_gpu(uv, pose, intrinsics)
    if uv.dim() != 3 or uv.shape[2] != 2 or tuple(pose.shape) != (uv.shape[0], 4, 4) or \
            tuple(intrinsics.shape) != (uv.shape[0], 4, 4):
        raise ValueError('camera_rays: uv is [B, S, 2], pose and intrinsics are [B, 4, 4]; got %s, %s, %s'
                         % (tuple(uv.shape), tuple(pose.shape), tuple(intrinsics.shape)))
    B, S, _ = uv.shape
    dirs = torch.empty(B, S, 3, device=uv.device, dtype=torch.float32)
    orig = torch.empty(B, S, 3, device=uv.device, dtype=torch.float32)
    uv_c, pose_c, k_c = _f32(uv), _f32(pose), _f32(intrinsics)      # converted copies must outlive the launch call
    if B * S > 0:       # (an empty tensor has no address: the entry point would take its NULL for a missing argument)
        call('nefii_camera_rays', _ptr(uv_c), _ptr(pose_c), _ptr(k_c), B, S, _ptr(dirs), _ptr(orig))
    return dirs, orig
