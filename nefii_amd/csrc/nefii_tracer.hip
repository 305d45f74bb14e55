// nefii_tracer.hip - SDF ray tracer for gfx950: RayTracing.forward of the reference
// (code/model/ray_tracing.py:29-337) restated as a per-ray state machine driven in ROUNDS.
//
// Every round is two launches on one stream, with no host synchronisation:
//   advance : one thread per ray.  Consumes the SDF values its ray asked for in the previous round,
//             moves the ray's state machine (sphere tracing both ends + back-off line search ->
//             100-sample bracket search -> bisection -> min-SDF search) and appends the ray's next
//             SDF queries to a compacted work list (wave ballot + prefix popcount, one atomic per block).
//   eval    : the fused SDF MLP (mlp_tile.h) over dense 32-query tiles of that list - rays in different
//             phases share tiles, so the matrix cores only ever see live queries.
// Ray state is a few floats per ray in global memory (L2 resident); all heavy traffic is the MLP.
// Arithmetic order follows the reference exactly (separate multiply and add for o + t*d etc.); the
// only semantic difference is that bisection stops per ray instead of when the whole batch converged.
#include <cstdlib>
#include <vector>

#include "sdf_launch.h"
#include "hip_check.h"

using namespace nefii;

namespace {

// PH_SAMPLER_C / PH_MINSDF_C: the ray's n_steps samples are being evaluated by the single-pass (coarse) evaluator; the
// exact phases PH_SAMPLER / PH_MINSDF follow once the samples that decide have been re-evaluated in split precision
// PH_SAMPLER_X: the bracket search's FIRST `chunk` samples are being evaluated in split precision (through the refine
// list) before anything else: sphere tracing stops right in front of the surface, so the first negative sample is one of the
// first few for most rays that have one (median index 1-3 of 100 on the bench scenes) - and the reference's decision then
// depends on no later sample.  A ray without a negative sample among them goes on to PH_SAMPLER_C as before.
enum Phase : int { PH_DONE = 0, PH_TRACE = 1, PH_SAMPLER = 2, PH_BISECT = 3, PH_MINSDF = 4, PH_SAMPLER_C = 5, PH_MINSDF_C = 6,
                   PH_SAMPLER_X = 7 };
// local to advance_kernel, never stored: the stage behind tracing / sampler / bisection; nothing more to do this round
constexpr int PH_POST = 100, PH_WAIT = -1;
constexpr int NCNT = NEFII_TRACE_COUNTERS;
constexpr int NEAR_PROBES = 6;     // skipped samples per staged search that the audit evaluates because their bound cleared the limit by < 2 tau
enum Kind : int { Q_START = 0, Q_END = 1, Q_MID = 2 };
enum Walk : int { WALK_NONE = 0, WALK_BEGIN = 1, WALK_AUDIT = 2 };      // Emit::walk

// ops.trace_iterations (nefii_amd/ops/tracer.py) reads the sphere-tracing iteration count out of a kept workspace: the flag words
// follow RayState's TRACE_WS_FLOAT_ARRAYS float arrays, the count sits at F_K_SHIFT = TRACE_ITER_SHIFT
// (mirrored as _lib.TRACE_WS_FLOAT_ARRAYS / _lib.TRACE_ITER_SHIFT)
constexpr int TRACE_WS_FLOAT_ARRAYS = 13, TRACE_ITER_SHIFT = 20;
struct RayState {            // SoA views into the workspace
    float *t_s, *t_e, *cur_s, *cur_e, *nxt_s, *nxt_e, *t_min, *t_max, *res_s, *res_e, *lo, *hi, *mid;
    int *flags;              // phase | live/pending bits | counters (packed, see below)
    float *big;              // [n][n_steps] dense query results
    unsigned *singles;       // [2n]  (ray << 2 | kind)
    unsigned *dense;         // [n]   (ray << 1 | which)  which: 0 sampler, 1 min-sdf
    unsigned *tri;           // [n]   rays in bisection: 7 speculative queries each (3 levels of the bisection tree)
    unsigned *cdense;        // [4n]  (window << 29 | ray << 1 | which): quarter rows (CW samples of a ray's n_steps) for the coarse evaluator
    unsigned *refine;        // [n * cap]  (ray << 7 | sample): coarse samples to re-evaluate in split precision
    unsigned *csingles;      // [2n]  (ray << 2 | kind): sphere-tracing queries for the coarse evaluator (tiered sphere tracing)
    int *block_live;         // [ceil(n / 256)]  advance_kernel: does this block still hold a ray that is not done?
    unsigned *crefine;       // [n * CREF_CAP]  (ray << 7 | sample): single samples for the COARSE evaluator (staged min-SDF search)
    unsigned char *ord;      // [groups][n_steps]  staged min-SDF search: ord[k] = index of the k-th smallest of the group's draws
};
// staged searches: most second-stage samples of one ray (a ray with more takes its whole row, as without the staging)
constexpr int CREF_CAP = 76;       // (n_steps 100: the 75 depths outside the first stage + the probe - no search falls back)

// flags layout
constexpr int F_PHASE = 0x7;          // bits 0-2
constexpr int F_LIVE_S = 1 << 3, F_LIVE_E = 1 << 4, F_PEND_S = 1 << 5, F_PEND_E = 1 << 6;
constexpr int F_STEPPED = 1 << 7;     // results belong to a step / back-off (not the initial evaluation)
constexpr int F_SPH = 1 << 8, F_SAMP = 1 << 9, F_HIT = 1 << 10;
// behind sphere tracing (which clears F_STEPPED when it ends) the bit says that the ray never traced: the SDF interval grid
// proved in round 0 that its fronts cross (certify_crossing) - its min-SDF search audits what it evaluates (certify_audit)
constexpr int F_CERT = F_STEPPED;
// min-SDF search: the ray runs / ran a staged search of its OWN - once its row is in, the rays of its wave may take their
// bounds from it (shared first stage, minsdf_share); set when its first stage goes out, cleared with the rest by end_trace
constexpr int F_OWN = 1 << 11;      // (in PH_TRACE of an eval-mode trace the bit is F_PROBE, certify_free_stretch's: such a ray never reaches the min-SDF search)
constexpr int F_IT_SHIFT = 12, F_IT_MASK = 0xFF;     // sphere-tracing iteration / bisection step
constexpr int F_K_SHIFT = TRACE_ITER_SHIFT, F_K_MASK = 0xF;        // back-off count
// the sub-stage of PH_SAMPLER_C / PH_MINSDF_C: what is with the coarse evaluator
constexpr int F_WIN_SHIFT = 24, F_WIN_MASK = 0x7;
enum SamplerWin : int {      // PH_SAMPLER_C
    SW_WHOLE_ROW = 0,                                                  // the whole row
    SW_WINDOW_1 = 1, SW_WINDOW_2 = 2, SW_WINDOW_3 = 3, SW_WINDOW_4 = 4,    // windowed search: the first w quarter rows
    SW_STAGE1 = 5, SW_STAGE2 = 6,                                      // first / second stage of the staged bracket search (minsdf_lipschitz)
    SW_GRID = 7                                                        // the samples the SDF interval grid did not decide are out (begin_grid_bracket)
};
enum MinSdfWin : int {       // PH_MINSDF_C
    MW_ROW_IN = 0,                  // the row's coarse values are in
    MW_SECOND = 1,                  // second stage of the two-stage refinement (its sample index is parked in the F_IT bits)
    MW_STAGE1 = 2, MW_STAGE2 = 3,   // first / second stage of the staged search (minsdf_lipschitz)
    MW_ENTER = 4,                   // shared first stage: the search is entered, no depth is out yet - the ray looks for a donor
    MW_SHARED = 5                   //   the candidates its donor's row left are out (the donor's lane is parked in the F_IT bits)
};
__device__ __forceinline__ int win_of(int fl) { return (fl >> F_WIN_SHIFT) & F_WIN_MASK; }
__device__ __forceinline__ int with_win(int fl, int w) { return (fl & ~(F_WIN_MASK << F_WIN_SHIFT)) | (w << F_WIN_SHIFT); }
constexpr int CWIN_STAGE1 = 4;        // cdense window code: the first stage's depths of a staged min-SDF search
// Tiered sphere tracing (nefii_tracer_params.trace_tier), PH_TRACE only.  F_CRS_x: the pending result of that end comes from
// the single-pass evaluator.  F_AUD_x: that end's query is being REPEATED in split precision this round and res_x still
// holds the coarse value (the split evaluator compares the two: the online audit of coarse_tau).
constexpr int F_CRS_S = 1 << 27, F_CRS_E = 1 << 28, F_AUD_S = 1 << 29, F_AUD_E = 1 << 30;
// samples per quarter row (window) of a coarse row
__host__ __device__ __forceinline__ int coarse_window(int n_steps) { return (n_steps + 3) >> 2; }

struct Params {
    nefii_tracer_params p;
    int64_t n;
    const float *o, *d;
    const uint8_t *obj;
    const float *lin, *steps;
    float *out_pts, *out_dist;
    uint8_t *out_hit;
    int *counters;           // [rounds][NEFII_TRACE_COUNTERS], columns NEFII_CNT_*
    int levels, tri_nodes;   // speculative bisection: levels per round, nodes = 2^levels - 1
    float tau;               // coarse pass: error bound of a coarse sample (0: coarse pass off)
    int cap;                 //              most samples of one ray refined individually
    int chunk;               //              leading samples of a bracket search evaluated exactly first (0: off)
    float chunk_gate;        //              ... for rays whose front SDF is below chunk_gate x the chunk's reach
    int window;              //              bracket searches inside the object mask take their coarse samples a quarter row at a time
    float tier_band;         // tiered sphere tracing: a coarse value v16 decides (v > thr, sign) when |v16| > tier_band; 0: off
    float tier_gate;         //              a step / back-off query goes to the coarse evaluator when the step that led to it is > tier_gate
    float lip;               // staged min-SDF search: Lipschitz bound of the SDF along a ray (0: off)
    int share;               //              ... its first stage is shared among the rays of a wave (minsdf_share; NEFII_MINSDF_SHARE)
    int stage_bracket;       //              ... and the bracket search of eval-mode traces / rays outside the mask staged too
    int miss_argmin;         // eval-mode bracket search: the argmin fallback of rays WITHOUT a negative sample is computed (1; 0: nobody reads it)
    // SDF interval grid (nefii_sdf_bound_grid_build; null: none): grid_n^3 cells over the cube [-radius, radius]^3 of the bounding
    // sphere, one word per cell - fp16 lo in the low half, fp16 hi in the high half, lo <= sdf <= hi throughout the cell
    const unsigned *cells;
    int grid_n;
    float grid_inv_h;        // cells per unit length
    // ... and the values it was built from (nefii_sdf_bound_grid_build_vertices; both null: cell intervals only): fp16 single-pass
    // values at the (grid_n + 1)^3 vertices and the fp16 slope bound of every cell - a sample the cell's interval leaves
    // undecided is bounded from the 8 corners of its cell (grid_corner_bounds)
    const unsigned short *vert_g, *cell_l;
    float grid_h;            // cell edge, as the build rounds it
    int grid_training;       // training-mode traces read the grid too: the bracket searches of their rays inside the object mask
    int walk_wave;           // the walks over the grid are run by the whole wave, one ray at a time (serve_grid_walks; NEFII_GRID_WALK_WAVE)
    // the block level over the cells (nefii_sdf_bound_grid_blocks; null: none): block_n^3 fp16 minima of lo, and whether round 0
    // ends the training-mode rays it proves to cross (certify_crossing; nefii_trace_grid.certify)
    const unsigned short *blocks;
    int block_n;
    int certify;
    int certify_free;        // eval-mode traces with unread misses end the rays whose remaining stretch the grid proves free (certify_free_stretch)
    int *cert_counts;        // [NEFII_CERTIFY_COUNTS], added to (null: not counted)
    RayState s;
};

// first stage of the staged min-SDF search: sorted position of its j-th depth, j < stage1_count (both ends included)
__host__ __device__ __forceinline__ int stage1_count(int ns) { return coarse_window(ns); }
__host__ __device__ __forceinline__ int stage1_pos(int ns, int j) { return (j * (ns - 1)) / (stage1_count(ns) - 1); }
// the staged bracket search takes the rays whose quarter-row windows are long searches: eval-mode traces (the secondary rays
// of the MC renderer, full-frame renders - most of their searches find their crossing late or not at all) and rays outside
// the object mask (whole rows, argmin); training-mode rays inside the mask stop in their first window and keep the windows -
// unless the trace reads the SDF interval grid (begin_coarse_bracket: P.grid_training), which serves them better than either
__device__ __forceinline__ bool staged_bracket(const Params &P, int64_t r) {
    return P.lip > 0.f && P.stage_bracket && (!P.p.training || P.obj[r] == 0);
}
__device__ __forceinline__ int minsdf_row(const Params &P, int64_t r) {
    const int g = P.p.minsdf_group;
    return g > 0 ? (int)(r / g) : 0;
}

// uniform draw i of ray r's min-SDF search: one row for the whole call, or one row per minsdf_group consecutive rays
// (several batches traced as one call keep their own draws)
__device__ __forceinline__ float minsdf_step(const Params &P, int64_t r, int i) {
    const int g = P.p.minsdf_group;
    return P.steps[(g > 0 ? (r / g) * (int64_t)P.p.n_steps : 0) + i];
}

// ---- work-list append: block-aggregated ------------------------------------------------------
// What one ray asks for this round: up to 2 single queries, one dense ray (split precision or coarse), one bisecting ray
// and n_ref single samples (bit set `cmask`).  Zero-initialised: a ray that asks for nothing; filled by the phase functions.
struct Emit {
    bool qs, qe;               // the ray's start / end sphere-tracing query ...
    bool cs, ce;               // ... goes to the COARSE evaluator (tiered sphere tracing)
    bool qt, qd;               // the ray bisects / all n_steps samples in split precision
    int nc, cwin;              // quarter rows cwin .. cwin + nc - 1 of the ray's samples for the coarse evaluator (4 from 0: the whole row)
    unsigned dense_which;      // 0 sampler, 1 min-sdf
    int consumed;              // bisection evaluations actually used this round (of the 7 speculated per ray)
    int n_alg;                 // dense searches entered this round (the reference evaluates n_steps samples for each)
    int n_ref;                 // samples of this ray to (re-)evaluate one by one (bits of cmask): in split precision, or
    unsigned cmask[4];
    int n_rep;                 // split-precision singles of this ray that repeat a coarse one
    bool ref_coarse;           // ... (staged searches) the n_ref samples go to the COARSE evaluator's list (crefine)
    int walk, walk_from;       // a walk over the SDF interval grid that the ray asks its wave for (serve_grid_walks): WALK_*, and
                               // begin_grid_bracket's `from`
    // (the words are picked by comparison, never by a run-time index: the whole struct then lives in registers)
    __device__ __forceinline__ void mark(int i) {
#pragma unroll
        for (int w = 0; w < 4; ++w) cmask[w] |= (i >> 5) == w ? 1u << (i & 31) : 0u;
    }
    __device__ __forceinline__ bool marked(int i) const {
        unsigned word = 0u;
#pragma unroll
        for (int w = 0; w < 4; ++w) word = (i >> 5) == w ? cmask[w] : word;
        return (word >> (i & 31)) & 1u;
    }
    __device__ __forceinline__ void clear_marks() { cmask[0] = cmask[1] = cmask[2] = cmask[3] = 0u; }
};
// block totals, and the work lists whose offsets they become
enum Total : int { T_SINGLES, T_DENSE, T_TRI, T_CONSUMED, T_REFINE, T_CWINDOWS, T_ALG, T_CSINGLES, T_REP, T_CREFINE, N_TOTALS };
enum List : int { L_SINGLES, L_DENSE, L_TRI, L_REFINE, L_CDENSE, L_CSINGLES, L_CREFINE, N_LISTS };

__device__ __forceinline__ void append_queries(const Params &P, int round, unsigned ray, const Emit &e) {
    __shared__ int wtot[N_TOTALS][4];
    __shared__ int base[N_LISTS];
    const bool qs = e.qs && !e.cs, qe = e.qe && !e.ce, qcs = e.qs && e.cs, qce = e.qe && e.ce;
    const int nc = e.nc, n_ref = e.n_ref;
    const bool ref_coarse = e.ref_coarse;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bs = __ballot(qs), be = __ballot(qe), bt = __ballot(e.qt), bd = __ballot(e.qd);
    const unsigned long long bcs = __ballot(qcs), bce = __ballot(qce);
    const unsigned long long lt = (1ull << lane) - 1ull;
    int cons = e.consumed, alg = e.n_alg, rep = e.n_rep;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cons += __shfl_xor(cons, o), alg += __shfl_xor(alg, o), rep += __shfl_xor(rep, o);
    int incl = ref_coarse ? 0 : n_ref;      // inclusive prefix sums of the two refine counts over the wave
    int incl2 = ref_coarse ? n_ref : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o), t2 = __shfl_up(incl2, o);
        if (lane >= o) incl += t, incl2 += t2;
    }
    const int wref = __shfl(incl, 63), wref2 = __shfl(incl2, 63);
    int cincl = nc;                 // ... and of the coarse window counts
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(cincl, o);
        if (lane >= o) cincl += t;
    }
    const int wcoarse = __shfl(cincl, 63);
    if (lane == 0) {
        wtot[T_SINGLES][wave] = __popcll(bs) + __popcll(be);
        wtot[T_DENSE][wave] = __popcll(bd);
        wtot[T_TRI][wave] = __popcll(bt);
        wtot[T_CONSUMED][wave] = cons;
        wtot[T_REFINE][wave] = wref;
        wtot[T_CWINDOWS][wave] = wcoarse;
        wtot[T_ALG][wave] = alg;
        wtot[T_CSINGLES][wave] = __popcll(bcs) + __popcll(bce);
        wtot[T_REP][wave] = rep;
        wtot[T_CREFINE][wave] = wref2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int t[N_TOTALS];
        for (int i = 0; i < N_TOTALS; ++i) t[i] = wtot[i][0] + wtot[i][1] + wtot[i][2] + wtot[i][3];
        int *cnt = P.counters + round * NCNT;
        // a list's counter is its length: the block's entries start at the value before the add
        base[L_SINGLES] = t[T_SINGLES] ? atomicAdd(&cnt[NEFII_CNT_SINGLES], t[T_SINGLES]) : 0;
        base[L_DENSE] = t[T_DENSE] ? atomicAdd(&cnt[NEFII_CNT_DENSE_ROWS], t[T_DENSE]) : 0;
        base[L_TRI] = t[T_TRI] ? atomicAdd(&cnt[NEFII_CNT_BISECT_RAYS], t[T_TRI]) : 0;
        if (t[T_CONSUMED]) atomicAdd(&cnt[NEFII_CNT_BISECT_USED], t[T_CONSUMED]);
        base[L_REFINE] = t[T_REFINE] ? atomicAdd(&cnt[NEFII_CNT_REFINED], t[T_REFINE]) : 0;
        base[L_CDENSE] = t[T_CWINDOWS] ? atomicAdd(&cnt[NEFII_CNT_COARSE_WINDOWS], t[T_CWINDOWS]) : 0;
        if (t[T_ALG]) atomicAdd(&cnt[NEFII_CNT_SEARCHES], t[T_ALG]);
        if (t[T_TRI]) atomicAdd(&cnt[NEFII_CNT_BISECT_EVALS], t[T_TRI] * P.tri_nodes);      // speculative bisection evaluations executed
        base[L_CSINGLES] = t[T_CSINGLES] ? atomicAdd(&cnt[NEFII_CNT_COARSE_SINGLES], t[T_CSINGLES]) : 0;
        if (t[T_REP]) atomicAdd(&cnt[NEFII_CNT_REPEATS], t[T_REP]);
        base[L_CREFINE] = t[T_CREFINE] ? atomicAdd(&cnt[NEFII_CNT_COARSE_SAMPLES], t[T_CREFINE]) : 0;
    }
    __syncthreads();
    int off_s = base[L_SINGLES], off_d = base[L_DENSE], off_t = base[L_TRI], off_r = base[L_REFINE], off_c = base[L_CDENSE],
        off_cs = base[L_CSINGLES], off_r2 = base[L_CREFINE];
    for (int w = 0; w < wave; ++w) {
        off_r2 += wtot[T_CREFINE][w];
        off_s += wtot[T_SINGLES][w];
        off_d += wtot[T_DENSE][w];
        off_t += wtot[T_TRI][w];
        off_r += wtot[T_REFINE][w];
        off_c += wtot[T_CWINDOWS][w];
        off_cs += wtot[T_CSINGLES][w];
    }
    if (qs) P.s.singles[off_s + __popcll(bs & lt)] = (ray << 2) | Q_START;
    if (qe) P.s.singles[off_s + __popcll(bs) + __popcll(be & lt)] = (ray << 2) | Q_END;
    if (qcs) P.s.csingles[off_cs + __popcll(bcs & lt)] = (ray << 2) | Q_START;
    if (qce) P.s.csingles[off_cs + __popcll(bcs) + __popcll(bce & lt)] = (ray << 2) | Q_END;
    if (e.qd) P.s.dense[off_d + __popcll(bd & lt)] = (ray << 1) | e.dense_which;
    if (e.qt) P.s.tri[off_t + __popcll(bt & lt)] = ray;
    for (int k = 0; k < nc; ++k)
        P.s.cdense[off_c + cincl - nc + k] = ((unsigned)(e.cwin + k) << 29) | (ray << 1) | e.dense_which;
    if (n_ref > 0) {
        size_t o = ref_coarse ? (size_t)off_r2 + incl2 - n_ref : (size_t)off_r + incl - n_ref;
        unsigned *list = ref_coarse ? P.s.crefine : P.s.refine;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned mbits = e.cmask[w];
            while (mbits) {
                const int bit = __ffs(mbits) - 1;
                mbits &= mbits - 1;
                list[o++] = (ray << 7) | (unsigned)(32 * w + bit);
            }
        }
    }
    __syncthreads();
}

// depth of heap node j (root 0, children 2j+1 / 2j+2) of the speculative bisection tree over [lo, hi]: replay the
// recurrence mid = (lo + hi) / 2 (ray_tracing.py:262,275) along the node's path - the speculated points ARE the
// points sequential bisection would visit.  Path bits, MSB first after the leading 1 of (j+1): 1 = "f(mid) > 0"
// (lo = mid), 0 = hi = mid.
__device__ __forceinline__ float tri_depth(float lo, float hi, int j) {
    const unsigned k = (unsigned)j + 1u;
    const int level = 31 - __clz(k);
    float mid = fmul(fadd(lo, hi), 0.5f);
    for (int b = level - 1; b >= 0; --b) {
        if ((k >> b) & 1u) lo = mid; else hi = mid;
        mid = fmul(fadd(lo, hi), 0.5f);
    }
    return mid;
}

__device__ __forceinline__ void finish(const Params &P, int64_t r, float dist, bool hit) {
    const float ox = P.o[r * 3], oy = P.o[r * 3 + 1], oz = P.o[r * 3 + 2];
    const float dx = P.d[r * 3], dy = P.d[r * 3 + 1], dz = P.d[r * 3 + 2];
    P.out_dist[r] = dist;
    P.out_hit[r] = hit ? 1 : 0;
    P.out_pts[r * 3] = fadd(ox, fmul(dist, dx));
    P.out_pts[r * 3 + 1] = fadd(oy, fmul(dist, dy));
    P.out_pts[r * 3 + 2] = fadd(oz, fmul(dist, dz));
}

// staged min-SDF search: sorted order of every row of draws (rank by value, ties by index), once per call
__global__ __launch_bounds__(128) void minsdf_order_kernel(Params P) {
    const int ns = P.p.n_steps, i = threadIdx.x;
    if (i >= ns) return;
    const float *st = P.steps + (size_t)blockIdx.x * ns;
    const float si = st[i];
    int rank = 0;
    for (int j = 0; j < ns; ++j) {
        const float sj = st[j];
        rank += (sj < si || (sj == si && j < i)) ? 1 : 0;
    }
    P.s.ord[(size_t)blockIdx.x * ns + rank] = (unsigned char)i;
}

// ---- the per-ray state machine ---------------------------------------------------------------
// One function per phase.  Each consumes what its ray asked for last round, fills `e` with what the ray asks for this
// round and returns the phase to go on with IN THIS ROUND: PH_WAIT once the ray's flags are stored and it waits for an
// evaluation (or is done), any other phase to fall through to that phase's function further down advance_kernel's chain.

// ---- crossing certificate from the block level of the SDF interval grid ------------------------
// One step of the bounds a <= t_s, b >= t_e on the two fronts of the ray o + t d: a walk over EVERY block the chord [a, b]
// crosses, from block to block through the faces the chord leaves by (at a face crossing shared by two axes the walk takes
// them one after the other - the block it leaves out touches the chord in a point of the closed blocks on either side, whose
// bounds hold there too).  A front that stands in block j, which the chord is in from depth in_j to out_j, finds an SDF value
// of at least s_j = lo_j - off there and moves by that: the start front to at least max(a, in_j) + s_j, the end front to at
// most min(b, out_j) - s_j, whichever block it stands in -
//   na = min_j (max(a, in_j) + s_j),      nb = max_j (min(b, out_j) - s_j).
// False as soon as a block has lo <= stop (a NaN too), and where the chord leaves the cube or the block array: no bound.
// looks: block look-ups made.
__device__ __forceinline__ bool chord_block_step(const Params &P, float ox, float oy, float oz, float dx, float dy, float dz,
                                                 float a, float b, float off, float stop, float &na, float &nb, int &looks) {
    const float inf = __builtin_inff();
    const float rad = P.p.object_bounding_sphere;
    const float inv_hb = P.grid_inv_h * (1.f / NEFII_BOUND_GRID_BLOCK), hb = P.grid_h * NEFII_BOUND_GRID_BLOCK;
    const float ext = (float)P.grid_n * (1.f / NEFII_BOUND_GRID_BLOCK);      // the cube's edge in blocks (the last one may be short)
    const int gb = P.block_n;
    const float fx = fmul(fadd(fadd(ox, fmul(a, dx)), rad), inv_hb);
    const float fy = fmul(fadd(fadd(oy, fmul(a, dy)), rad), inv_hb);
    const float fz = fmul(fadd(fadd(oz, fmul(a, dz)), rad), inv_hb);
    if (!(fx >= 0.f && fx < ext && fy >= 0.f && fy < ext && fz >= 0.f && fz < ext)) return false;      // (NaN: outside)
    int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    // depth behind a at which the chord leaves the current block along each axis, and what one block more adds to it
    const float sx = dx != 0.f ? hb / fabsf(dx) : inf, sy = dy != 0.f ? hb / fabsf(dy) : inf, sz = dz != 0.f ? hb / fabsf(dz) : inf;
    float tx = dx > 0.f ? ((float)(ix + 1) - fx) * sx : dx < 0.f ? (fx - (float)ix) * sx : inf;
    float ty = dy > 0.f ? ((float)(iy + 1) - fy) * sy : dy < 0.f ? (fy - (float)iy) * sy : inf;
    float tz = dz > 0.f ? ((float)(iz + 1) - fz) * sz : dz < 0.f ? (fz - (float)iz) * sz : inf;
    const int ux = dx > 0.f ? 1 : -1, uy = dy > 0.f ? 1 : -1, uz = dz > 0.f ? 1 : -1;
    const float len = fsub(b, a);
    float in = 0.f;       // where the chord enters the current block, behind a
    na = inf, nb = -inf;
    for (int n = 0; n < 3 * NEFII_BOUND_GRID_MAX; ++n) {      // (a walk enters at most 3 gb blocks; the bound is for the reader)
        const float lo = (float)__builtin_bit_cast(_Float16, P.blocks[((size_t)ix * gb + (size_t)iy) * gb + (size_t)iz]);
        ++looks;
        if (!(lo > stop)) return false;
        const float s = fsub(lo, off);
        const float tn = fminf(tx, fminf(ty, tz));
        na = fminf(na, fadd(fadd(a, in), s));
        nb = fmaxf(nb, fsub(fadd(a, fminf(tn, len)), s));
        if (!(tn < len)) return true;
        in = tn;
        if (tx == tn) ix += ux, tx += sx;
        else if (ty == tn) iy += uy, ty += sy;
        else iz += uz, tz += sz;
        if ((unsigned)ix >= (unsigned)gb || (unsigned)iy >= (unsigned)gb || (unsigned)iz >= (unsigned)gb) return false;
    }
    return false;
}

// Do the two fronts of a training-mode ray surely cross within sphere_tracing_iters?  Bounds a_k <= t_s, b_k >= t_e of the fronts
// after k steps, from a_0 = t0, b_0 = t1.  Every SDF value the tracing can meet in a block - exact, or the single-pass
// evaluator's, within tau of it - is at least lo - off, off = tau + margin.  While that exceeds sdf_threshold in every block of
// the chord [a_k, b_k] no front arrives, none backs off (no value is negative), and each moves at least as chord_block_step
// says - at least by m_k - off, m_k the least lo of the chord: the rule a_k+1 = a_k + m_k, b_k+1 = b_k - m_k with each block's
// own lo counted from where the chord enters it, so that a block near the surface in the middle of the ray does not hold back
// fronts that are still far from it.  The true fronts have crossed once the bounds have.  The margin covers the rounding of the
// walk's depths and points (1e-6 of a coordinate) at any slope a network has.
__device__ __forceinline__ bool certify_crossing(const Params &P, float ox, float oy, float oz, float dx, float dy, float dz,
                                                 float t0, float t1, int &looks) {
    const float off = fadd(P.tau, NEFII_CERTIFY_MARGIN), stop = fadd(P.p.sdf_threshold, off);
    float a = t0, b = t1;
    for (int k = 0; k <= P.p.sphere_tracing_iters; ++k) {
        if (a >= b) return true;
        if (k == P.p.sphere_tracing_iters) break;
        float na, nb;
        if (!chord_block_step(P, ox, oy, oz, dx, dy, dz, a, b, off, stop, na, nb, looks)) break;
        a = na;
        b = nb;
    }
    return false;
}

__device__ __forceinline__ bool grid_bounds(const Params &P, int64_t r, float t, float &lo, float &hi);

// ---- free-stretch certificate of eval-mode rays whose misses nobody reads ----------------------
// Is every point of the chord [a, b] of the ray o + t d in a cell with lo > stop?  One walk of chord_block_step's kind over
// boxes of `edge` cells a side: the blocks (edge = NEFII_BOUND_GRID_BLOCK, from P.blocks) or the cells themselves (edge = 1,
// the lo half of P.cells).  A block that is not free is walked again by its cells, over the depths the chord is in it (the
// few cells of its neighbours that the rounding of those depths may add can only fail the test).  False where the chord
// leaves the cube.  looks: look-ups made.
template <int EDGE>
__device__ __forceinline__ bool chord_free(const Params &P, float ox, float oy, float oz, float dx, float dy, float dz, float a,
                                           float b, float stop, int &looks);
template <int EDGE>
__device__ __forceinline__ bool box_free(const Params &P, float ox, float oy, float oz, float dx, float dy, float dz, int ix,
                                         int iy, int iz, float a, float b, float stop, int &looks) {
    if constexpr (EDGE == 1) {
        const unsigned w = P.cells[((size_t)ix * P.grid_n + (size_t)iy) * P.grid_n + (size_t)iz];
        return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu)) > stop;
    } else {
        const float lo = (float)__builtin_bit_cast(_Float16, P.blocks[((size_t)ix * P.block_n + (size_t)iy) * P.block_n + (size_t)iz]);
        if (lo > stop) return true;
        return chord_free<1>(P, ox, oy, oz, dx, dy, dz, a, b, stop, looks);
    }
}
template <int EDGE>
__device__ __forceinline__ bool chord_free(const Params &P, float ox, float oy, float oz, float dx, float dy, float dz, float a,
                                           float b, float stop, int &looks) {
    const float inf = __builtin_inff();
    const float rad = P.p.object_bounding_sphere;
    const float inv_h = P.grid_inv_h * (1.f / EDGE), h = P.grid_h * EDGE;
    const float ext = (float)P.grid_n * (1.f / EDGE);
    const int g = EDGE == 1 ? P.grid_n : P.block_n;
    const float fx = fmul(fadd(fadd(ox, fmul(a, dx)), rad), inv_h);
    const float fy = fmul(fadd(fadd(oy, fmul(a, dy)), rad), inv_h);
    const float fz = fmul(fadd(fadd(oz, fmul(a, dz)), rad), inv_h);
    if (!(fx >= 0.f && fx < ext && fy >= 0.f && fy < ext && fz >= 0.f && fz < ext)) return false;      // (NaN: outside)
    int ix = (int)fx, iy = (int)fy, iz = (int)fz;
    const float sx = dx != 0.f ? h / fabsf(dx) : inf, sy = dy != 0.f ? h / fabsf(dy) : inf, sz = dz != 0.f ? h / fabsf(dz) : inf;
    float tx = dx > 0.f ? ((float)(ix + 1) - fx) * sx : dx < 0.f ? (fx - (float)ix) * sx : inf;
    float ty = dy > 0.f ? ((float)(iy + 1) - fy) * sy : dy < 0.f ? (fy - (float)iy) * sy : inf;
    float tz = dz > 0.f ? ((float)(iz + 1) - fz) * sz : dz < 0.f ? (fz - (float)iz) * sz : inf;
    const int ux = dx > 0.f ? 1 : -1, uy = dy > 0.f ? 1 : -1, uz = dz > 0.f ? 1 : -1;
    const float len = fsub(b, a);
    float in = 0.f;
    for (int n = 0; n < 3 * NEFII_BOUND_GRID_MAX; ++n) {
        const float tn = fminf(tx, fminf(ty, tz));
        ++looks;
        if (!box_free<EDGE>(P, ox, oy, oz, dx, dy, dz, ix, iy, iz, fadd(a, in), fadd(a, fminf(tn, len)), stop, looks)) return false;
        if (!(tn < len)) return true;
        in = tn;
        if (tx == tn) ix += ux, tx += sx;
        else if (ty == tn) iy += uy, ty += sy;
        else iz += uz, tz += sz;
        if ((unsigned)ix >= (unsigned)g || (unsigned)iy >= (unsigned)g || (unsigned)iz >= (unsigned)g) return false;
    }
    return false;
}

// An eval-mode ray whose misses nobody reads (unread_misses) and whose start front stands at t_s: with every cell of the
// stretch [t_s, t_max] - up to where the ray leaves the bounding sphere - at lo > sdf_threshold + tau + margin, the ray ends
// as a miss.  Every position the start front can take while t_s < t_e lies on that stretch (the end front never moves behind
// t_max, a back-off never in front of the depth it started from) and every value it can meet there - exact or single-pass -
// exceeds the threshold: it never arrives.  If the fronts cross the ray has no hit; if the iterations run out, the bracket
// search's samples lie between the fronts, none is negative, and the argmin is not read.  What the end front meets - even
// behind the stretch, where a step may overshoot - moves t_e only.  One look-up first: most attempts fail at t_s's own cell.
__device__ __forceinline__ bool certify_free_stretch(const Params &P, int64_t r, float t_s, int &looks) {
    const float stop = fadd(P.p.sdf_threshold, fadd(P.tau, NEFII_CERTIFY_MARGIN));
    float lo, hi;
    ++looks;
    if (!grid_bounds(P, r, t_s, lo, hi) || !(lo > stop)) return false;
    const float t_max = P.s.t_max[r];
    if (!(t_s < t_max)) return false;
    return chord_free<NEFII_BOUND_GRID_BLOCK>(P, P.o[r * 3], P.o[r * 3 + 1], P.o[r * 3 + 2], P.d[r * 3], P.d[r * 3 + 1],
                                              P.d[r * 3 + 2], t_s, t_max, stop, looks);
}

// ... ends: outputs finite, no hit.  One certified ray in 16, picked by a hash, first sends one hash-picked depth of its stretch to
// the single-pass evaluator as a probe (F_PROBE: the start front's query, t_s parked in `mid`); step_trace holds the value
// against its cell next round and ends the ray then
constexpr int F_PROBE = 1 << 11;      // (F_OWN's bit: the min-SDF search's, which an eval-mode ray never enters)
__device__ __forceinline__ int end_free(const Params &P, int64_t r, int round, int &fl, Emit &e, float t_s) {
    const unsigned h0 = ((unsigned)r * 2654435761u) ^ 0x9E3779B1u, h = (h0 ^ (h0 >> 15)) * 0x85EBCA6Bu;
    if ((h >> 28) == 0u) {
        const float u = (float)((h >> 4) & 0xFFFFu) * (1.f / 65536.f);
        P.s.mid[r] = t_s;
        P.s.t_s[r] = fadd(t_s, fmul(u, fsub(P.s.t_max[r], t_s)));
        e.qs = e.cs = true;
        atomicAdd(P.counters + round * NCNT + NEFII_CNT_PROBES, 1);
        fl = PH_TRACE | F_SPH | F_PROBE;
        P.s.flags[r] = fl;
        return PH_WAIT;
    }
    finish(P, r, t_s, false);
    fl = F_SPH | F_CERT | PH_DONE;
    P.s.flags[r] = fl;
    return PH_WAIT;
}

// round 0: bounding-sphere intersection (rend_util.py:200-221) and state initialisation (:107-134)
__device__ __forceinline__ int init_ray(const Params &P, int64_t r, int round, int &fl, Emit &e, int &looks) {
    const bool tier = P.tier_band > 0.f;
    const float ox = P.o[r * 3], oy = P.o[r * 3 + 1], oz = P.o[r * 3 + 2];
    const float dx = P.d[r * 3], dy = P.d[r * 3 + 1], dz = P.d[r * 3 + 2];
    const float b = fadd(fadd(fmul(dx, ox), fmul(dy, oy)), fmul(dz, oz));
    const float nrm = sqrtf(fadd(fadd(fmul(ox, ox), fmul(oy, oy)), fmul(oz, oz)));
    const float rad = P.p.object_bounding_sphere;
    const float under = fsub(fmul(b, b), fsub(fmul(nrm, nrm), fmul(rad, rad)));
    const bool sph = under > 0.f;
    float t0 = 0.f, t1 = 0.f;
    if (sph) {
        const float sq = sqrtf(under);
        t0 = fmaxf(fsub(-sq, b), 0.01f);
        t1 = fmaxf(fsub(sq, b), 0.01f);
    }
    P.s.t_s[r] = t0;
    P.s.t_e[r] = t1;
    P.s.t_min[r] = t0;
    P.s.t_max[r] = t1;
    P.s.nxt_s[r] = 0.f;
    P.s.nxt_e[r] = 0.f;
    P.s.cur_s[r] = 0.f;
    P.s.cur_e[r] = 0.f;
    fl = PH_TRACE;
    if (!sph) return PH_TRACE;      // nothing to evaluate: the tracing stage ends this ray's trace right away
    if (P.certify && certify_crossing(P, ox, oy, oz, dx, dy, dz, t0, t1, looks)) {
        // the fronts would cross: no hit, nothing for the bracket search - the state end_trace leaves such a ray in (post()
        // sends it to the min-SDF search, which reads t_min and t_max and overwrites the depth)
        fl = F_SPH | F_CERT;
        P.s.mid[r] = t0;
        return PH_POST;
    }
    if (P.certify_free && certify_free_stretch(P, r, t0, looks)) return end_free(P, r, round, fl, e, t0);
    fl |= F_SPH | F_LIVE_S | F_LIVE_E | F_PEND_S | F_PEND_E;
    e.qs = e.qe = true;
    // tiered sphere tracing: the first evaluations lie on the bounding sphere, far from the surface - unless the
    // ray starts inside it (secondary rays: t0 clamped to 0.01 off the surface they leave)
    e.cs = tier && t0 > 0.01f;
    e.ce = tier && t1 > 0.01f;
    fl |= (e.cs ? F_CRS_S : 0) | (e.ce ? F_CRS_E : 0);
    P.s.flags[r] = fl;
    return PH_WAIT;     // wait for the first evaluation
}

// first stage of a staged search: whatever no evaluator writes of samples `from`.. stays +inf (positive, neither a minimum
// nor within any band of one); a quarter row's worth of the samples, spread over the row, goes to the coarse evaluator
__device__ __forceinline__ void begin_stage1(const Params &P, int64_t r, int from, int stage_code, int &fl, Emit &e) {
    float *v = P.s.big + (size_t)r * P.p.n_steps;
    for (int i = from; i < P.p.n_steps; ++i) v[i] = __builtin_inff();
    e.nc = 1;
    e.cwin = CWIN_STAGE1;
    fl = with_win(fl, stage_code);
}

// ---- staged bracket search from the SDF interval grid -----------------------------------------
// Under frozen geometry the network's values are bounded cell by cell once (nefii_sdf_bound_grid_build): lo <= sdf <= hi over
// a cell, from the single-pass values at its corners, their error bound and a slope bound measured around the cell.  A
// bracket search of an eval-mode trace - or, where asked for, of a training-mode ray inside the object mask - then needs no
// evaluated first stage: one look-up per sample bounds it.
// The bounds of the point of ray r at depth t; false (and -inf / +inf) outside the cube: no bound, the sample is evaluated.
__device__ __forceinline__ bool grid_bounds(const Params &P, int64_t r, float t, float &lo, float &hi) {
    const float rad = P.p.object_bounding_sphere, g = (float)P.grid_n;
    const float ox = P.o[r * 3], oy = P.o[r * 3 + 1], oz = P.o[r * 3 + 2];
    const float dx = P.d[r * 3], dy = P.d[r * 3 + 1], dz = P.d[r * 3 + 2];
    const float fx = fmul(fadd(fadd(ox, fmul(t, dx)), rad), P.grid_inv_h);
    const float fy = fmul(fadd(fadd(oy, fmul(t, dy)), rad), P.grid_inv_h);
    const float fz = fmul(fadd(fadd(oz, fmul(t, dz)), rad), P.grid_inv_h);
    lo = -__builtin_inff(), hi = __builtin_inff();
    if (!(fx >= 0.f && fx < g && fy >= 0.f && fy < g && fz >= 0.f && fz < g)) return false;      // (NaN: outside)
    const unsigned w = P.cells[((size_t)(int)fx * P.grid_n + (size_t)(int)fy) * P.grid_n + (size_t)(int)fz];
    lo = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu));
    hi = (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
    return true;
}

// The same point bounded from the 8 corners of its cell (P.vert_g, P.cell_l: nefii_sdf_bound_grid_build_vertices): with the fp16
// corner values g_c, the cell's slope bound L and the distances d_c = |p - x_c| + 1e-6 (the 1e-6 covers the rounding of p and x_c),
//   lo = max_c (g_c - e_c - L d_c) - tau,   hi = min_c (g_c + e_c + L d_c) + tau,   e_c = 2^-11 |g_c| + 2^-25
// (e_c: what rounding g_c to the nearest fp16 can have moved it by).  The same measured quantities and the same slope claim
// as the cell's interval, without its spread over the corners and with the true reach instead of the largest.  False outside
// the cube.  The two corners along z of each of the four (x, y) pairs are neighbours in memory.
__device__ __forceinline__ bool grid_corner_bounds(const Params &P, int64_t r, float t, float &lo, float &hi) {
    const float rad = P.p.object_bounding_sphere, g = (float)P.grid_n;
    const float ox = P.o[r * 3], oy = P.o[r * 3 + 1], oz = P.o[r * 3 + 2];
    const float dx = P.d[r * 3], dy = P.d[r * 3 + 1], dz = P.d[r * 3 + 2];
    const float px = fadd(ox, fmul(t, dx)), py = fadd(oy, fmul(t, dy)), pz = fadd(oz, fmul(t, dz));
    const float fx = fmul(fadd(px, rad), P.grid_inv_h), fy = fmul(fadd(py, rad), P.grid_inv_h), fz = fmul(fadd(pz, rad), P.grid_inv_h);
    lo = -__builtin_inff(), hi = __builtin_inff();
    if (!(fx >= 0.f && fx < g && fy >= 0.f && fy < g && fz >= 0.f && fz < g)) return false;
    const int ci = (int)fx, cj = (int)fy, ck = (int)fz;
    const size_t V = (size_t)P.grid_n + 1;
    const float L = (float)__builtin_bit_cast(_Float16, P.cell_l[((size_t)ci * P.grid_n + (size_t)cj) * P.grid_n + (size_t)ck]);
    unsigned short gc[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned short *row = P.vert_g + ((size_t)(ci + (c >> 1)) * V + (size_t)(cj + (c & 1))) * V + (size_t)ck;
        gc[2 * c] = row[0];
        gc[2 * c + 1] = row[1];
    }
    float ex2[2], ey2[2], ez2[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const float ex = fsub(px, fadd(-rad, fmul((float)(ci + a), P.grid_h)));
        const float ey = fsub(py, fadd(-rad, fmul((float)(cj + a), P.grid_h)));
        const float ez = fsub(pz, fadd(-rad, fmul((float)(ck + a), P.grid_h)));
        ex2[a] = fmul(ex, ex), ey2[a] = fmul(ey, ey), ez2[a] = fmul(ez, ez);
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float v = (float)__builtin_bit_cast(_Float16, gc[c]);
        const float dist = fadd(sqrtf(fadd(fadd(ex2[c >> 2], ey2[(c >> 1) & 1]), ez2[c & 1])), 1e-6f);
        const float reach = fadd(fmul(L, dist), fadd(fmul(fabsf(v), 0x1p-11f), 0x1p-25f));
        lo = fmaxf(lo, fsub(v, reach));
        hi = fminf(hi, fadd(v, reach));
    }
    lo = fsub(lo, P.tau);
    hi = fadd(hi, P.tau);
    return true;
}

// A bracket search starts from the grid (fl: PH_SAMPLER_C; samples in front of `from` hold exact values: bounds of
// themselves).  What the search decides is sampler_staged's: the FIRST negative sample, the sign of its bracket partner and
// - unless the ray lies inside the object mask and surely has a negative sample - the argmin.
//   j1, the first sample with hi < -tau, is surely negative.  With j1 on a ray inside the mask whose sample 0 is surely
//     positive (lo_0 > 0; sample 0 would pair with the LAST sample) only the samples up to j1 matter, and only their sign;
//   a sample is skipped for good when lo > lim: 0 where only signs matter (also when nobody reads the argmin), else
//     max(0, min_i hi_i + tau) - positive, and above the exact minimum: not the argmin;
//   the others go to the coarse evaluator one by one (crefine), with staged_walk's probes: up to NEAR_PROBES skipped samples
//     whose bound clears lim by less than 2 tau and one picked by a hash;
//   more than CREF_CAP of them: the whole row, as without the staging.
// With the vertex values at hand (P.vert_g) the walk has two levels: the cell intervals first, one look-up per sample, then
// the corner bounds of the samples they leave - combined as max of the lower, min of the upper ends - and j1, U, lim and last
// once more from those (tests/test_bound_vertices_cpu.py restates the rule).
// Skipped samples stay at +inf.  Next round (SW_GRID) grid_audit holds every evaluated sample against the interval relied on.
__device__ __forceinline__ void begin_grid_bracket(const Params &P, int64_t r, int round, int from, int &fl, Emit &e) {
    const int ns = P.p.n_steps;
    float *v = P.s.big + (size_t)r * ns;
    const float a = P.s.t_s[r], rng = fsub(P.s.t_e[r], a);
    const bool obj = P.obj[r] != 0;
    // first pass: the lower bounds are parked in the row itself (the upper ones only feed j1 and U)
    int j1 = ns;
    float U = __builtin_inff(), lo0 = 0.f;
    for (int i = 0; i < ns; ++i) {
        float lo, hi;
        if (i < from)
            lo = hi = v[i];
        else
            grid_bounds(P, r, fadd(a, fmul(P.lin[i], rng)), lo, hi);
        if (hi < -P.tau && j1 == ns) j1 = i;
        U = fminf(U, hi);
        if (i == 0) lo0 = lo;
        if (i >= from) v[i] = lo;
    }
    bool front_only = obj && j1 < ns && lo0 > 0.f;
    bool sign_only = front_only || !P.miss_argmin;
    float lim = sign_only ? 0.f : fmaxf(0.f, fadd(U, P.tau));
    int last = front_only ? j1 : ns - 1;
    if (P.vert_g) {
        // second pass: the samples the cell intervals leave to be evaluated (the others can neither become j1 nor lower U:
        // their lo is positive and above U) are bounded from their cell's corners; lo only rises, hi only falls, so j1 moves
        // forward, U, lim and last fall and the survivors below are a subset of the cell intervals' own
        for (int i = from; i <= last; ++i) {
            const float lb = v[i];
            if (fsub(lb, 1e-6f) > lim) continue;
            float lo, hi;
            if (!grid_corner_bounds(P, r, fadd(a, fmul(P.lin[i], rng)), lo, hi)) continue;
            v[i] = fmaxf(lb, lo);
            if (i == 0) lo0 = v[i];
            U = fminf(U, hi);
            if (hi < -P.tau && i < j1) {
                j1 = i;
                if (obj && lo0 > 0.f) break;      // front_only: nothing behind j1 matters
            }
        }
        front_only = obj && j1 < ns && lo0 > 0.f;
        sign_only = front_only || !P.miss_argmin;
        lim = sign_only ? 0.f : fmaxf(0.f, fadd(U, P.tau));
        last = front_only ? j1 : ns - 1;
    }
    int k = 0, n_near = 0, probe = -1;
    unsigned probe_h = ~0u;
    for (int i = from; i < ns; ++i) {
        const float lb = v[i];
        v[i] = __builtin_inff();
        if (i > last) continue;
        if (!(fsub(lb, 1e-6f) > lim)) {
            e.mark(i);
            ++k;
        } else if (n_near < NEAR_PROBES && !(fsub(lb, 1e-6f) > fadd(lim, fmul(2.f, P.tau)))) {
            e.mark(i);
            ++k, ++n_near;
        } else {
            const unsigned h = ((unsigned)r * 2654435761u) ^ ((unsigned)(i + 1) * 0x9E3779B1u);
            const unsigned hh = (h ^ (h >> 15)) * 0x85EBCA6Bu;
            if (hh < probe_h) probe_h = hh, probe = i;
        }
    }
    if (probe >= 0) {
        e.mark(probe);
        ++k, ++n_near;
    }
    if (n_near > 0) atomicAdd(P.counters + round * NCNT + NEFII_CNT_PROBES, n_near);
    if (k > 0 && k <= CREF_CAP) {
        e.n_ref = k;
        e.ref_coarse = true;
        fl = with_win(fl, SW_GRID);
    } else {        // too many to list (or, with nothing to evaluate, no round to wait for): the whole row
        e.clear_marks();
        e.nc = 4;
    }
}

// PH_SAMPLER_C, SW_GRID: every value of the row - the evaluated samples and the leading exact ones - against both ends of its
// cell's interval (|coarse - exact| < tau); a violation lands where the slope bound's do
__device__ __forceinline__ void grid_audit(const Params &P, int64_t r, int round) {
    const int ns = P.p.n_steps;
    const float *v = P.s.big + (size_t)r * ns;
    const float a = P.s.t_s[r], rng = fsub(P.s.t_e[r], a);
    float worst = 0.f;
    int n_corner = 0;
    for (int i = 0; i < ns; ++i) {
        if (!(v[i] < __builtin_inff())) continue;
        float lo, hi;
        const float t = fadd(a, fmul(P.lin[i], rng));
        if (!grid_bounds(P, r, t, lo, hi)) continue;
        if (P.vert_g && n_corner < CREF_CAP) {      // the combined interval begin_grid_bracket relied on (probes: as if it had)
            float lo_c, hi_c;
            grid_corner_bounds(P, r, t, lo_c, hi_c);
            lo = fmaxf(lo, lo_c), hi = fminf(hi, hi_c);
            ++n_corner;
        }
        worst = fmaxf(worst, fmaxf(fsub(fsub(lo, P.tau), v[i]), fsub(v[i], fadd(hi, P.tau))));
    }
    if (worst > 0.f) atomicMax(P.counters + round * NCNT + NEFII_CNT_LIP_AUDIT, __float_as_int(worst));
}

// ---- the two grid walks, run by the whole wave -------------------------------------------------
// One thread walking its ray's n_steps samples keeps the other 63 lanes of its wave waiting through every look-up; in most
// rounds few rays of a wave search.  So the phase chain only REQUESTS a walk (Emit::walk) and the wave serves the requests
// one ray at a time (serve_grid_walks): lane i holds sample 64 p + i of pass p < ceil(n_steps / 64) (n_steps <= 128, as
// Emit::cmask has it).  Every floating-point expression a lane evaluates is the one begin_grid_bracket / grid_audit
// evaluate for that sample; what is reordered - min, max, first index, counts - does not depend on the order (fminf / fmaxf
// drop a NaN whichever side it is on, and both forms start from +inf / 0).  Outputs, counters and work lists are those of
// the thread-per-ray form, which stays behind NEFII_GRID_WALK_WAVE=0 (tests/test_gpu_grid_walk.py holds one to the other;
// tests/test_grid_walk_cpu.py the restated selection rules to the sequential ones).
__device__ __forceinline__ float wave_fmin(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ float wave_fmax(float x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
    return x;
}
__device__ __forceinline__ unsigned wave_umin(unsigned x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned y = (unsigned)__shfl_xor((int)x, o);
        x = y < x ? y : x;
    }
    return x;
}
// lowest sample index set in the ballots of the two passes
__device__ __forceinline__ int first_sample(unsigned long long b0, unsigned long long b1, int none) {
    return b0 ? __ffsll(b0) - 1 : b1 ? 63 + __ffsll(b1) : none;
}

struct GridMarks {      // what begin_grid_bracket leaves in Emit::cmask: the ballots of the two passes, and their count
    unsigned long long m0, m1;
    int k;
};

// begin_grid_bracket for ray r (wave-uniform), all lanes.  The cell pass and the survivors are plain restatements.  The
// corner pass bounds every candidate at once where the sequential loop may `break`; the two agree:
//   the candidates are fixed before the loop (lim and last are the cell pass's), and lo0 changes at sample 0 only, which the
//     loop visits first - so `obj && lo0 > 0` is one condition for the whole loop, known once sample 0 is bounded;
//   where it is false the loop never breaks: it visits every candidate, as here;
//   where it is true the loop breaks at i*, the first candidate with hi < -tau in front of the old j1 - the new j1, here
//     the lowest index of that ballot.  Then front_only holds, so lim = 0 whatever U is (U is the one quantity that may
//     differ: the candidates behind i* have lowered it here) and last = i*: the samples behind i*, whose bounds the loop
//     has not raised, are neither marked nor probed - they lie past `last` - and end at +inf like every other.
__device__ __forceinline__ GridMarks wave_grid_bracket(const Params &P, int64_t r, int round, int from) {
    const int ns = P.p.n_steps, lane = threadIdx.x & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const float inf = __builtin_inff();
    float *v = P.s.big + (size_t)r * ns;
    const float a = P.s.t_s[r], rng = fsub(P.s.t_e[r], a);
    const bool obj = P.obj[r] != 0, two = ns > 64;
    // cell pass (the lower bounds stay in registers)
    float lb[2] = {inf, inf}, t[2] = {0.f, 0.f};
    bool in[2] = {false, false};
    unsigned long long neg[2] = {0ull, 0ull};
    float U = inf;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (p && !two) continue;
        const int i = 64 * p + lane;
        in[p] = i < ns;
        float lo = inf, hi = inf;
        if (in[p] && i < from) lo = hi = v[i];
        if (in[p] && i >= from) {
            t[p] = fadd(a, fmul(P.lin[i], rng));
            grid_bounds(P, r, t[p], lo, hi);
        }
        neg[p] = __ballot(in[p] && hi < -P.tau);
        U = fminf(U, wave_fmin(in[p] ? hi : inf));
        lb[p] = lo;
    }
    int j1 = first_sample(neg[0], neg[1], ns);
    float lo0 = __shfl(lb[0], 0);
    bool front_only = obj && j1 < ns && lo0 > 0.f;
    bool sign_only = front_only || !P.miss_argmin;
    float lim = sign_only ? 0.f : fmaxf(0.f, fadd(U, P.tau));
    int last = front_only ? j1 : ns - 1;
    if (P.vert_g) {
        // corner pass
        unsigned long long negc[2] = {0ull, 0ull};
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (p && !two) continue;
            const int i = 64 * p + lane;
            float lo = -inf, hi = inf;
            bool c = in[p] && i >= from && i <= last && !(fsub(lb[p], 1e-6f) > lim);
            if (c) c = grid_corner_bounds(P, r, t[p], lo, hi);
            if (c) lb[p] = fmaxf(lb[p], lo);
            negc[p] = __ballot(c && hi < -P.tau);
            U = fminf(U, wave_fmin(c ? hi : inf));
        }
        const int jc = first_sample(negc[0], negc[1], ns);
        j1 = jc < j1 ? jc : j1;
        lo0 = __shfl(lb[0], 0);
        front_only = obj && j1 < ns && lo0 > 0.f;
        sign_only = front_only || !P.miss_argmin;
        lim = sign_only ? 0.f : fmaxf(0.f, fadd(U, P.tau));
        last = front_only ? j1 : ns - 1;
    }
    // survivors; the near-miss probes: the first NEAR_PROBES of the near set in index order; the hash probe: the least
    // (hash, index) of the rest (begin_grid_bracket's `hh < probe_h` keeps the lowest index among equal hashes, and never
    // takes a hash of ~0u)
    const float lim2 = fadd(lim, fmul(2.f, P.tau));
    bool act[2] = {false, false}, surv[2] = {false, false}, near[2] = {false, false};
    unsigned long long S[2] = {0ull, 0ull}, N[2] = {0ull, 0ull}, Sel[2] = {0ull, 0ull};
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (p && !two) continue;
        const int i = 64 * p + lane;
        const float x = fsub(lb[p], 1e-6f);
        act[p] = in[p] && i >= from && i <= last;
        surv[p] = act[p] && !(x > lim);
        near[p] = act[p] && !surv[p] && !(x > lim2);
        S[p] = __ballot(surv[p]);
        N[p] = __ballot(near[p]);
        if (in[p] && i >= from) v[i] = inf;      // skipped samples stay at +inf
    }
    unsigned hh[2] = {~0u, ~0u};
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (p && !two) continue;
        const int i = 64 * p + lane;
        const int before = (p ? __popcll(N[0]) : 0) + __popcll(N[p] & lt);
        const bool sel = near[p] && before < NEAR_PROBES;
        Sel[p] = __ballot(sel);
        if (act[p] && !surv[p] && !sel) {
            const unsigned h = ((unsigned)r * 2654435761u) ^ ((unsigned)(i + 1) * 0x9E3779B1u);
            hh[p] = (h ^ (h >> 15)) * 0x85EBCA6Bu;
        }
    }
    const unsigned hmin = wave_umin(hh[0] < hh[1] ? hh[0] : hh[1]);
    const unsigned long long P0 = __ballot(hh[0] == hmin), P1 = __ballot(hh[1] == hmin);
    const int probe = hmin != ~0u ? first_sample(P0, P1, -1) : -1;
    GridMarks g;
    g.m0 = S[0] | Sel[0] | (probe >= 0 && probe < 64 ? 1ull << probe : 0ull);
    g.m1 = S[1] | Sel[1] | (probe >= 64 ? 1ull << (probe - 64) : 0ull);
    g.k = __popcll(g.m0) + __popcll(g.m1);
    const int n_near = __popcll(Sel[0]) + __popcll(Sel[1]) + (probe >= 0 ? 1 : 0);
    if (lane == 0 && n_near > 0) atomicAdd(P.counters + round * NCNT + NEFII_CNT_PROBES, n_near);
    return g;
}

// grid_audit for ray r (wave-uniform), all lanes: the corner bounds go to the first CREF_CAP evaluated samples inside the
// cube, in index order
__device__ __forceinline__ void wave_grid_audit(const Params &P, int64_t r, int round) {
    const int ns = P.p.n_steps, lane = threadIdx.x & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const float *v = P.s.big + (size_t)r * ns;
    const float a = P.s.t_s[r], rng = fsub(P.s.t_e[r], a);
    const bool two = ns > 64;
    float x[2] = {0.f, 0.f}, t[2] = {0.f, 0.f}, lo[2] = {0.f, 0.f}, hi[2] = {0.f, 0.f};
    bool el[2] = {false, false};
    unsigned long long E[2] = {0ull, 0ull};
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (p && !two) continue;
        const int i = 64 * p + lane;
        if (i < ns) x[p] = v[i];
        if (i < ns && x[p] < __builtin_inff()) {
            t[p] = fadd(a, fmul(P.lin[i], rng));
            el[p] = grid_bounds(P, r, t[p], lo[p], hi[p]);
        }
        E[p] = __ballot(el[p]);
    }
    float worst = 0.f;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (p && !two) continue;
        if (!el[p]) continue;
        const int before = (p ? __popcll(E[0]) : 0) + __popcll(E[p] & lt);
        if (P.vert_g && before < CREF_CAP) {
            float lo_c, hi_c;
            grid_corner_bounds(P, r, t[p], lo_c, hi_c);
            lo[p] = fmaxf(lo[p], lo_c), hi[p] = fminf(hi[p], hi_c);
        }
        worst = fmaxf(worst, fmaxf(fsub(fsub(lo[p], P.tau), x[p]), fsub(x[p], fadd(hi[p], P.tau))));
    }
    worst = wave_fmax(worst);
    if (lane == 0 && worst > 0.f) atomicMax(P.counters + round * NCNT + NEFII_CNT_LIP_AUDIT, __float_as_int(worst));
}

// Called by WHOLE waves: the walks the rays of this wave have requested, one ray at a time.  A begin leaves its marks, the
// count and SW_GRID (or the whole-row fallback) with the requesting lane, as begin_grid_bracket does, and stores its flags.
__device__ __forceinline__ void serve_grid_walks(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(e.walk != WALK_NONE);
    while (pending) {
        const int src = __ffsll(pending) - 1;
        pending &= pending - 1;
        // (the rays of a wave are consecutive; all of this is wave-uniform: scalar registers, scalar loads of the ray)
        const int64_t rr = __builtin_amdgcn_readfirstlane((int)(r - lane) + src);
        const int kind = __builtin_amdgcn_readfirstlane(__shfl(e.walk, src));
        const int from = __builtin_amdgcn_readfirstlane(__shfl(e.walk_from, src));
        if (kind == WALK_AUDIT) {
            wave_grid_audit(P, rr, round);
            continue;
        }
        const GridMarks g = wave_grid_bracket(P, rr, round, from);
        if (lane == src) {
            if (g.k > 0 && g.k <= CREF_CAP) {
                e.cmask[0] = (unsigned)g.m0, e.cmask[1] = (unsigned)(g.m0 >> 32);
                e.cmask[2] = (unsigned)g.m1, e.cmask[3] = (unsigned)(g.m1 >> 32);
                e.n_ref = g.k;
                e.ref_coarse = true;
                fl = with_win(fl, SW_GRID);
            } else {        // too many to list, or nothing to evaluate: the whole row
                e.clear_marks();
                e.nc = 4;
            }
            P.s.flags[r] = fl;
        }
    }
    e.walk = WALK_NONE;
}

// a bracket search's coarse pass starts (fl: PH_SAMPLER_C, F_WIN clear; samples in front of `from` hold exact values)
__device__ __forceinline__ void begin_coarse_bracket(const Params &P, int64_t r, int round, int from, bool in_mask, int &fl, Emit &e) {
    if (P.cells && P.lip > 0.f && P.stage_bracket && (!P.p.training || (P.grid_training && in_mask))) {
        // under frozen geometry the first stage is read from the SDF interval grid: eval-mode traces, and in training mode the
        // rays inside the object mask (those outside it keep their evaluated first stage below)
        if (P.walk_wave)
            e.walk = WALK_BEGIN, e.walk_from = from;
        else
            begin_grid_bracket(P, r, round, from, fl, e);
    } else if (staged_bracket(P, r)) {
        // staged search (minsdf_lipschitz): a quarter row's worth of samples spread over the row first
        // (leading samples keep their exact values: evaluated samples like any other)
        begin_stage1(P, r, from, SW_STAGE1, fl, e);
    } else if ((P.window & 1) && in_mask) {
        // inside the object mask the search ends at the first negative sample: the quarter rows go out one
        // at a time (P.window; outside the mask the argmin over the whole row is the result)
        e.nc = 1;
        fl = with_win(fl, SW_WINDOW_1);
    } else {
        e.nc = 4;
    }
}

// tracing finished for this ray (ray_tracing.py:43-64): on to the bracket search between the two fronts, or - no live front
// left - to the stage behind it
__device__ __forceinline__ int end_trace(const Params &P, int64_t r, int round, int &fl, Emit &e, float t_s, float t_e,
                                         float cur_s, float cur_e, bool live_s, int it) {
    const bool coarse = P.tau > 0.f;
    const bool hit = t_s < t_e;
    // (the K field is free from here on: it keeps the iterations this ray's sphere tracing took - read by
    // tools/tier_parity.py from the workspace, by nothing else)
    fl = (fl & F_SPH) | (hit ? F_HIT : 0) | (live_s ? F_SAMP : 0) | ((it & F_K_MASK) << F_K_SHIFT);
    P.s.t_s[r] = t_s;
    P.s.t_e[r] = t_e;
    if (!live_s) {
        P.s.mid[r] = t_s;      // dist so far
        return PH_POST;        // falls through to the post-sampler stage
    }
    // what is left between the two fronts is often a short stretch hugging the surface (a grazing ray):
    // the SDF is ~1-Lipschitz, so |sdf| <= (sdf_s + sdf_e + length) / 2 on it - when that is within the
    // coarse pass's error bound nearly every sample would have to be refined, and the samples go to the
    // split evaluator directly (a performance choice only: either way decides from exact values)
    const bool go_coarse = coarse && 0.5f * (cur_s + cur_e + (t_e - t_s)) > 3.f * P.tau;
    // inside the object mask (outside it the argmin over ALL samples is the result) the first `chunk`
    // samples go ahead in split precision: PH_SAMPLER_X
    // ... when a negative sample among them is plausible: the SDF at the front (cur_s, ~ the distance to
    // the surface) is within reach of the chunk's last sample (a heuristic about WHICH path is cheaper -
    // either way decides from exact values)
    if (go_coarse && P.chunk > 0 && P.obj[r] != 0 &&
        cur_s <= P.chunk_gate * (float)(P.chunk - 1) * (t_e - t_s) / (float)(P.p.n_steps - 1)) {
        fl |= PH_SAMPLER_X;
        e.n_ref = P.chunk;
        e.cmask[0] = (1u << P.chunk) - 1u;
    } else {
        fl |= go_coarse ? PH_SAMPLER_C : PH_SAMPLER;
        e.qd = !go_coarse;
        if (go_coarse) begin_coarse_bracket(P, r, round, 0, P.obj[r] != 0, fl, e);
    }
    e.n_alg = 1;
    e.dense_which = 0;
    P.s.flags[r] = fl;
    return PH_WAIT;
}

// PH_TRACE: sphere tracing of both ends + back-off line search
__device__ __forceinline__ int step_trace(const Params &P, int64_t r, int round, int &fl, Emit &e, int &looks) {
    const nefii_tracer_params &tp = P.p;
    if (P.certify_free && (fl & F_PROBE)) {
        // the probe of a ray certify_free_stretch ended is in: against both ends of its cell's interval, as grid_audit does
        const float v = P.s.res_s[r];
        float lo, hi;
        if (grid_bounds(P, r, P.s.t_s[r], lo, hi)) {
            const float worst = fmaxf(fsub(fsub(lo, P.tau), v), fsub(v, fadd(hi, P.tau)));
            if (worst > 0.f) atomicMax(P.counters + round * NCNT + NEFII_CNT_LIP_AUDIT, __float_as_int(worst));
        }
        finish(P, r, P.s.mid[r], false);
        fl = F_SPH | F_CERT | PH_DONE;
        P.s.flags[r] = fl;
        return PH_WAIT;
    }
    const bool tier = P.tier_band > 0.f;
    const float thr = tp.sdf_threshold;
    float t_s = P.s.t_s[r], t_e = P.s.t_e[r];
    float cur_s = P.s.cur_s[r], cur_e = P.s.cur_e[r];
    float nxt_s = P.s.nxt_s[r], nxt_e = P.s.nxt_e[r];
    bool live_s = fl & F_LIVE_S, live_e = fl & F_LIVE_E;
    int it = (fl >> F_IT_SHIFT) & F_IT_MASK, k = (fl >> F_K_SHIFT) & F_K_MASK;
    if (fl & F_PEND_S) nxt_s = P.s.res_s[r];
    if (fl & F_PEND_E) nxt_e = P.s.res_e[r];
    // Tiered sphere tracing (nefii_tracer_params.trace_tier).  What the recurrence decides with an SDF value v is
    // `v <= thr` (the front has arrived) and `v < 0` (back off); a value v16 of the single-pass evaluator, |v16 - v| <
    // tau, decides both the same way when |v16| > tier_band (>= tau + thr) - it is then taken AS the value: the front
    // advances by v16 instead of v (not bit-identical to the split-precision trace: DESIGN, "tiered sphere tracing").
    // Inside the band the same query is repeated in split precision before anything moves.
    fl &= ~(F_AUD_S | F_AUD_E);
    const bool rep_s = (fl & F_PEND_S) && (fl & F_CRS_S) && !(fabsf(nxt_s) > P.tier_band);
    const bool rep_e = (fl & F_PEND_E) && (fl & F_CRS_E) && !(fabsf(nxt_e) > P.tier_band);
    if (rep_s || rep_e) {
        if (rep_s) e.qs = true, fl = (fl & ~F_CRS_S) | F_AUD_S, ++e.n_rep;
        if (rep_e) e.qe = true, fl = (fl & ~F_CRS_E) | F_AUD_E, ++e.n_rep;
        P.s.flags[r] = fl;         // everything else as it is: the other end's result stays in res_x and is read again
        return PH_WAIT;
    }
    bool wait = false;
    fl &= ~(F_CRS_S | F_CRS_E);
    if (fl & F_STEPPED) {
        // back-off line search for ends that crossed the surface (ray_tracing.py:170-188)
        const bool bad_s = nxt_s < 0.f, bad_e = nxt_e < 0.f;
        if ((bad_s || bad_e) && k < tp.line_step_iters) {
            const float back = (1.f - tp.line_search_step) / (float)(1 << k);
            fl &= ~(F_PEND_S | F_PEND_E);
            if (bad_s) {
                t_s = fsub(t_s, fmul(back, cur_s));
                e.qs = true;
                e.cs = tier && back * cur_s > P.tier_gate;
                fl |= F_PEND_S | (e.cs ? F_CRS_S : 0);
            }
            if (bad_e) {
                t_e = fadd(t_e, fmul(back, cur_e));
                e.qe = true;
                e.ce = tier && back * cur_e > P.tier_gate;
                fl |= F_PEND_E | (e.ce ? F_CRS_E : 0);
            }
            ++k;
            wait = true;
        } else {
            live_s = live_s && (t_s < t_e);
            live_e = live_e && (t_s < t_e);
        }
    }
    if (!wait) {
        // loop top (ray_tracing.py:136-157)
        cur_s = live_s ? nxt_s : 0.f;
        if (cur_s <= thr) cur_s = 0.f;
        cur_e = live_e ? nxt_e : 0.f;
        if (cur_e <= thr) cur_e = 0.f;
        live_s = live_s && (cur_s > thr);
        live_e = live_e && (cur_e > thr);
        if (it == tp.sphere_tracing_iters || !(live_s || live_e)) return end_trace(P, r, round, fl, e, t_s, t_e, cur_s, cur_e, live_s, it);
        ++it;
        t_s = fadd(t_s, cur_s);
        t_e = fsub(t_e, cur_e);
        // (before the round's queries go out) the rest of the ray proven free of the surface: a miss nobody reads
        if (P.certify_free && live_s && t_s < t_e && certify_free_stretch(P, r, t_s, looks)) return end_free(P, r, round, fl, e, t_s);
        nxt_s = 0.f;
        nxt_e = 0.f;
        k = 0;
        fl &= ~(F_PEND_S | F_PEND_E);
        if (live_s) {
            e.qs = true;
            e.cs = tier && cur_s > P.tier_gate;     // the step just taken ~ the distance the front was from the surface
            fl |= F_PEND_S | (e.cs ? F_CRS_S : 0);
        }
        if (live_e) {
            e.qe = true;
            e.ce = tier && cur_e > P.tier_gate;
            fl |= F_PEND_E | (e.ce ? F_CRS_E : 0);
        }
        fl |= F_STEPPED;
    }
    // a step or a back-off is under way
    fl &= ~(F_LIVE_S | F_LIVE_E | (F_IT_MASK << F_IT_SHIFT) | (F_K_MASK << F_K_SHIFT));
    fl |= (live_s ? F_LIVE_S : 0) | (live_e ? F_LIVE_E : 0) | (it << F_IT_SHIFT) | (k << F_K_SHIFT);
    P.s.t_s[r] = t_s;
    P.s.t_e[r] = t_e;
    P.s.cur_s[r] = cur_s;
    P.s.cur_e[r] = cur_e;
    P.s.nxt_s[r] = nxt_s;
    P.s.nxt_e[r] = nxt_e;
    P.s.flags[r] = fl;
    return PH_WAIT;
}

// PH_SAMPLER_X
__device__ __forceinline__ int sampler_leading(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    // the first `chunk` samples hold EXACT values.  A negative one among them at index >= 1 (index 0 would pair with
    // the LAST sample, ray_tracing.py:245-246) settles the search: `ind` is the first negative sample, the bracket is
    // (ind - 1, ind), the ray has a hit inside the object mask, so neither the argmin nor any later sample is read -
    // the exact stage below runs on these values with the rest of the row out of the way.  Otherwise: all n_steps
    // samples through the coarse evaluator, as if this stage had not been.
    const int ns = P.p.n_steps;
    float *v = P.s.big + (size_t)r * ns;
    int ind = -1;
    for (int i = 0; i < P.chunk; ++i)
        if (v[i] < 0.f && ind < 0) ind = i;
    if (ind >= 1) {
        for (int i = P.chunk; i < ns; ++i) v[i] = 3.0e38f;
        return PH_SAMPLER;
    }
    fl = (fl & ~F_PHASE) | PH_SAMPLER_C;
    begin_coarse_bracket(P, r, round, P.chunk, true, fl, e);      // (PH_SAMPLER_X rays lie inside the object mask)
    e.dense_which = 0;
    P.s.flags[r] = fl;
    return PH_WAIT;
}

// ---- the staged searches' walk ---------------------------------------------------------------
// Both dense searches are staged the same way (nefii_tracer_params.minsdf_lipschitz): a first stage of stage1_count
// samples spread over the SORTED depths of the row is in; the walk visits the sorted positions between them.  Lower bound
// of sample s between evaluated neighbours a < s < b from the Lipschitz bound L and the coarse values c (|c - v| < tau):
//   v_s >= max(c_a - L (t_s - t_a), c_b - L (t_b - t_s)) - tau.
//   first stage done: s is skipped for good when that bound exceeds the search's limit `lim`; the others go to the coarse
//     evaluator one by one (list crefine) - with a few of the skipped ones as PROBES of the audit;
//   second stage done: every sample evaluated since is audited against the bound (c_s > bound - tau must hold).
// A Search says what differs: sample(k), the row index of sorted position k; depth(i), where sample i lies on [0, 1];
// lim; skip(k, v), positions of the first walk that need no decision; STAGE2, the F_WIN code of its second stage; WHICH,
// the row's list entry when more than CREF_CAP samples survive and the whole row goes out, as without the staging.
// Returns true when the ray waits for evaluations (flags stored), false when the row's values are in.
template <typename Search>
__device__ __forceinline__ bool staged_walk(const Params &P, int64_t r, int round, int &fl, Emit &e, const float *v, float Llen,
                                            bool stage1, const Search &S) {
    const int ns = P.p.n_steps;
    int *cnt = P.counters + round * NCNT;
    int ja = 0, k = 0, n_near = 0;
    float worst = 0.f;
    int probe = -1;             // one of the SKIPPED samples, picked by a hash of (ray, position): evaluated after all, so that
    unsigned probe_h = ~0u;     // the audit also sees the bound where it was relied upon (a ray costs one evaluation more)
    for (int kk = 1; kk < ns - 1; ++kk) {
        if (kk == stage1_pos(ns, ja + 1)) {
            ++ja;
            continue;
        }
        const int ia = S.sample(stage1_pos(ns, ja)), ib = S.sample(stage1_pos(ns, ja + 1)), is = S.sample(kk);
        const float sa = S.depth(ia), sb = S.depth(ib), ss = S.depth(is);
        const float lb = fsub(fmaxf(fsub(v[ia], fmul(Llen, fsub(ss, sa))), fsub(v[ib], fmul(Llen, fsub(sb, ss)))), P.tau);
        if (stage1) {
            if (S.skip(kk, v)) continue;
            if (!(fsub(lb, 1e-6f) > S.lim)) {
                e.mark(is);
                ++k;
            } else if (n_near < NEAR_PROBES && !(fsub(lb, 1e-6f) > fadd(S.lim, fmul(2.f, P.tau)))) {
                // skipped, but its bound clears the limit by less than 2 tau: the skipped samples closest to mattering are
                // evaluated after all - as PROBES of the audit (the second walk holds every evaluated sample against its
                // bound); a probe's value decides nothing the bound had not decided (ABI 15, NEFII_CNT_PROBES)
                e.mark(is);
                ++k, ++n_near;
            } else {
                const unsigned h = ((unsigned)r * 2654435761u) ^ ((unsigned)(kk + 1) * 0x9E3779B1u);
                const unsigned hh = (h ^ (h >> 15)) * 0x85EBCA6Bu;
                if (hh < probe_h) probe_h = hh, probe = is;
            }
        } else if (v[is] < __builtin_inff()) {
            worst = fmaxf(worst, fsub(fsub(lb, P.tau), v[is]));
        }
    }
    fl = with_win(fl, 0);       // (SW_WHOLE_ROW / MW_ROW_IN, unless a second stage follows)
    if (stage1 && probe >= 0) {
        e.mark(probe);
        ++k, ++n_near;
    }
    if (stage1 && n_near > 0) atomicAdd(cnt + NEFII_CNT_PROBES, n_near);
    if (stage1 && k > 0) {
        if (k <= CREF_CAP) {
            e.n_ref = k;
            e.ref_coarse = true;
            fl = with_win(fl, Search::STAGE2);
        } else {        // too many to list: the whole row, as without the staging
            e.clear_marks();
            e.nc = 4;
            e.dense_which = Search::WHICH;
        }
        P.s.flags[r] = fl;
        return true;
    }
    // (samples that hold exact values are audited with the rest: an exact value obeys the bound a fortiori)
    if (worst > 0.f) atomicMax(cnt + NEFII_CNT_LIP_AUDIT, __float_as_int(worst));
    e.clear_marks();      // the row's values are in: decided further down, this round
    return false;
}

// the bracket search's samples: sorted as they are, at P.lin
struct BracketSearch {
    const float *lin;
    float lim;
    int last;               // samples from here on are not needed
    static constexpr int STAGE2 = SW_STAGE2;
    static constexpr unsigned WHICH = 0;
    __device__ __forceinline__ int sample(int k) const { return k; }
    __device__ __forceinline__ float depth(int i) const { return lin[i]; }
    // not needed / one of the leading exact samples
    __device__ __forceinline__ bool skip(int k, const float *v) const { return k >= last || v[k] < __builtin_inff(); }
};

// the min-SDF search's depths: the row's uniform draws, visited in their sorted order ord[]
struct MinSdfSearch {
    const Params &P;
    int64_t r;
    const unsigned char *ord;
    float lim;
    static constexpr int STAGE2 = MW_STAGE2;
    static constexpr unsigned WHICH = 1;
    __device__ __forceinline__ int sample(int k) const { return ord[k]; }
    __device__ __forceinline__ float depth(int i) const { return minsdf_step(P, r, i); }
    __device__ __forceinline__ bool skip(int, const float *) const { return false; }
};

// PH_SAMPLER_C, SW_STAGE1 / SW_STAGE2
__device__ __forceinline__ int sampler_staged(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    // Staged bracket search (staged_walk).  What the search decides: the FIRST negative sample and - unless the ray lies
    // inside the object mask and surely has one - the argmin.
    //   stage 1 done: with a surely negative first-stage sample j1 on a ray inside the mask only the samples in front
    //     of j1 matter, and only their sign: s is skipped for good when its bound is > 0.  Otherwise s must also not be
    //     the argmin: skipped when its bound exceeds max(0, best + tau);
    //   stage 2 done: audit, then the row - skipped samples at +inf: positive, never a minimum - is decided as a whole.
    const int ns = P.p.n_steps, n1 = stage1_count(ns);
    const float *v = P.s.big + (size_t)r * ns;
    if (win_of(fl) == SW_GRID) {        // the search started from the grid: audit, then the row is decided as a whole
        if (P.walk_wave)
            e.walk = WALK_AUDIT;        // (served before anything further down the chain can reuse the row)
        else
            grid_audit(P, r, round);
        fl = with_win(fl, SW_WHOLE_ROW);
        return PH_SAMPLER_C;
    }
    const float Llen = fmul(P.lip, fsub(P.s.t_e[r], P.s.t_s[r]));
    const bool obj = P.obj[r] != 0;
    float best = __builtin_inff();
    int j1 = ns;
    for (int j = 0; j < n1; ++j) {
        const int i = stage1_pos(ns, j);
        best = fminf(best, v[i]);
        if (v[i] < -P.tau && j1 == ns) j1 = i;
    }
    const bool front_only = obj && j1 < ns && !(v[0] < P.tau);      // (sample 0 possibly negative: the row is decided as a whole)
    const bool sign_only = front_only || !P.miss_argmin;
    const BracketSearch S = {P.lin, sign_only ? 0.f : fmaxf(0.f, fadd(best, P.tau)), front_only ? j1 : ns - 1};
    return staged_walk(P, r, round, fl, e, v, Llen, win_of(fl) == SW_STAGE1, S) ? PH_WAIT : PH_SAMPLER_C;
}

// PH_SAMPLER_C, SW_WINDOW_1 .. SW_WINDOW_4
__device__ __forceinline__ int sampler_windows(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    // Windowed search (rays inside the object mask): the first wn quarter rows hold coarse values.  A sample that is
    // SURELY negative (< -tau) among them ends the search exactly as the whole row would: the decision below reads the
    // samples up to it only (no argmin: the ray has its negative sample inside the mask), so the rest of the row gets out
    // of the way unevaluated.  Not if the first candidate is sample 0 - its bracket partner is the LAST sample
    // (ray_tracing.py:245-246): then, and when all four quarters are in, the row is completed and decided as a whole.
    const int ns = P.p.n_steps, cw = coarse_window(ns);
    const int wn = win_of(fl);
    const int have = wn * cw < ns ? wn * cw : ns;
    float *v = P.s.big + (size_t)r * ns;
    int i0 = -1, i1 = -1;
    for (int i = 0; i < have; ++i) {
        const float x = v[i];
        if (x < P.tau && i0 < 0) i0 = i;
        if (x < -P.tau && i1 < 0) i1 = i;
    }
    if (i1 >= 0 && i0 > 0) {
        for (int i = have; i < ns; ++i) v[i] = 3.0e38f;
        fl = with_win(fl, SW_WHOLE_ROW);                    // decided below, this round
    } else if (have < ns) {
        const bool rest = i0 == 0;                          // all remaining quarters at once
        e.nc = rest ? 4 - wn : 1;
        e.cwin = wn;
        fl = with_win(fl, rest ? SW_WINDOW_4 : wn + 1);
        e.dense_which = 0;
        P.s.flags[r] = fl;
        return PH_WAIT;
    } else {
        fl = with_win(fl, SW_WHOLE_ROW);                    // the whole row is in
    }
    return PH_SAMPLER_C;
}

// PH_SAMPLER_C, SW_WHOLE_ROW
__device__ __forceinline__ int sampler_coarse(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    // The n_steps samples hold COARSE values v16 with |v16 - v| < tau.  What the exact stage below decides from them:
    // the first negative sample `ind`, the signs at ind and ind-1 (bracket), and - unless the ray surely has a
    // negative sample and lies inside the object mask - the argmin.  Samples that cannot decide from their coarse
    // value are re-evaluated in split precision (refine list; next round's exact stage then sees exact values
    // exactly where it matters); with none, the exact stage runs right away on the coarse values.
    const int ns = P.p.n_steps;
    const float tau = P.tau;
    const float *v = P.s.big + (size_t)r * ns;
    int i0 = -1, i1 = -1;           // first sample that may be negative / that surely is
    float vmin = v[0];
    for (int i = 0; i < ns; ++i) {
        const float x = v[i];
        if (x < tau && i0 < 0) i0 = i;
        if (x < -tau && i1 < 0) i1 = i;
        vmin = x < vmin ? x : vmin;
    }
    const bool obj = P.obj[r] != 0;
    const bool need_argmin = P.miss_argmin && !(obj && i1 >= 0);
    int n_sign = 0, n_min = 0;
    if (i0 >= 0) {
        const int end = i1 >= 0 ? i1 : ns;
        for (int i = i0; i < end; ++i)
            if (v[i] < tau) {
                e.mark(i);
                ++n_sign;
            }
        // bracket quirk: ind = 0 pairs with sample ns-1 (ray_tracing.py:245-246)
        if (i0 == 0 && fabsf(v[ns - 1]) < tau && !e.marked(ns - 1)) {
            e.mark(ns - 1);
            ++n_sign;
        }
    }
    if (need_argmin) {
        const float lim = vmin + 2.f * tau;
        for (int i = 0; i < ns; ++i)
            if (v[i] <= lim) {
                e.mark(i);
                ++n_min;
            }
    }
    if (n_sign == 0 && n_min <= 1) return PH_SAMPLER;       // every decision is certain from the coarse values
    const int k = __popc(e.cmask[0]) + __popc(e.cmask[1]) + __popc(e.cmask[2]) + __popc(e.cmask[3]);
    if (k <= P.cap) e.n_ref = k; else e.qd = true;      // too many: all n_steps samples in split precision
    e.dense_which = 0;
    fl = (fl & ~F_PHASE) | PH_SAMPLER;
    P.s.flags[r] = fl;
    return PH_WAIT;
}

// PH_SAMPLER
__device__ __forceinline__ int sampler_exact(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    // first sign change among the n_steps samples, argmin fallback, bracket (ray_tracing.py:203-255)
    const nefii_tracer_params &tp = P.p;
    const int ns = tp.n_steps;
    const float a = P.s.t_s[r], rng = fsub(P.s.t_e[r], a);
    const float *v = P.s.big + (size_t)r * ns;
    int ind = -1, zero = -1, amin = 0;
    float vmin = v[0];
    for (int i = 0; i < ns; ++i) {
        const float x = v[i];
        if (x < 0.f && ind < 0) ind = i;
        if (x == 0.f && zero < 0) zero = i;
        if (x < vmin) {
            vmin = x;
            amin = i;
        }
    }
    if (ind < 0) ind = zero >= 0 ? zero : ns - 1;
    const bool net_hit = v[ind] < 0.f;
    const bool obj = P.obj[r] != 0;
    float dist = fadd(a, fmul(P.lin[ind], rng));
    if (!(obj && net_hit)) dist = fadd(a, fmul(P.lin[amin], rng));
    fl = (fl & ~F_HIT) | (net_hit ? F_HIT : 0);
    const bool root = tp.training ? (net_hit && obj) : net_hit;
    if (root) {
        const int im = ind > 0 ? ind - 1 : ns - 1;
        const float hi = fadd(a, fmul(P.lin[ind], rng)), f_hi = v[ind];
        const float lo = fadd(a, fmul(P.lin[im], rng)), f_lo = v[im];
        const float mid = fmul(fadd(lo, hi), 0.5f);
        const bool work = (f_lo > 0.f) && (f_hi < 0.f) && (hi > lo);
        dist = mid;
        if (work && tp.n_rootfind_steps > 0) {
            P.s.lo[r] = lo;
            P.s.hi[r] = hi;
            P.s.mid[r] = mid;
            fl = (fl & ~(F_PHASE | (F_IT_MASK << F_IT_SHIFT))) | PH_BISECT;
            e.qt = true;
            P.s.flags[r] = fl;
            return PH_WAIT;
        }
    }
    P.s.mid[r] = dist;
    return PH_POST;
}

// PH_BISECT
__device__ __forceinline__ int bisect(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    // up to `bisect_levels` bisection steps per round (ray_tracing.py:264-277, per ray): the nodes of the next
    // levels of the bisection tree were evaluated speculatively last round; walk them with the sequential rule
    float lo = P.s.lo[r], hi = P.s.hi[r], mid = P.s.mid[r];
    const float *f = P.s.big + (size_t)r * P.p.n_steps;
    int it = (fl >> F_IT_SHIFT) & F_IT_MASK;
    int node = 0;
    bool more = true;
    for (int level = 0; level < P.levels && more; ++level) {
        const float f_mid = f[node];
        ++e.consumed;
        const int bit = f_mid > 0.f ? 1 : 0;
        if (bit) lo = mid; else hi = mid;
        mid = fmul(fadd(lo, hi), 0.5f);
        ++it;
        more = (fsub(hi, lo) > 1e-6f) && (it < P.p.n_rootfind_steps);
        node = 2 * node + 1 + bit;
    }
    P.s.mid[r] = mid;
    if (!more) return PH_POST;
    P.s.lo[r] = lo;
    P.s.hi[r] = hi;
    fl = (fl & ~(F_IT_MASK << F_IT_SHIFT)) | (it << F_IT_SHIFT);
    P.s.flags[r] = fl;
    e.qt = true;
    return PH_WAIT;
}

// PH_POST
__device__ __forceinline__ int post(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    // after tracing / sampler: eval mode returns; training mode handles rays that miss (:71-97)
    const bool coarse = P.tau > 0.f;
    float dist = P.s.mid[r];
    const bool hit = fl & F_HIT, samp = fl & F_SAMP, sph = fl & F_SPH;
    const bool obj = P.obj[r] != 0;
    bool done = true;
    if (P.p.training) {
        const bool in_m = !hit && obj && !samp, out_m = !obj && !samp;
        if (in_m || out_m) {
            if (!sph) {
                const float ox = P.o[r * 3], oy = P.o[r * 3 + 1], oz = P.o[r * 3 + 2];
                const float dx = P.d[r * 3], dy = P.d[r * 3 + 1], dz = P.d[r * 3 + 2];
                dist = -fadd(fadd(fmul(dx, ox), fmul(dy, oy)), fmul(dz, oz));
            } else {
                if (hit && out_m) P.s.t_min[r] = dist;
                fl = (fl & ~F_PHASE) | (coarse ? PH_MINSDF_C : PH_MINSDF);
                e.qd = !coarse;
                e.nc = coarse ? 4 : 0;
                // staged search: a quarter row's worth of the depths, spread over their sorted order, first
                if (coarse && P.lip > 0.f) begin_stage1(P, r, 0, MW_STAGE1, fl, e);
                // ... unless the first stage is shared: nothing goes out before minsdf_share has looked for a donor
                if (coarse && P.lip > 0.f && P.share) {
                    e.nc = 0;
                    fl = with_win(fl, MW_ENTER);
                }
                P.s.flags[r] = fl;
                e.n_alg = 1;
                e.dense_which = 1;
                done = false;
            }
        }
    }
    if (done) {
        finish(P, r, dist, hit);
        P.s.flags[r] = (fl & ~F_PHASE) | PH_DONE;
    }
    return PH_WAIT;
}

// PH_MINSDF_C, MW_STAGE1 / MW_STAGE2
__device__ __forceinline__ int minsdf_staged(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    // Staged min-SDF search (staged_walk) over the depths in sorted order.
    //   stage 1 done: s is skipped for good when its bound exceeds best + tau >= the exact value at the lowest
    //     first-stage depth - it is not the argmin;
    //   stage 2 done: audit, then the argmin over the row's coarse values as without the staging.
    const int ns = P.p.n_steps, n1 = stage1_count(ns);
    const float *v = P.s.big + (size_t)r * ns;
    const unsigned char *ord = P.s.ord + (size_t)minsdf_row(P, r) * ns;
    const float Llen = fmul(P.lip, fsub(P.s.t_max[r], P.s.t_min[r]));
    float best = __builtin_inff();
    for (int j = 0; j < n1; ++j) best = fminf(best, v[ord[stage1_pos(ns, j)]]);
    const MinSdfSearch S = {P, r, ord, fadd(best, P.tau)};
    return staged_walk(P, r, round, fl, e, v, Llen, win_of(fl) == MW_STAGE1, S) ? PH_WAIT : PH_MINSDF_C;
}

// ---- shared first stage of the staged min-SDF search -----------------------------------------
// The slope bound L is a bound in space, not only along a ray: a value v_c[i] that ray c holds at depth fraction s_i (coarse
// or exact: |v_c[i] - f(p_c(s_i))| <= tau either way) bounds the exact value of ray f at the same fraction,
//   lo_i = v_c[i] - L d_i - tau <= f(p_f(s_i)) <= v_c[i] + L d_i + tau = up_i,    d_i = |p_f(s_i) - p_c(s_i)|,
// with each ray's own origin, direction, t_min and t_max.  The rays of one pixel are millimetres apart, so a ray whose
// wave holds a finished search (the DONOR: same row of draws, F_OWN, row in) takes these bounds in place of a first stage:
//   U = min up_i bounds its exact minimum from above; a depth between the donor's evaluated neighbours a < s < b in sorted
//   order has the lower bound max(lo_a - L len (s - s_a), lo_b - L len (s_b - s)), an evaluated one lo_i itself; what
//   clears U (by staged_walk's 1e-6) is skipped for good, the rest goes to the coarse evaluator through crefine.
// The exact argmin's bound is <= its value <= U, so it - and any sample tying with it - is never skipped.  Probes and the
// audit are staged_walk's: one hash-picked skipped depth and up to NEAR_PROBES within 2 tau of mattering are evaluated
// after all, and the second pass holds every evaluated depth against the bound (recomputed from the donor's row, whose
// refined entries hold exact values by then: bounds of the same kind).
// With more than stage1_count depths to evaluate (probes included) the ray runs its own two-stage search instead - no
// ray evaluates more than it would alone.
struct RayLine {       // p(s) = a + s b over the min-SDF search's stretch of a ray
    float ax, ay, az, bx, by, bz;
};
__device__ __forceinline__ RayLine minsdf_line(const Params &P, int64_t r) {
    const float t0 = P.s.t_min[r], len = fsub(P.s.t_max[r], t0);
    const float dx = P.d[r * 3], dy = P.d[r * 3 + 1], dz = P.d[r * 3 + 2];
    return {fadd(P.o[r * 3], fmul(t0, dx)), fadd(P.o[r * 3 + 1], fmul(t0, dy)), fadd(P.o[r * 3 + 2], fmul(t0, dz)),
            fmul(len, dx), fmul(len, dy), fmul(len, dz)};
}

// the walk of ray r over donor c's row.  first: decide and emit (false: too many, nothing emitted); else: audit
__device__ __forceinline__ bool shared_walk(const Params &P, int64_t r, int64_t c, int round, Emit &e, bool first) {
    const int ns = P.p.n_steps;
    int *cnt = P.counters + round * NCNT;
    const float *v = P.s.big + (size_t)r * ns, *vc = P.s.big + (size_t)c * ns;
    const unsigned char *ord = P.s.ord + (size_t)minsdf_row(P, r) * ns;
    const RayLine f = minsdf_line(P, r), d = minsdf_line(P, c);
    const float ax = fsub(f.ax, d.ax), ay = fsub(f.ay, d.ay), az = fsub(f.az, d.az);
    const float bx = fsub(f.bx, d.bx), by = fsub(f.by, d.by), bz = fsub(f.bz, d.bz);
    const float Llen = fmul(P.lip, fsub(P.s.t_max[r], P.s.t_min[r]));
    // L d_i + tau (1e-6: the evaluators round their points differently, by a few ulp of a coordinate)
    auto slack = [&](float s) {
        const float x = fadd(ax, fmul(s, bx)), y = fadd(ay, fmul(s, by)), z = fadd(az, fmul(s, bz));
        return fadd(fmul(P.lip, fadd(sqrtf(fadd(fadd(fmul(x, x), fmul(y, y)), fmul(z, z))), 1e-6f)), P.tau);
    };
    float U = __builtin_inff();
    if (first)
        for (int i = 0; i < ns; ++i)
            if (vc[i] < __builtin_inff()) U = fminf(U, fadd(vc[i], slack(minsdf_step(P, r, i))));
    float lo_a = -__builtin_inff(), s_a = 0.f, lo_b = -__builtin_inff(), s_b = 1.f, worst = 0.f;
    int kb = -1, k = 0, n_near = 0, probe = -1;
    unsigned probe_h = ~0u;
    for (int kk = 0; kk < ns; ++kk) {
        const int is = ord[kk];
        const float ss = minsdf_step(P, r, is);
        float lb;
        if (vc[is] < __builtin_inff()) {
            lb = lo_a = fsub(vc[is], slack(ss));
            s_a = ss;
        } else {
            if (kb < kk) {      // the donor's next evaluated depth in sorted order (the ends of a staged row always are)
                lo_b = -__builtin_inff();
                for (kb = kk + 1; kb < ns; ++kb) {
                    const int ib = ord[kb];
                    if (vc[ib] < __builtin_inff()) {
                        s_b = minsdf_step(P, r, ib);
                        lo_b = fsub(vc[ib], slack(s_b));
                        break;
                    }
                }
            }
            lb = fmaxf(fsub(lo_a, fmul(Llen, fsub(ss, s_a))), fsub(lo_b, fmul(Llen, fsub(s_b, ss))));
        }
        if (!first) {
            if (v[is] < __builtin_inff()) worst = fmaxf(worst, fsub(fsub(lb, P.tau), v[is]));
        } else if (!(fsub(lb, 1e-6f) > U)) {
            e.mark(is);
            ++k;
        } else if (n_near < NEAR_PROBES && !(fsub(lb, 1e-6f) > fadd(U, fmul(2.f, P.tau)))) {
            e.mark(is);
            ++k, ++n_near;
        } else {
            const unsigned h = ((unsigned)r * 2654435761u) ^ ((unsigned)(kk + 1) * 0x9E3779B1u);
            const unsigned hh = (h ^ (h >> 15)) * 0x85EBCA6Bu;
            if (hh < probe_h) probe_h = hh, probe = is;
        }
    }
    if (!first) {
        if (worst > 0.f) atomicMax(cnt + NEFII_CNT_LIP_AUDIT, __float_as_int(worst));
        return true;
    }
    if (probe >= 0) {
        e.mark(probe);
        ++k, ++n_near;
    }
    if (k > stage1_count(ns)) {
        e.clear_marks();
        return false;
    }
    if (n_near > 0) atomicAdd(cnt + NEFII_CNT_PROBES, n_near);
    e.n_ref = k;
    e.ref_coarse = true;
    return true;
}

// PH_MINSDF_C, MW_ENTER.  Called by WHOLE waves (ballots): who follows whom, who searches on its own, who waits.
//   a donor is in (fl0, the flags this round began with: F_OWN and past its second stage - a row the evaluators have
//     written before this launch and that only refinement touches from here on): its lowest lane is followed, this round;
//   none, but a ray of the row runs its own search: wait - nothing goes out, the flags stay, the block stays live;
//   neither: the lowest entering lane of the row leads - it searches as without the sharing - and the others wait.
// A ray with F_OWN never waits, so every wait ends: within two rounds a search of the row is in.  Rows of draws
// (minsdf_group) are runs of consecutive rays, hence of consecutive lanes: `mine` is the ray's run within its wave.
__device__ __forceinline__ int minsdf_share(const Params &P, int64_t r, int round, int ph, int fl0, int &fl, Emit &e) {
    const int lane = threadIdx.x & 63;
    const int p0 = fl0 & F_PHASE;
    const bool own = fl0 & F_OWN, stage1 = p0 == PH_MINSDF_C && win_of(fl0) == MW_STAGE1;
    const bool ready = own && (p0 == PH_DONE || p0 == PH_MINSDF || (p0 == PH_MINSDF_C && !stage1));
    const bool want = (fl & F_PHASE) == PH_MINSDF_C && win_of(fl) == MW_ENTER;
    unsigned long long mine = ~0ull;
    const int g = P.p.minsdf_group;
    if (g > 0) {
        const int64_t base = r - lane, head = (r / g) * g - base, tail = head + g - 1;
        const int lo = head > 0 ? (int)head : 0, hi = tail < 63 ? (int)tail : 63;
        mine = (hi >= 63 ? ~0ull : (1ull << (hi + 1)) - 1ull) & ~((1ull << lo) - 1ull);
    }
    const unsigned long long donors = __ballot(ready) & mine, busy = __ballot(own && stage1) & mine;
    const unsigned long long free_lanes = __ballot(want && !donors && !busy) & mine;
    if (!want) return ph;
    bool search = !donors && !busy && __ffsll(free_lanes) - 1 == lane;
    if (donors) {
        const int c = __ffsll(donors) - 1;
        if (shared_walk(P, r, r - lane + c, round, e, true))
            fl = (with_win(fl, MW_SHARED) & ~(F_IT_MASK << F_IT_SHIFT)) | (c << F_IT_SHIFT);
        else
            search = true;
    }
    if (search) {
        e.nc = 1;
        e.cwin = CWIN_STAGE1;
        fl = with_win(fl, MW_STAGE1) | F_OWN;
    }
    e.dense_which = 1;
    P.s.flags[r] = fl;
    return PH_WAIT;
}

// PH_MINSDF_C, MW_SHARED: the candidates' values are in - audit, then the row is decided as after a second stage
__device__ __forceinline__ int minsdf_shared(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    const int c = (fl >> F_IT_SHIFT) & F_IT_MASK;
    shared_walk(P, r, r - (threadIdx.x & 63) + c, round, e, false);
    fl = with_win(fl, MW_ROW_IN) & ~(F_IT_MASK << F_IT_SHIFT);
    return PH_MINSDF_C;
}

// PH_MINSDF_C, MW_SECOND
__device__ __forceinline__ int minsdf_second_stage(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    // second stage of the two-stage refinement below: sample a (kept in the iteration bits) now holds its EXACT value
    // v*.  The exact argmin m has exact_m <= v*, hence coarse_m <= v* + tau: only such samples are refined; every other
    // one has exact > v* and keeps a coarse value > v* + tau - the exact stage's argmin over the mixed row is the
    // reference's (first index of the exact minimum).
    const int ns = P.p.n_steps;
    const float *v = P.s.big + (size_t)r * ns;
    const int a = (fl >> F_IT_SHIFT) & F_IT_MASK;
    const float lim = v[a] + P.tau;
    int k = 0;
    for (int i = 0; i < ns; ++i)
        if (i != a && v[i] <= lim) {
            e.mark(i);
            ++k;
        }
    fl = with_win(fl, MW_ROW_IN) & ~(F_IT_MASK << F_IT_SHIFT);
    if (k == 0) return PH_MINSDF;
    if (k <= P.cap) e.n_ref = k; else e.qd = true;
    e.dense_which = 1;
    fl = (fl & ~F_PHASE) | PH_MINSDF;
    P.s.flags[r] = fl;
    return PH_WAIT;
}

// PH_MINSDF_C, MW_ROW_IN
__device__ __forceinline__ int minsdf_coarse(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    // argmin over coarse values: every sample within 2 tau of the coarse minimum could be the exact one
    const int ns = P.p.n_steps;
    const float *v = P.s.big + (size_t)r * ns;
    float vmin = v[0];
    int amin = 0;
    for (int i = 1; i < ns; ++i)
        if (v[i] < vmin) {
            vmin = v[i];
            amin = i;
        }
    const float lim = vmin + 2.f * P.tau;
    int k = 0;
    for (int i = 0; i < ns; ++i)
        if (v[i] <= lim) {
            e.mark(i);
            ++k;
        }
    if (k <= 1) return PH_MINSDF;
    if ((P.window & 2) && k >= 4 && ns <= 256) {
        // two stages: the coarse argmin alone first - its exact value v* bounds the exact minimum from above, and the
        // second stage's window (coarse <= v* + tau) is about half of this one's (coarse <= coarse min + 2 tau)
        e.clear_marks();
        e.mark(amin);
        e.n_ref = 1;
        fl = (with_win(fl, MW_SECOND) & ~(F_IT_MASK << F_IT_SHIFT)) | (amin << F_IT_SHIFT);
    } else {
        if (k <= P.cap) e.n_ref = k; else e.qd = true;
        e.dense_which = 1;
        fl = (fl & ~F_PHASE) | PH_MINSDF;
    }
    P.s.flags[r] = fl;
    return PH_WAIT;
}

// A ray that certify_crossing ended: every depth of its min-SDF search lies on the certified chord [t_min, t_max].  Each value
// the row holds (single-pass or exact, within tau of exact; skipped depths are +inf) against both ends of its cell's interval,
// as grid_audit does - a certificate that leaned on a cell whose interval does not hold shows here, in the audit's counter
__device__ __forceinline__ void certify_audit(const Params &P, int64_t r, int round) {
    const int ns = P.p.n_steps;
    const float *v = P.s.big + (size_t)r * ns;
    const float tmin = P.s.t_min[r], len = fsub(P.s.t_max[r], tmin);
    float worst = 0.f;
    for (int i = 0; i < ns; ++i) {
        if (!(v[i] < __builtin_inff())) continue;
        float lo, hi;
        if (!grid_bounds(P, r, fadd(fmul(minsdf_step(P, r, i), len), tmin), lo, hi)) continue;
        worst = fmaxf(worst, fmaxf(fsub(fsub(lo, P.tau), v[i]), fsub(v[i], fadd(hi, P.tau))));
    }
    if (worst > 0.f) atomicMax(P.counters + round * NCNT + NEFII_CNT_LIP_AUDIT, __float_as_int(worst));
}

// PH_MINSDF: argmin over the depths (ray_tracing.py:309-337)
__device__ __forceinline__ int minsdf_exact(const Params &P, int64_t r, int round, int &fl, Emit &e) {
    const int ns = P.p.n_steps;
    const float *v = P.s.big + (size_t)r * ns;
    if ((fl & F_CERT) && P.cells) certify_audit(P, r, round);
    int amin = 0;
    float vmin = v[0];
    for (int i = 1; i < ns; ++i)
        if (v[i] < vmin) {
            vmin = v[i];
            amin = i;
        }
    const float tmin = P.s.t_min[r], tmax = P.s.t_max[r];
    const float dist = fadd(fmul(minsdf_step(P, r, amin), fsub(tmax, tmin)), tmin);
    finish(P, r, dist, fl & F_HIT);
    P.s.flags[r] = (fl & ~F_PHASE) | PH_DONE;
    return PH_WAIT;
}

__global__ __launch_bounds__(256) void advance_kernel(Params P, int round) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = r < P.n;
    // a block whose rays are all done has nothing to advance and nothing to append (late rounds - the bisection's - keep a
    // few percent of a big batch's rays: config 3 spent 3.4 ms per step in this kernel)
    if (round > 0 && P.s.block_live[blockIdx.x] == 0) return;
    Emit e = {};
    int fl = 0, fl0 = 0, ph = PH_WAIT, looks = 0;
    if (valid) {
        fl0 = fl = P.s.flags[r];
        ph = fl & F_PHASE;
        // in this order: a phase that has what it needs hands over to a later one in the same round
        if (round == 0) ph = init_ray(P, r, round, fl, e, looks);
        if (ph == PH_TRACE) ph = step_trace(P, r, round, fl, e, looks);
        if (ph == PH_SAMPLER_X) ph = sampler_leading(P, r, round, fl, e);
        if (ph == PH_SAMPLER_C && win_of(fl) >= SW_STAGE1) ph = sampler_staged(P, r, round, fl, e);
    }
    // the grid walks requested so far - all of them: end_trace, sampler_leading and sampler_staged lie above - by the whole
    // wave (every lane gets here); an audited row is read before post() can hand it to the min-SDF search
    if (P.walk_wave && P.cells) serve_grid_walks(P, r, round, fl, e);
    if (P.certify_free && P.cert_counts) {      // (every lane gets here) the rays ended as free this round, probes included, and the look-ups
        const unsigned long long cert = __ballot(valid && ph == PH_WAIT && (((fl & F_CERT) && (fl & F_PHASE) == PH_DONE && (fl0 & F_PHASE) != PH_DONE && !(fl0 & F_PROBE)) || ((fl & F_PROBE) && !(fl0 & F_PROBE))));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) looks += __shfl_xor(looks, o);
        if ((threadIdx.x & 63) == 0) {
            if (cert) atomicAdd(P.cert_counts + 2, __popcll(cert));
            if (looks > 0) atomicAdd(P.cert_counts + 3, looks);
        }
    }
    if (round == 0 && P.certify && P.cert_counts) {      // (every lane gets here) the wave's certified rays and block look-ups
        const unsigned long long cert = __ballot(valid && ph == PH_POST && (fl & F_CERT));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) looks += __shfl_xor(looks, o);
        if ((threadIdx.x & 63) == 0) {
            if (cert) atomicAdd(P.cert_counts, __popcll(cert));
            if (looks > 0) atomicAdd(P.cert_counts + 1, looks);
        }
    }
    if (valid) {
        if (ph == PH_SAMPLER_C && win_of(fl) != SW_WHOLE_ROW) ph = sampler_windows(P, r, round, fl, e);
        if (ph == PH_SAMPLER_C) ph = sampler_coarse(P, r, round, fl, e);
        if (ph == PH_SAMPLER) ph = sampler_exact(P, r, round, fl, e);
        if (ph == PH_BISECT) ph = bisect(P, r, round, fl, e);
        if (ph == PH_POST) ph = post(P, r, round, fl, e);
    }
    // (every lane gets here: lanes past the last ray hold PH_DONE and no F_OWN - they neither enter nor give)
    if (P.share) ph = minsdf_share(P, r, round, ph, fl0, fl, e);
    if (valid) {
        if (ph == PH_MINSDF_C && win_of(fl) == MW_SHARED) ph = minsdf_shared(P, r, round, fl, e);
        if (ph == PH_MINSDF_C && (win_of(fl) == MW_STAGE1 || win_of(fl) == MW_STAGE2)) ph = minsdf_staged(P, r, round, fl, e);
        if (ph == PH_MINSDF_C && win_of(fl) == MW_SECOND) ph = minsdf_second_stage(P, r, round, fl, e);
        if (ph == PH_MINSDF_C) ph = minsdf_coarse(P, r, round, fl, e);
        if (ph == PH_MINSDF) ph = minsdf_exact(P, r, round, fl, e);
    }
    append_queries(P, round, (unsigned)r, e);
    const int alive = __syncthreads_or(valid && (P.s.flags[r] & F_PHASE) != PH_DONE);
    if (threadIdx.x == 0) P.s.block_live[blockIdx.x] = alive;
}

// ---- SDF evaluation of one round's work list -------------------------------------------------
// queries of a round in split precision, in this order: singles | dense rays x n_steps | bisecting rays x tree nodes |
// refined coarse samples
struct RoundWork {
    int n_single;
    int64_t n_sd, n_sdt, total;
};
__device__ __forceinline__ RoundWork round_work(const Params &P, int round) {
    const int *c = P.counters + round * NCNT;
    RoundWork w;
    w.n_single = c[NEFII_CNT_SINGLES];
    w.n_sd = (int64_t)c[NEFII_CNT_SINGLES] + (int64_t)c[NEFII_CNT_DENSE_ROWS] * P.p.n_steps;
    w.n_sdt = w.n_sd + (int64_t)c[NEFII_CNT_BISECT_RAYS] * P.tri_nodes;
    w.total = w.n_sdt + c[NEFII_CNT_REFINED];
    return w;
}

// depth of dense sample i of ray r: the bracket search's linspace (ray_tracing.py:205) or the min-SDF search's uniform
// draws (:319); the one expression both the dense and the refine path use
__device__ __forceinline__ float dense_depth(const Params &P, int64_t r, int i, bool minsdf) {
    if (minsdf) {
        const float tmin = P.s.t_min[r], tmax = P.s.t_max[r];
        return fadd(fmul(minsdf_step(P, r, i), fsub(tmax, tmin)), tmin);
    }
    const float a = P.s.t_s[r];
    return fadd(a, fmul(P.lin[i], fsub(P.s.t_e[r], a)));
}

// the point of ray r at depth t
__device__ __forceinline__ float3 ray_point(const Params &P, int64_t r, float t) {
    return make_float3(fadd(P.o[r * 3], fmul(t, P.d[r * 3])), fadd(P.o[r * 3 + 1], fmul(t, P.d[r * 3 + 1])),
                       fadd(P.o[r * 3 + 2], fmul(t, P.d[r * 3 + 2])));
}

// row `tid` of a tile's raw[ROWS][9]: the point - the net's one encoded input; the other two stay zero
__device__ __forceinline__ void put_point(float *raw, int tid, float px, float py, float pz) {
    float *rw = raw + tid * 9;
    rw[0] = px, rw[1] = py, rw[2] = pz;
    rw[3] = rw[4] = rw[5] = rw[6] = rw[7] = rw[8] = 0.f;
}

// a tile of an explicit point list x[n][3] -> out[n] (nefii_sdf_eval*): rows past n are padding (dest = nullptr).  Writes its
// row itself: through put_point() the compiler splits the 12-byte load of the point into three.
template <int ROWS>
__device__ __forceinline__ void load_points_tile(const float *__restrict__ x, int64_t n, float *__restrict__ out, int64_t tile,
                                                 float *raw, float **dest, int tid = threadIdx.x) {
    if (tid >= ROWS) return;
    const int64_t q = tile * ROWS + tid;
    float *rw = raw + tid * 9;
    const bool live = q < n;
    rw[0] = live ? x[q * 3] : 0.f, rw[1] = live ? x[q * 3 + 1] : 0.f, rw[2] = live ? x[q * 3 + 2] : 0.f;
    rw[3] = rw[4] = rw[5] = rw[6] = rw[7] = rw[8] = 0.f;
    dest[tid] = live ? out + q : nullptr;
}

// decode the ROWS queries of a tile into points (raw[ROWS][9]) and result addresses (dest[ROWS])
// `old` (optional, [ROWS]): for a coarse-pass sample that is being re-evaluated, its coarse value (NaN for every other query) -
// the evaluator compares it with the split-precision value it is about to store (the online audit of coarse_tau)
template <int ROWS>
__device__ __forceinline__ void decode_tile(const Params &P, int64_t tile, const RoundWork &W, float *raw, float **dest,
                                            float *old = nullptr) {
    const int tid = threadIdx.x;
    if (tid >= ROWS) return;
    const int ns = P.p.n_steps;
    int64_t q = tile * ROWS + tid;
    float *dst = nullptr;
    float px = 0.f, py = 0.f, pz = 0.f;
    float coarse_v = __builtin_nanf("");
    if (q < W.total) {
        int64_t r;
        float t;
        if (q < W.n_single) {
            const unsigned e = P.s.singles[q];
            r = e >> 2;
            const int kind = e & 3;
            t = kind == Q_START ? P.s.t_s[r] : (kind == Q_END ? P.s.t_e[r] : P.s.mid[r]);
            dst = kind == Q_END ? &P.s.res_e[r] : &P.s.res_s[r];
            // a sphere-tracing query repeated in split precision: res_x still holds its coarse value
            if (old && P.tier_band > 0.f && (P.s.flags[r] & (kind == Q_END ? F_AUD_E : F_AUD_S))) coarse_v = *dst;
        } else if (q >= W.n_sdt) {
            const unsigned e = P.s.refine[q - W.n_sdt];
            r = e >> 7;
            const int i = e & 127;
            const int ph = P.s.flags[r] & F_PHASE;
            t = dense_depth(P, r, i, ph == PH_MINSDF || ph == PH_MINSDF_C);    // (_C: the first of the two refinement stages)
            dst = &P.s.big[(size_t)r * ns + i];
            if (old && ph != PH_SAMPLER_X) coarse_v = *dst;     // (the leading samples of a bracket search have no coarse value)
        } else if (q >= W.n_sd) {
            const int64_t qq = q - W.n_sd;
            const int64_t ti = qq / P.tri_nodes;
            const int j = (int)(qq - ti * P.tri_nodes);
            r = P.s.tri[ti];
            t = tri_depth(P.s.lo[r], P.s.hi[r], j);
            dst = &P.s.big[(size_t)r * ns + j];
        } else {
            const int64_t qq = q - W.n_single;
            const int64_t di = qq / ns;
            const int i = (int)(qq - di * ns);
            const unsigned e = P.s.dense[di];
            r = e >> 1;
            t = dense_depth(P, r, i, e & 1);
            dst = &P.s.big[(size_t)r * ns + i];
        }
        const float3 p = ray_point(P, r, t);
        px = p.x, py = p.y, pz = p.z;
    }
    dest[tid] = dst;
    if (old) old[tid] = coarse_v;
    put_point(raw, tid, px, py, pz);
}

// queries of a round's coarse list: n_rows samples of the (quarter) rows, then the tier's sphere-tracing queries, then the
// second stage's single depths; returns their sum
__device__ __forceinline__ int64_t coarse_work(const Params &P, int round, int64_t &n_rows) {
    const int *c = P.counters + round * NCNT;
    n_rows = (int64_t)c[NEFII_CNT_COARSE_WINDOWS] * coarse_window(P.p.n_steps);
    return n_rows + c[NEFII_CNT_COARSE_SINGLES] + c[NEFII_CNT_COARSE_SAMPLES];
}

// the same for the coarse evaluator's list: rays x n_steps samples
// queries [0, n_rows): the quarter rows' samples; [n_rows, total): the sphere-tracing queries of the tier (csingles)
template <int ROWS>
__device__ __forceinline__ void decode_tile_coarse(const Params &P, int round, int64_t tile, int64_t n_rows, int64_t total,
                                                   float *raw, float **dest, int tid = threadIdx.x) {
    if (tid >= ROWS) return;
    const int ns = P.p.n_steps, cw = coarse_window(ns);
    const int64_t q = tile * ROWS + tid;
    float *dst = nullptr;
    float px = 0.f, py = 0.f, pz = 0.f;
    const int64_t di = q / cw;
    const unsigned e = q < n_rows ? P.s.cdense[di] : 0u;
    int i = (int)(e >> 29) * cw + (int)(q - di * cw);
    if (q < n_rows && (e >> 29) == CWIN_STAGE1) {     // first stage of a staged min-SDF search: slot j -> sorted position -> sample
        const int j = (int)(q - di * cw);
        const int64_t rr = (e & 0x1FFFFFFFu) >> 1;
        i = j >= stage1_count(ns) ? ns : (e & 1) ? P.s.ord[(size_t)minsdf_row(P, rr) * ns + stage1_pos(ns, j)] : stage1_pos(ns, j);
    }
    const int64_t n_cs = P.counters[round * NCNT + NEFII_CNT_COARSE_SINGLES];
    if (q >= n_rows + n_cs && q < total) {            // second stage: single depths
        const unsigned s = P.s.crefine[q - n_rows - n_cs];
        const int64_t r = s >> 7;
        const int si = (int)(s & 127u);
        const float t = dense_depth(P, r, si, (P.s.flags[r] & F_PHASE) == PH_MINSDF_C);      // (else: a bracket search's sample)
        dst = &P.s.big[(size_t)r * ns + si];
        const float3 p = ray_point(P, r, t);
        px = p.x, py = p.y, pz = p.z;
    } else if (q >= n_rows && q < total) {
        const unsigned s = P.s.csingles[q - n_rows];
        const int64_t r = s >> 2;
        const bool end = (s & 3) == Q_END;
        const float t = end ? P.s.t_e[r] : P.s.t_s[r];
        dst = end ? &P.s.res_e[r] : &P.s.res_s[r];
        const float3 p = ray_point(P, r, t);
        px = p.x, py = p.y, pz = p.z;
    } else if (q < n_rows && i < ns) {
        const int64_t r = (e & 0x1FFFFFFFu) >> 1;
        const float t = dense_depth(P, r, i, e & 1);
        dst = &P.s.big[(size_t)r * ns + i];
        const float3 p = ray_point(P, r, t);
        px = p.x, py = p.y, pz = p.z;
    }
    dest[tid] = dst;
    put_point(raw, tid, px, py, pz);
}

__global__ __launch_bounds__(256, 1) void eval_kernel(Params P, nefii_mlp m, int round) {
    NEFII_CLAIM_SIMD_1();
    __shared__ Lds lds;
    __shared__ float raw[TILE * 9];
    __shared__ float *dest[TILE];
    const RoundWork W = round_work(P, round);
    const int64_t total = W.total;
    const int64_t n_tiles = (total + TILE - 1) / TILE;
    const int ke = max_ke(m);
    const int Lm1 = m.n_layers - 1;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        decode_tile<TILE>(P, tile, W, raw, dest);
        __syncthreads();
        encode_tile(m, raw, lds.E, ke);
        __syncthreads();
        for (int l = 0; l <= Lm1; ++l) {
            const nefii_layer &L = m.layer[l];
            f32x16 acc[4];
            int ntw;
            layer_gemm(L, lds.X, lds.E, L.w_fwd, L.n_pad >> 5, acc, ntw);
            __syncthreads();
            if (l < Lm1) {
                NEFII_ACT_SWITCH(m.act, { NEFII_FOR_ACC(acc, ntw, { lds.X[row * XS + col] = act_fwd(val + L.bias[col], ACT); }) })
            } else {
                NEFII_FOR_ACC(acc, ntw, {
                    if (col == 0 && dest[row]) *dest[row] = val + L.bias[0];
                })
            }
            __syncthreads();
        }
    }
}

// split-precision variant (3 x fp16 MFMA per k-step, mlp_tile.h)
__global__ __launch_bounds__(256, 1) void eval_kernel16(Params P, nefii_mlp m, int round) {    // 81 KB of LDS: one workgroup per CU anyway
    NEFII_CLAIM_SIMD_1();
    __shared__ Lds16 lds;
    __shared__ float raw[TILE * 9];
    __shared__ float *dest[TILE];
    const RoundWork W = round_work(P, round);
    const int64_t total = W.total;
    const int64_t n_tiles = (total + TILE - 1) / TILE;
    const int ke = max_ke(m);
    const int Lm1 = m.n_layers - 1;
    const float inv_scale = 1.f / (W16_SCALE * A16_SCALE);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        decode_tile<TILE>(P, tile, W, raw, dest);
        __syncthreads();
        encode_tile16(m, raw, lds, ke);
        __syncthreads();
        for (int l = 0; l <= Lm1; ++l) {
            const nefii_layer &L = m.layer[l];
            f32x16 acc[4];
            int ntw;
            layer_gemm16(L, lds, L.n_pad >> 5, acc, ntw);
            __syncthreads();
            if (l < Lm1) {
                NEFII_ACT_SWITCH(m.act, {
                    NEFII_FOR_ACC(acc, ntw, {
                        const float hval = act_fwd(val * inv_scale + L.bias[col], ACT);
                        split16a(hval, lds.Xh[row * XS16 + col], lds.Xl[row * XS16 + col]);
                    })
                })
            } else {
                NEFII_FOR_ACC(acc, ntw, {
                    if (col == 0 && dest[row]) *dest[row] = val * inv_scale + L.bias[0];
                })
            }
            __syncthreads();
        }
    }
}

// wide split-precision variant: 64 queries per workgroup of 8 waves (mlp_tile.h, Lds16w)
// One tile: raw[64][9] holds the points, dest[64] where each SDF value goes (nullptr = padding row).
__device__ __forceinline__ void sdf_tile16w(const nefii_mlp &m, Lds16w &lds, const float *raw, float *const *dest,
                                            int ke) {
    const int Lm1 = m.n_layers - 1;
    const float inv_scale = 1.f / (W16_SCALE * A16_SCALE);
    encode_tile16w(m, raw, lds, ke);
    __syncthreads();
    for (int l = 0; l <= Lm1; ++l) {
        const nefii_layer &L = m.layer[l];
        f32x16 acc[4];
        int nct;
        layer_gemm16w(L, lds, L.n_pad >> 5, acc, nct);
        __syncthreads();
        if (l < Lm1) {
            const float k16 = inv_scale * A16_SCALE;
            NEFII_ACT_SWITCH(m.act, {
                NEFII_FOR_ACC_WT(acc, nct, L.n_pad >> 5, {
                    const float4v b = *reinterpret_cast<const float4v *>(L.bias + f0);
                    float4v hs;       // A16_SCALE * activation
                    _Pragma("unroll") for (int k = 0; k < 4; ++k) {
                        const float zs = __builtin_fmaf(v[k], k16, b[k] * A16_SCALE);
                        hs[k] = ACT == NEFII_ACT_SOFTPLUS100 ? softplus100_s16(zs)
                                                             : act_fwd(zs * (1.f / A16_SCALE), ACT) * A16_SCALE;
                    }
                    const half4 hi = __builtin_convertvector(hs, half4);
                    const half4 lo = __builtin_convertvector(hs - __builtin_convertvector(hi, float4v), half4);
                    *reinterpret_cast<half4 *>(&lds.Xh[query * XS16 + f0]) = hi;
                    *reinterpret_cast<half4 *>(&lds.Xl[query * XS16 + f0]) = lo;
                })
            })
        } else {
            NEFII_FOR_ACC_WT(acc, nct, L.n_pad >> 5, {
                if (f0 == 0 && dest[query]) *dest[query] = v[0] * inv_scale + L.bias[0];
            })
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(512, 2) void eval_kernel16w(Params P, nefii_mlp m, int round) {
    NEFII_CLAIM_SIMD_2();
    __shared__ Lds16w lds;
    __shared__ float raw[TILE_W * 9];
    __shared__ float *dest[TILE_W];
    const RoundWork W = round_work(P, round);
    const int64_t total = W.total;
    const int64_t n_tiles = (total + TILE_W - 1) / TILE_W;
    const int ke = max_ke(m);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        decode_tile<TILE_W>(P, tile, W, raw, dest);
        __syncthreads();
        sdf_tile16w(m, lds, raw, dest, ke);
    }
}

// pipelined variant (mlp_tile.h "16p"): 512-wide hidden layers, fragment stream never drains.
// Two instantiations are launched per round and the round's query count (known on the device only) picks the one that
// works: RT = 2 (64-query tiles) for rounds of more than SMALL_ROUND queries, RT = 1 (32-query tiles) for the others - a
// round with fewer 64-query tiles than half the CUs puts twice as many CUs to work on tiles with half the matrix work
// and epilogue (the fragment stream per tile is the same: ~110 instead of ~150 us per round).  Kept as two kernels:
// fused into one, the register allocation of the 64-query path degraded (60 spills, dense rounds +25 %).
constexpr int64_t SMALL_ROUND = 64 * 128;
// nefii_tracer_params.small_round overrides the threshold: a trace that runs beside others is bound by chip time, not by
// its own latency, and a 32-query tile costs 1.5x the chip time per query of a 64-query one
__device__ __forceinline__ int64_t small_round(const Params &P) { return P.p.small_round > 0 ? P.p.small_round : SMALL_ROUND; }
template <int NW, int RT>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 1 : 2) void eval_kernel16p(Params P, nefii_mlp m, int round) {
    static_assert(NW == 8, "register claim below: two waves per SIMD");
    NEFII_CLAIM_SIMD_2();
    __shared__ Lds16p lds;
    __shared__ float raw[TILE_W * 9];
    __shared__ float *dest[TILE_W];
    const RoundWork W = round_work(P, round);
    const int64_t total = W.total;
    if ((total <= small_round(P)) != (RT == 1)) return;
    constexpr int ROWS = 32 * RT;
    const int64_t n_tiles = (total + ROWS - 1) / ROWS;
    if (blockIdx.x >= n_tiles) return;
    const int ke = max_ke(m);
    typename P16<NW>::Stage b[P16<NW>::NB];
    PCursor cur;
    int ph = 0;
    prime16p<NW>(m, b, cur);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        decode_tile<ROWS>(P, tile, W, raw, dest);
        __syncthreads();
        sdf_tile16p<NW, RT>(m, lds, raw, dest, b, cur, ph, ke);
    }
}

// a padded fragment stream (the deep-prefetch instance's, "16f"'s, the single-pass one) multiplies whatever follows a layer's
// own K columns in the activation image (the row's pad columns, the next row, `tail`) by zero weights: all of it must be
// finite from the first tile on
template <typename LDS>
__device__ __forceinline__ void zero_lds(LDS &lds) {
    uint32_t *p = reinterpret_cast<uint32_t *>(&lds);
    for (int i = threadIdx.x; i < (int)(sizeof(LDS) / 4); i += blockDim.x) p[i] = 0u;
    __syncthreads();
}

// Which of the two per-round instances (QT == 2: 32-query tiles; else BIG-query tiles) takes which queries.  Rounds up to
// SMALL_ROUND: all in 32-query tiles.  Larger rounds: big tiles (64 / 96 queries); when the big tiles form whole waves of
// one tile per CU plus a remainder that fits one wave of 32-query tiles, that remainder goes to the 32-query instance (a
// wave of those is done in ~110 instead of ~160 us).
// This instance's tiles: first .. first + n_tiles - 1, 16 QT queries each.
template <int QT, int BIG>
__device__ __forceinline__ void split_round(int64_t total, int64_t small, int64_t &first_out, int64_t &n_tiles_out) {
    constexpr int NCU = 256;
    int64_t first = 0, n_tiles;       // (assigned to the references once, at the end: the scalar registers stay the inline form's)
    if (total <= small) {
        n_tiles = QT == 2 ? (total + 31) / 32 : 0;
    } else {
        const int64_t nbig = (total + BIG - 1) / BIG, whole = nbig / NCU * NCU, rem = nbig - whole;
        const bool split = whole > 0 && rem > 0 && rem * (BIG / 32) <= NCU;
        if (QT == 2) {
            first = split ? whole * (BIG / 32) : 0;
            n_tiles = split ? (total - whole * BIG + 31) / 32 : 0;
        } else {
            n_tiles = split ? whole : nbig;
        }
    }
    first_out = first, n_tiles_out = n_tiles;
}

// the same on v_mfma_f32_16x16x32_f16 (mlp_tile.h "16q"; nefii_mlp.reserved == 1).  FT = 4: 512-wide hidden layers,
// 64- / 32-query tiles; FT = 2: 256-wide hidden layers (conf_neus.conf), 96- / 32-query tiles.
template <int QT, int FT, bool DEEP = false>
__global__ __launch_bounds__(512, 2) void eval_kernel16q(Params P, nefii_mlp m, int round) {
    NEFII_CLAIM_SIMD_2();
    constexpr int RMAX = QGeo<FT>::ROWS;
    __shared__ LdsQ<FT> lds;
    __shared__ float raw[RMAX * 9];
    __shared__ float *dest[RMAX];
    __shared__ float old[RMAX];
    const RoundWork W = round_work(P, round);
    const int64_t total = W.total;
    constexpr int ROWS = 16 * QT;
    int64_t first, n_tiles;
    split_round<QT, QGeo<FT>::ROWS>(total, small_round(P), first, n_tiles);
    if (blockIdx.x >= n_tiles) return;
    // DEEP: 8 fragment stages instead of 4 for the 32-query instance of the 512-wide shape.  It pays when few CUs stream
    // (batches of <= 1024 rays: <= 64 tiles per round, each bound by the latency of its own 7.6 MB stream - config 1:
    // 2.49 -> 2.17 ms per step); with every CU streaming the tiles are bound by L2 bandwidth instead and the deeper
    // pipeline only adds its priming (config 2's small rounds: 104 -> 110 us), so the host picks it by batch size.
    constexpr int NB = DEEP ? 8 : 4;
    static_assert(!DEEP || (QT == 2 && FT == 4), "deep prefetch: the 32-query instance of the 512-wide shape");
    if (NB == 8) zero_lds(lds);
    P16<8>::Stage b[NB];
    PCursor cur;
    prime16q<FT, NB>(m, b, cur);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const bool audit = P.tau > 0.f;
        decode_tile<ROWS>(P, first + tile, W, raw, dest, audit ? old : nullptr);
        __syncthreads();
        sdf_tile16q<QT, FT, NB>(m, lds, raw, dest, b, cur, audit ? old : nullptr, P.counters + round * NCNT + NEFII_CNT_TAU_AUDIT);
    }
}

// "16f" (mlp_tile.h, nefii_tracer_params.split_fp8): the same work lists and tile shapes as eval_kernel16q<QT, 4>, the correction
// products on block-scaled fp8; f8_stream = the fifth copy of nefii_mlp.w_stream
template <int QT>
__global__ __launch_bounds__(512, 2) void eval_kernel16f(Params P, nefii_mlp m, int round, const void *f8_stream) {
    NEFII_CLAIM_SIMD_2();
    constexpr int RMAX = QGeo<4>::ROWS;
    __shared__ LdsF lds;
    __shared__ float raw[RMAX * 9];
    __shared__ float *dest[RMAX];
    __shared__ float old[RMAX];
    const RoundWork W = round_work(P, round);
    const int64_t total = W.total;
    constexpr int ROWS = 16 * QT;
    int64_t first, n_tiles;
    split_round<QT, RMAX>(total, small_round(P), first, n_tiles);
    if (blockIdx.x >= n_tiles) return;
    zero_lds(lds);        // the 128-padded stream multiplies what follows a layer's own columns by zero weights: keep it finite
    SStage<4> b[4];
    PCursor cur;
    prime16f(m, f8_stream, b, cur);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const bool audit = P.tau > 0.f;
        decode_tile<ROWS>(P, first + tile, W, raw, dest, audit ? old : nullptr);
        __syncthreads();
        sdf_tile16f<QT>(m, lds, raw, dest, b, cur, audit ? old : nullptr, P.counters + round * NCNT + NEFII_CNT_TAU_AUDIT);
    }
}

__global__ __launch_bounds__(512, 2) void sdf_points_kernel16f(nefii_mlp m, const float *__restrict__ x, int64_t n,
                                                              float *__restrict__ out, const void *f8_stream) {
    NEFII_CLAIM_SIMD_2();
    constexpr int ROWS = QGeo<4>::ROWS, QT = ROWS / 16;
    __shared__ LdsF lds;
    __shared__ float raw[ROWS * 9];
    __shared__ float *dest[ROWS];
    const int64_t n_tiles = (n + ROWS - 1) / ROWS;
    zero_lds(lds);
    SStage<4> b[4];
    PCursor cur;
    prime16f(m, f8_stream, b, cur);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        load_points_tile<ROWS>(x, n, out, tile, raw, dest);
        __syncthreads();
        sdf_tile16f<QT>(m, lds, raw, dest, b, cur);
    }
}

// the coarse evaluator (mlp_tile.h "16s") over the round's coarse list: one fp16 pass, 16 * QT queries per tile
// DB (the 64- / 96-row default tiles): two activation images, one barrier per layer (mlp_tile.h, sdf_tile16s2)
template <int FT, int ROWS, bool DB>
using LdsSx = typename std::conditional<DB, LdsS2<FT, ROWS>, LdsS<FT, ROWS>>::type;

template <int QT, int FT, bool DB = true>
__global__ __launch_bounds__(512, 2) void eval_kernel16s(Params P, nefii_mlp m, int round) {
    NEFII_CLAIM_SIMD_2();
    constexpr int ROWS = 16 * QT, RMAX = ROWS;
    __shared__ LdsSx<FT, ROWS, DB> lds;
    __shared__ float raw[RMAX * 9];
    __shared__ float *dest[RMAX];
    int64_t n_rows;
    const int64_t total = coarse_work(P, round, n_rows);
    const int64_t n_tiles = (total + ROWS - 1) / ROWS;
    if (blockIdx.x >= n_tiles) return;
    zero_lds(lds);      // the K-padded stream multiplies what follows a layer's own columns by zero weights: keep it finite
    SStage<FT> b[4];
    PCursor cur;
    prime16s<FT>(m, b, cur);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        decode_tile_coarse<ROWS>(P, round, tile, n_rows, total, raw, dest);
        __syncthreads();
        if constexpr (DB)
            sdf_tile16s2<QT, FT>(m, lds, raw, dest, b, cur);
        else
            sdf_tile16s<QT, FT>(m, lds, raw, dest, b, cur);
    }
}

template <int QT, int FT, bool DB = true>
__global__ __launch_bounds__(512, 2) void sdf_points_kernel16s(nefii_mlp m, const float *__restrict__ x, int64_t n,
                                                              float *__restrict__ out) {
    NEFII_CLAIM_SIMD_2();
    constexpr int ROWS = 16 * QT, RMAX = ROWS;
    __shared__ LdsSx<FT, ROWS, DB> lds;
    __shared__ float raw[RMAX * 9];
    __shared__ float *dest[RMAX];
    const int64_t n_tiles = (n + ROWS - 1) / ROWS;
    zero_lds(lds);
    SStage<FT> b[4];
    PCursor cur;
    prime16s<FT>(m, b, cur);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        load_points_tile<ROWS>(x, n, out, tile, raw, dest);
        __syncthreads();
        if constexpr (DB)
            sdf_tile16s2<QT, FT>(m, lds, raw, dest, b, cur);
        else
            sdf_tile16s<QT, FT>(m, lds, raw, dest, b, cur);
#ifdef NEFII_STAMPS
        if (blockIdx.x == 0 && threadIdx.x == 0) g_stamp_tile = g_stamp_tile + 1;
        __syncthreads();
#endif
    }
}

// "16d" (mlp_tile.h): the single-pass tile on four waves; a workgroup is two independent four-wave groups, each a persistent
// worker over its own tiles (tile = 2 x workgroup + group, stride 2 x grid), image, decode buffers and barrier counter
template <int QT>
__global__ __launch_bounds__(512, 2) void eval_kernel16d(Params P, nefii_mlp m, int round) {
    NEFII_CLAIM_SIMD_2();
    constexpr int ROWS = 16 * QT;
    __shared__ LdsS2<4, ROWS> lds;
    __shared__ float raw[2 * ROWS * 9];
    __shared__ float *dest[2 * ROWS];
    __shared__ unsigned bar[3];
    int64_t n_rows;
    const int64_t total = coarse_work(P, round, n_rows);
    const int64_t n_tiles = (total + ROWS - 1) / ROWS;
    if (blockIdx.x >= n_tiles) return;
    if (threadIdx.x < 3) bar[threadIdx.x] = 0u;
    zero_lds(lds);      // (ends with the one workgroup barrier of this kernel)
    const int g = threadIdx.x >> 8;
    // group 0 takes tiles [0, grid), group 1 [grid, 2 grid), ...: a round of no more tiles than workgroups runs one group per CU
    if (blockIdx.x + g * (int64_t)gridDim.x < n_tiles) {
        GroupBarrier gb(&bar[g]);
        SStage<4> b[4];
        PCursor cur[2];
        prime16d<QT>(m, b, cur);
        for (int64_t tile = blockIdx.x + g * (int64_t)gridDim.x; tile < n_tiles; tile += 2 * (int64_t)gridDim.x) {
            decode_tile_coarse<ROWS>(P, round, tile, n_rows, total, raw + g * ROWS * 9, dest + g * ROWS, threadIdx.x & 255);
            gb.sync();
            sdf_tile16d<QT>(m, lds.X[g], raw + g * ROWS * 9, dest + g * ROWS, b, cur, gb);
        }
    }
    GroupBarrier::hold(&bar[2]);
}

template <int QT>
__global__ __launch_bounds__(512, 2) void sdf_points_kernel16d(nefii_mlp m, const float *__restrict__ x, int64_t n,
                                                              float *__restrict__ out) {
    NEFII_CLAIM_SIMD_2();
    constexpr int ROWS = 16 * QT;
    __shared__ LdsS2<4, ROWS> lds;
    __shared__ float raw[2 * ROWS * 9];
    __shared__ float *dest[2 * ROWS];
    __shared__ unsigned bar[3];
    const int64_t n_tiles = (n + ROWS - 1) / ROWS;
    if (threadIdx.x < 3) bar[threadIdx.x] = 0u;
    zero_lds(lds);
    const int g = threadIdx.x >> 8, tl = threadIdx.x & 255;
    if (blockIdx.x + g * (int64_t)gridDim.x >= n_tiles) {
        GroupBarrier::hold(&bar[2]);
        return;
    }
    GroupBarrier gb(&bar[g]);
    SStage<4> b[4];
    PCursor cur[2];
    prime16d<QT>(m, b, cur);
#ifdef NEFII_STAMPS
    if (tl == 0 && blockIdx.x < 256) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_dhwid[2 * (2 * blockIdx.x + g)] = hw, g_dhwid[2 * (2 * blockIdx.x + g) + 1] = xcc;
    }
#endif
    int seq = 0;
    float *rawg = raw + g * ROWS * 9;
    float **destg = dest + g * ROWS;
    for (int64_t tile = blockIdx.x + g * (int64_t)gridDim.x; tile < n_tiles; tile += 2 * (int64_t)gridDim.x, ++seq) {
        load_points_tile<ROWS>(x, n, out, tile, rawg, destg, tl);
        gb.sync();
        sdf_tile16d<QT>(m, lds.X[g], rawg, destg, b, cur, gb, seq);
    }
    GroupBarrier::hold(&bar[2]);
}

template <int FT>
__global__ __launch_bounds__(512, 2) void sdf_points_kernel16q(nefii_mlp m, const float *__restrict__ x, int64_t n,
                                                              float *__restrict__ out) {
    NEFII_CLAIM_SIMD_2();
    constexpr int ROWS = QGeo<FT>::ROWS, QT = ROWS / 16;
    __shared__ LdsQ<FT> lds;
    __shared__ float raw[ROWS * 9];
    __shared__ float *dest[ROWS];
    const int64_t n_tiles = (n + ROWS - 1) / ROWS;
    P16<8>::Stage b[4];
    PCursor cur;
    prime16q<FT>(m, b, cur);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        load_points_tile<ROWS>(x, n, out, tile, raw, dest);
        __syncthreads();
        sdf_tile16q<QT, FT>(m, lds, raw, dest, b, cur);
    }
}

template <int NW>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 1 : 2) void sdf_points_kernel16p(nefii_mlp m,
                                                                                const float *__restrict__ x,
                                                                                int64_t n, float *__restrict__ out) {
    NEFII_CLAIM_SIMD_2();
    __shared__ Lds16p lds;
    __shared__ float raw[TILE_W * 9];
    __shared__ float *dest[TILE_W];
    const int64_t n_tiles = (n + TILE_W - 1) / TILE_W;
    const int ke = max_ke(m);
    typename P16<NW>::Stage b[P16<NW>::NB];
    PCursor cur;
    int ph = 0;
    prime16p<NW>(m, b, cur);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        load_points_tile<TILE_W>(x, n, out, tile, raw, dest);
        __syncthreads();
        sdf_tile16p<NW, 2>(m, lds, raw, dest, b, cur, ph, ke);
#ifdef NEFII_STAMPS
        if (blockIdx.x == 0 && threadIdx.x == 0) g_stamp_tile = g_stamp_tile + 1;
        __syncthreads();
#endif
    }
}

#ifdef NEFII_STAMPS
extern "C" int nefii_debug_dstamps(unsigned long long *host_out, unsigned *hwid_out) {
    hipError_t e = hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_dstamps), sizeof(unsigned long long) * 512 * 12 * 5);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpyFromSymbol(hwid_out, HIP_SYMBOL(g_dhwid), sizeof(unsigned) * 1024);
    return (int)e;
}
extern "C" int nefii_debug_stamps(unsigned long long *host_out) {
    int zero = 0;
    hipError_t e = hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 2 * 8 * 12 * 5);
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_tile), &zero, sizeof(int));
    return (int)e;
}
#endif

constexpr int P16W = 8;      // waves per workgroup of the pipelined kernels

// ================================================================================================
// SDF value + last-hidden features + input gradient (normals) of a point list on the fragment stream: get_rbg_value's
// implicit_network(x) + gradient(x) (reference implicit_differentiable_renderer.py:85-104,533-540) for the nets
// vg_shape() takes; the generic 32-row kernel (nefii_mlp.hip) spends ~1 ms per tile on the same work.
// One workgroup of 8 waves per CU, 16 QT rows per tile:
//   forward  - the "16q" evaluator (mlp_tile.h), its epilogue also stashing 16 h_l (fp32, the accumulator layout: one
//              coalesced 16-byte store per lane and feature-tile x query-tile) in the workgroup's own workspace slot;
//   backward - gz_{NH-1} = w_last * sigma'(h_{NH-1}); then per layer l = NH-1 .. 1 the SAME k-loop over the transposed
//              layer's units (contraction over the layer's outputs, gz_l as the LDS image) and an epilogue that
//              multiplies by sigma'(h_{l-1}) from the stash; the encoding columns' gradient of the skip layer and of
//              layer 0 comes from a 32x32x16 side GEMM of waves 0-3 over the layer's own transposed fragments, kept
//              as fp32 in the LDS image's (free by then) encoding columns; last the chain through the encoding.
// ================================================================================================
template <int FT>
__device__ __forceinline__ float *vg_ge_row(LdsQ<FT> &lds, int te, int row) {
    return reinterpret_cast<float *>((te ? lds.Xl : lds.Xh) + row * QGeo<FT>::XP + QGeo<FT>::HW);
}

// GE[row][32 te ..] += gz_l[row][:] . W_l[:, encoding columns 32 te ..] for the layer's two encoding tiles; one wave per
// (encoding tile, 32-row tile): waves 0..3 (64-row tiles) / 0..5 (96-row tiles)
template <int QT, int FT>
__device__ __forceinline__ void vg_enc_grad(const nefii_layer &L, LdsQ<FT> &lds, int wave, int lane, float inv_scale) {
    static_assert(QT % 2 == 0 && QT <= 8, "whole 32-row tiles, one wave each");
    constexpr int XP = QGeo<FT>::XP, EP = QGeo<FT>::HW;
    if (wave >= QT) return;
    const int te = wave & 1, rt = wave >> 1;
    const int r = lane & 31, h = lane >> 5;
    const int KT = (L.k_x + L.k_e) >> 5, t = (L.k_x >> 5) + te, S = L.n_pad >> 4;
    const half8 *wb = reinterpret_cast<const half8 *>(L.w_bwd_f16x3) + ((size_t)t * 2) * 64 + lane;
    const _Float16 *ah = lds.Xh + (32 * rt + r) * XP + 8 * h + (EP - L.n_pad);
    const _Float16 *al = lds.Xl + (32 * rt + r) * XP + 8 * h + (EP - L.n_pad);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int s0 = 0; s0 < S; s0 += 4) {        // S = 32: four 16-deep steps per trip, their fragment loads issued together
        half8 wh[4], wl[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) wh[u] = wb[(size_t)(s0 + u) * KT * 128], wl[u] = wb[(size_t)(s0 + u) * KT * 128 + 64];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const half8 xh = *reinterpret_cast<const half8 *>(ah + 16 * (s0 + u));
            const half8 xl = *reinterpret_cast<const half8 *>(al + 16 * (s0 + u));
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[u], xh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[u], xh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[u], xl, acc, 0, 0, 0);
        }
    }
    float *ge = vg_ge_row<FT>(lds, te, 32 * rt + r);       // this lane owns its 16 slots of the row: plain read-modify-write
#pragma unroll
    for (int i = 0; i < 16; ++i) ge[(i & 3) + 8 * (i >> 2) + 4 * h] += acc[i] * inv_scale;
}

template <int QT, int FT>
__global__ __launch_bounds__(512, 2) void sdf_value_grad16q_kernel(nefii_mlp m, const float *__restrict__ x, int64_t n,
                                                                  float *__restrict__ sdf_out, int out_stride,
                                                                  float *__restrict__ feat_out, int feat_stride,
                                                                  float *__restrict__ grad_out, float4v *__restrict__ ws,
                                                                  size_t vg_off, int Gw) {
    NEFII_CLAIM_SIMD_2();
    constexpr int ROWS = 16 * QT, NW = 8, RT = QT / 2, XP = QGeo<FT>::XP, EP = QGeo<FT>::HW, NJ = FT * QT;
    static_assert(ROWS <= QGeo<FT>::ROWS, "rows of the LDS image");
    __shared__ LdsQ<FT> lds;
    __shared__ float raw[ROWS * 9];
    __shared__ float psum[NW * ROWS];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int NH = m.n_layers - 1;
    const float inv_scale = 1.f / (W16_SCALE * A16_SCALE), k16 = inv_scale * A16_SCALE;
    const int64_t n_tiles = (n + ROWS - 1) / ROWS;
    // stash element (layer l, accumulator j) of this lane: stash[(l * NW * NJ + j) * 64]
    float4v *stash = ws + ((size_t)blockIdx.x * NH * NW + wave) * NJ * 64 + lane;
    constexpr size_t SL = (size_t)NW * NJ * 64;             // float4 per layer
    P16<8>::Stage b[4];
    PCursor cur;
    cur.bytes = (unsigned)Gw * 4096;
    cur.base = reinterpret_cast<const half8 *>(m.w_stream) + vg_off + (size_t)wave * Gw * 256 + lane;
    cur.off = 0;
#pragma unroll
    for (int u = 0; u < 3; ++u) pload<8>(b[u], cur);
    const int boff = 16 * FT * wave + (lane & (16 * FT - 1));
    const _Float16 *qh0 = lds.Xh + (lane & 15) * XP + 8 * (lane >> 4), *ql0 = lds.Xl + (lane & 15) * XP + 8 * (lane >> 4);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = tile * ROWS;
        for (int i = tid; i < ROWS * 9; i += 512) {
            const int p = i / 9, c = i - 9 * p;
            int64_t idx = base + p;
            if (idx >= n) idx = n - 1;
            raw[i] = c < 3 ? x[idx * 3 + c] : 0.f;
        }
        float bnext = m.layer[0].bias[boff];
        __syncthreads();
        encode_tile16q<FT>(m, raw, lds, ROWS);
        __syncthreads();
        // ------------------------------------------------ forward
        for (int l = 0; l < NH; ++l) {
            const nefii_layer &L = m.layer[l];
            const int units = q_units<FT>(L);
            const _Float16 *ah = qh0 + (EP - L.k_x), *al = ql0 + (EP - L.k_x);
            const float *bp = m.layer[l + 1 < NH ? l + 1 : l].bias + boff;
            asm volatile("" ::"s"(units), "v"(ah), "v"(al), "v"(bp));
            __builtin_amdgcn_s_waitcnt(0x0070);
            __builtin_amdgcn_sched_barrier(0);
            const float bvec = bnext;
            f32x4 acc[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j][i] = 0.f;
            QAct<QT> a[2];
            qload_a<QT, XP>(a[0], ah, al, 0);
            qgemm<QT, FT>(units, b, a, cur, ah, al, acc);
            bnext = *bp;
            __builtin_amdgcn_sched_barrier(0);
            half4 phi[NJ], plo[NJ];
            const int bsrc = __builtin_bit_cast(int, bvec * A16_SCALE);
            float4v *st = stash + (size_t)l * SL;
            const bool feat = feat_out != nullptr && l == NH - 1;
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) {
                float4v bs;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    bs[k] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(4 * (16 * ft + 4 * (lane >> 4) + k), bsrc));
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    const int j = ft * QT + qt;
                    float4v hs;
#pragma unroll
                    for (int k = 0; k < 4; ++k) hs[k] = softplus100_s16(__builtin_fmaf(acc[j][k], k16, bs[k]));
                    st[j * 64] = hs;
                    const half4 hi = __builtin_convertvector(hs, half4);
                    phi[j] = hi;
                    plo[j] = __builtin_convertvector(hs - __builtin_convertvector(hi, float4v), half4);
                    if (feat) {
                        const int64_t row = base + 16 * qt + (lane & 15);
                        const int f0 = 16 * FT * wave + 16 * ft + 4 * (lane >> 4);
                        if (row < n) {
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                if (f0 + k < L.n_out) feat_out[(size_t)row * feat_stride + f0 + k] = hs[k] * (1.f / A16_SCALE);
                        }
                    }
                }
            }
            __syncthreads();
            _Float16 *xh = lds.Xh + (EP - L.n_pad), *xl = lds.Xl + (EP - L.n_pad);
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) {
                const int f0 = 16 * FT * wave + 16 * ft + 4 * (lane >> 4);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    const int query = 16 * qt + (lane & 15);
                    *reinterpret_cast<half4 *>(xh + query * XP + f0) = phi[ft * QT + qt];
                    *reinterpret_cast<half4 *>(xl + query * XP + f0) = plo[ft * QT + qt];
                }
            }
            __syncthreads();
        }
        // last layer: 32x32x16 fragments of the layer's own w_f16x3.  One column (use_last_as_f nets): K split over the
        // waves (as in "16q"); a wide one (SDF + feature columns): whole (column tile, row tile) products per wave.
        if (m.layer[NH].n_pad > 32) {
            const int r = lane & 31, h = lane >> 5;
            const nefii_layer &L = m.layer[NH];
            const int NT = L.n_pad >> 5, S = L.k_x >> 4;
            const half8 *wl = reinterpret_cast<const half8 *>(L.w_f16x3) + lane;
            for (int c = wave; c < NT * RT; c += NW) {
                const int t = c / RT, rt = c - t * RT;
                const _Float16 *ah = lds.Xh + (32 * rt + r) * XP + 8 * h + (EP - L.k_x);
                const _Float16 *al = lds.Xl + (32 * rt + r) * XP + 8 * h + (EP - L.k_x);
                f32x16 acc2;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc2[i] = 0.f;
                for (int s0 = 0; s0 < S; s0 += 4) {
                    half8 wh[4], wlo[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        wh[u] = wl[((size_t)(s0 + u) * NT + t) * 128], wlo[u] = wl[((size_t)(s0 + u) * NT + t) * 128 + 64];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const half8 xh8 = *reinterpret_cast<const half8 *>(ah + 16 * (s0 + u));
                        const half8 xl8 = *reinterpret_cast<const half8 *>(al + 16 * (s0 + u));
                        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[u], xh8, acc2, 0, 0, 0);
                        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wlo[u], xh8, acc2, 0, 0, 0);
                        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[u], xl8, acc2, 0, 0, 0);
                    }
                }
                const int64_t row = base + 32 * rt + r;
                if (row < n) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int f = 32 * t + (i & 3) + 8 * (i >> 2) + 4 * h;
                        if (f < L.n_out) sdf_out[(size_t)row * out_stride + f] = acc2[i] * inv_scale + L.bias[f];
                    }
                }
            }
            __syncthreads();        // every wave is done reading h_{NH-1} from the image
        } else {
            const int r = lane & 31, h = lane >> 5;
            const nefii_layer &L = m.layer[NH];
            const int NT = L.n_pad >> 5;
            const half8 *wl = reinterpret_cast<const half8 *>(L.w_f16x3) + lane;
            const _Float16 *ah = lds.Xh + r * XP + 8 * h + (EP - L.k_x), *al = lds.Xl + r * XP + 8 * h + (EP - L.k_x);
            const int ksw = (L.k_x >> 4) / NW;
            f32x16 acc2[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc2[rt][i] = 0.f;
            for (int u = 0; u < ksw; ++u) {
                const int s = wave * ksw + u;
                const half8 wh = wl[(size_t)s * NT * 128], wlo = wl[(size_t)s * NT * 128 + 64];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const half8 xh8 = *reinterpret_cast<const half8 *>(ah + rt * 32 * XP + 16 * s);
                    const half8 xl8 = *reinterpret_cast<const half8 *>(al + rt * 32 * XP + 16 * s);
                    acc2[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh8, acc2[rt], 0, 0, 0);
                    acc2[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wlo, xh8, acc2[rt], 0, 0, 0);
                    acc2[rt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xl8, acc2[rt], 0, 0, 0);
                }
            }
            if (h == 0) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) psum[wave * ROWS + 32 * rt + r] = acc2[rt][0];
            }
            __syncthreads();        // partial sums complete; every wave is done reading h_{NH-1} from the image
            if (tid < ROWS) {
                float sum = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) sum += psum[w * ROWS + tid];
                if (base + tid < n) sdf_out[(size_t)(base + tid) * out_stride] = sum * inv_scale + L.bias[0];
            }
        }
        // ------------------------------------------------ backward
        // seed: gz_{NH-1}[row][f] = W_last[0][f] * sigma'(h_{NH-1}[row][f]); the encoding columns become the fp32 GE rows
        {
            const nefii_layer &LL = m.layer[NH];
            const half8 *wlb = reinterpret_cast<const half8 *>(LL.w_bwd_f16x3);       // s16 = 0: outputs 0..7 of lanes 0..31
            const float4v *st = stash + (size_t)(NH - 1) * SL;
            for (int i = tid; i < ROWS * 32; i += 512) {
                vg_ge_row<FT>(lds, 0, i >> 5)[i & 31] = 0.f;
                vg_ge_row<FT>(lds, 1, i >> 5)[i & 31] = 0.f;
            }
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) {
                const int f0 = 16 * FT * wave + 16 * ft + 4 * (lane >> 4);
                float4v wv;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int f = f0 + k;
                    const half8 hi = wlb[((size_t)(f >> 5) * 2) * 64 + (f & 31)], lo = wlb[((size_t)(f >> 5) * 2 + 1) * 64 + (f & 31)];
                    wv[k] = ((float)hi[0] + (float)lo[0]) * (1.f / W16_SCALE);
                }
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    const float4v hs = st[(ft * QT + qt) * 64];
                    const int query = 16 * qt + (lane & 15);
                    float4v v;
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = wv[k] * softplus100_bwd_fast(hs[k] * (1.f / A16_SCALE)) * A16_SCALE;
                    const half4 hi = __builtin_convertvector(v, half4);
                    *reinterpret_cast<half4 *>(lds.Xh + query * XP + f0) = hi;
                    *reinterpret_cast<half4 *>(lds.Xl + query * XP + f0) =
                        __builtin_convertvector(v - __builtin_convertvector(hi, float4v), half4);
                }
            }
            __syncthreads();
        }
        for (int l = NH - 1; l >= 1; --l) {
            const nefii_layer &L = m.layer[l];
            if (L.k_e) vg_enc_grad<QT, FT>(L, lds, wave, lane, inv_scale);
            const int units = vg_units_layer(L.n_pad, FT);
            const _Float16 *ah = qh0 + (EP - L.n_pad), *al = ql0 + (EP - L.n_pad);
            asm volatile("" ::"s"(units), "v"(ah), "v"(al));
            __builtin_amdgcn_s_waitcnt(0x0070);
            __builtin_amdgcn_sched_barrier(0);
            f32x4 acc[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j][i] = 0.f;
            QAct<QT> a[2];
            qload_a<QT, XP>(a[0], ah, al, 0);
            qgemm<QT, FT>(units, b, a, cur, ah, al, acc);
            half4 phi[NJ], plo[NJ];
            const float4v *st = stash + (size_t)(l - 1) * SL;
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) {
                float4v hs[QT];
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) hs[qt] = st[(ft * QT + qt) * 64];
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    const int j = ft * QT + qt;
                    float4v v;
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = acc[j][k] * k16 * softplus100_bwd_fast(hs[qt][k] * (1.f / A16_SCALE));
                    const half4 hi = __builtin_convertvector(v, half4);
                    phi[j] = hi;
                    plo[j] = __builtin_convertvector(v - __builtin_convertvector(hi, float4v), half4);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
            _Float16 *xh = lds.Xh + (EP - L.k_x), *xl = lds.Xl + (EP - L.k_x);
#pragma unroll
            for (int ft = 0; ft < FT; ++ft) {
                const int f0 = 16 * FT * wave + 16 * ft + 4 * (lane >> 4);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    const int query = 16 * qt + (lane & 15);
                    *reinterpret_cast<half4 *>(xh + query * XP + f0) = phi[ft * QT + qt];
                    *reinterpret_cast<half4 *>(xl + query * XP + f0) = plo[ft * QT + qt];
                }
            }
            __syncthreads();
        }
        vg_enc_grad<QT, FT>(m.layer[0], lds, wave, lane, inv_scale);
        __syncthreads();
        // chain through the positional encoding
        if (tid < ROWS * 3) {
            const int p = tid / 3, c = tid - 3 * p;
            if (base + p < n) {
                const float *v = raw + p * 9;
                const int w0 = enc_width(m.enc_freqs[0]);
                const float *g0 = vg_ge_row<FT>(lds, 0, p), *g1 = vg_ge_row<FT>(lds, 1, p);
                float g = 0.f;
                for (int col = 0; col < w0; ++col) {
                    int comp;
                    const float d = enc_deriv(v, col, comp);
                    if (comp == c) g += (col < 32 ? g0[col] : g1[col - 32]) * d;
                }
                grad_out[(size_t)(base + p) * 3 + c] = g;
            }
        }
        __syncthreads();
    }
}

// the same tile evaluator over an explicit point list (nefii_sdf_eval)
__global__ __launch_bounds__(512, 2) void sdf_points_kernel16w(nefii_mlp m, const float *__restrict__ x, int64_t n,
                                                              float *__restrict__ out) {
    NEFII_CLAIM_SIMD_2();
    __shared__ Lds16w lds;
    __shared__ float raw[TILE_W * 9];
    __shared__ float *dest[TILE_W];
    const int64_t n_tiles = (n + TILE_W - 1) / TILE_W;
    const int ke = max_ke(m);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        load_points_tile<TILE_W>(x, n, out, tile, raw, dest);
        __syncthreads();
        sdf_tile16w(m, lds, raw, dest, ke);
    }
}

// rows of min-SDF draws of a call (nefii_tracer_params.minsdf_group)
int64_t minsdf_rows(int64_t n, const nefii_tracer_params *p) {
    return p->minsdf_group > 0 ? (n + p->minsdf_group - 1) / p->minsdf_group : 1;
}

// (tests/test_gpu_grid_walk.py::_crefine_offset restates the order and sizes up to s.crefine, to read every round's list of single
// samples out of a kept workspace: a change of the layout in front of it is a change there)
size_t carve(RayState &s, char *base, int64_t n, int ns, int cap, int64_t step_rows) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    };
    float **fl[] = {&s.t_s, &s.t_e, &s.cur_s, &s.cur_e, &s.nxt_s, &s.nxt_e, &s.t_min,
                    &s.t_max, &s.res_s, &s.res_e, &s.lo, &s.hi, &s.mid};
    static_assert(sizeof(fl) / sizeof(fl[0]) == TRACE_WS_FLOAT_ARRAYS, "ops.trace_iterations finds the flags behind these");
    for (auto f : fl) *f = (float *)take(sizeof(float) * n);
    s.flags = (int *)take(sizeof(int) * n);
    s.big = (float *)take(sizeof(float) * (size_t)n * ns);
    s.singles = (unsigned *)take(sizeof(unsigned) * 2 * n);
    s.dense = (unsigned *)take(sizeof(unsigned) * n);
    s.tri = (unsigned *)take(sizeof(unsigned) * n);
    s.cdense = (unsigned *)take(sizeof(unsigned) * 4 * n);
    s.refine = (unsigned *)take(sizeof(unsigned) * (size_t)n * (cap > 0 ? cap : 0));
    s.csingles = (unsigned *)take(sizeof(unsigned) * 2 * n);
    s.block_live = (int *)take(sizeof(int) * ((n + 255) / 256));
    s.crefine = (unsigned *)take(step_rows > 0 ? sizeof(unsigned) * (size_t)n * CREF_CAP : 0);
    s.ord = (unsigned char *)take(step_rows > 0 ? (size_t)step_rows * ns : 0);
    return off;
}

}  // namespace

// ---- optional per-launch timing (HIP events on the launch stream; off by default) ------------------
namespace {
struct Prof {
    bool on = false;
    std::vector<hipEvent_t> ev;      // pairs: [2i] before, [2i+1] after each eval launch
    size_t used = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;   // whole nefii_trace_rays call
    bool have_span = false;
} g_prof;
hipEvent_t prof_event() {
    if (g_prof.used == g_prof.ev.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        g_prof.ev.push_back(e);
    }
    return g_prof.ev[g_prof.used++];
}
}  // namespace

extern "C" int nefii_trace_profile_enable(int on) {
    g_prof.on = on != 0;
    g_prof.used = 0;
    g_prof.have_span = false;
    return 0;
}

// Sum of the eval-kernel launch durations recorded since enable (ms), their count, and the span of the
// last nefii_trace_rays call (ms).  Synchronises on the recorded events.
extern "C" int nefii_trace_profile_read(double *eval_ms, int *n_eval, double *span_ms) {
    double tot = 0.0;
    for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
        hipError_t e = hipEventSynchronize(g_prof.ev[i + 1]);
        if (e != hipSuccess) return (int)e;
        float ms = 0.f;
        e = hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]);
        if (e != hipSuccess) return (int)e;
        tot += ms;
    }
    if (eval_ms) *eval_ms = tot;
    if (n_eval) *n_eval = (int)(g_prof.used / 2);
    if (span_ms) {
        *span_ms = 0.0;
        if (g_prof.have_span) {
            (void)hipEventSynchronize(g_prof.t1);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, g_prof.t0, g_prof.t1);
            *span_ms = ms;
        }
    }
    g_prof.used = 0;
    return 0;
}

// Per-launch durations (ms) of the recorded eval launches, in launch order; does not clear the record.
extern "C" int nefii_trace_profile_launches(float *h_ms, int cap) {
    int n = 0;
    for (size_t i = 0; i + 1 < g_prof.used && n < cap; i += 2, ++n) {
        hipError_t e = hipEventSynchronize(g_prof.ev[i + 1]);
        if (e != hipSuccess) return -(int)e;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]);
        h_ms[n] = ms;
    }
    return n;
}

namespace nefii {
static int vg_grid(int64_t n, int rows) {
    const int64_t n_tiles = (n + rows - 1) / rows;
    return (int)(n_tiles < 256 ? (n_tiles > 0 ? n_tiles : 1) : 256);     // one workgroup per CU, grid-strided
}
// NEFII_VG_STREAM=0: keep the generic 32-row kernel (A/B measurements)
static bool vg_enabled() {
    static const bool v = env_int("NEFII_VG_STREAM", 1) != 0;
    return v;
}
size_t value_grad_stream_ws_bytes(const nefii_mlp *m, int64_t n) {
    if (!m || n <= 0 || !m->w_stream || !vg_enabled()) return 0;
    const int ft = vg_shape(m);
    if (!ft) return 0;
    const int rows = ft == 4 ? 64 : 96;        // stash: one float4 per lane and (feature tile, query tile) of a wave
    return (size_t)vg_grid(n, rows) * (m->n_layers - 1) * 8 * (ft * rows / 16) * 64 * sizeof(float4v);
}
int value_grad_stream_launch(const nefii_mlp *m, const float *x, int64_t n, float *sdf_out, int out_stride, float *feat_out,
                             int feat_stride, float *grad_out, float *ws, hipStream_t st) {
    const int ft = m->w_stream && vg_enabled() ? vg_shape(m) : 0;
    if (!ft) return NEFII_E_UNSUPPORTED;
    const int Gw = stream_steps(m) + vg_units_bwd(m);
    if (ft == 4)
        hipLaunchKernelGGL((sdf_value_grad16q_kernel<4, 4>), dim3(vg_grid(n, 64)), dim3(512), 0, st, *m, x, n, sdf_out, out_stride,
                           feat_out, feat_stride, grad_out, reinterpret_cast<float4v *>(ws), vg_stream_offset(m), Gw);
    else
        hipLaunchKernelGGL((sdf_value_grad16q_kernel<6, 2>), dim3(vg_grid(n, 96)), dim3(512), 0, st, *m, x, n, sdf_out, out_stride,
                           feat_out, feat_stride, grad_out, reinterpret_cast<float4v *>(ws), vg_stream_offset(m), Gw);
    HIP_CHECK_LAUNCH();
    return 0;
}
}  // namespace nefii

// NEFII_COARSE_D=1: 512-wide nets' 64-query single-pass tiles on the two-group form ("16d", mlp_tile.h; bit-identical values).
// Round 5, same box: 59.6 -> 58.2 us per tile on full rounds, 71.2 -> 84.6 at one tile per CU; config 3 184.1 -> 183.9 ms per
// step, config 2 2.72 -> 2.75, config 1 0.815 -> 0.849: the tile gains in cycles (layer period 16.0 k -> 11.4 k per tile) what
// the chip takes back in clock (profiles/r05/two_group_tile/).  As two 4-wave workgroups per CU (no register claim: the
// packed-fp32 canary fails beside it) config 3 went 185.6 -> 178.7.  Default: the eight-wave form "16s".
// workgroups of the two-group form: group 0 takes tiles [0, grid), group 1 [grid, 2 grid): one per CU keeps both groups of every
// CU busy from 257 tiles on
static unsigned coarse_d_grid() {
    static const int g = env_int("NEFII_COARSE_D_GRID", 0);
    return (unsigned)(g > 0 ? g : 256);
}
static int coarse_two_groups() {
    static const int v = env_int("NEFII_COARSE_D", 0);
    return v;
}
// queries per tile of the single-pass evaluator, 16 * QT.  512-wide nets: QT 4 (default) / 6 / 8 (NEFII_COARSE_QT; the big
// tiles read activation fragments single-buffered and run their epilogue behind the barrier to fit 256 registers).
// Measured per 64 queries at 12 tiles per CU: 62.0 / 58.9 / 58.3 us, at one tile per CU 77 / 100 / 123 us - the tile is
// bound by its matrix work plus the epilogue's VALU work, not by the fragment stream, so bigger tiles buy ~5 % on
// full rounds and cost latency on small ones
static int coarse_qt() {
    static const int q = env_int("NEFII_COARSE_QT", 0);
    return q == 4 || q == 6 || q == 8 ? q : 0;
}
// rows of a coarse tile for a net of feature-tile count ft
static int coarse_rows(int ft) {
    const int q = coarse_qt();
    if (ft == 2) return 96;
    return 16 * (q ? q : 4);
}
// grid of a point-list kernel: one workgroup per tile of `rows` points, grid-strided from 512 on
static dim3 points_grid(int64_t n, int rows) {
    const int64_t n_tiles = (n + rows - 1) / rows;
    return dim3((int)(n_tiles < 512 ? n_tiles : 512));
}
// launches KERNEL<QT, FT, DB> for the configured tile
#define NEFII_COARSE_LAUNCH(KERNEL, KERNEL_D, ft, grid, st, ...)                                                    \
    do {                                                                                                            \
        const int rows_ = coarse_rows(ft);                                                                          \
        if ((ft) == 2)                                                                                              \
            hipLaunchKernelGGL((KERNEL<6, 2>), grid, dim3(512), 0, st, __VA_ARGS__);                                \
        else if (rows_ == 64 && coarse_two_groups())                                                                \
            hipLaunchKernelGGL((KERNEL_D<4>), dim3((grid).x < coarse_d_grid() ? (grid).x : coarse_d_grid()), dim3(512), 0, st, \
                               __VA_ARGS__);                                                                    \
        else if (rows_ == 64)                                                                                       \
            hipLaunchKernelGGL((KERNEL<4, 4>), grid, dim3(512), 0, st, __VA_ARGS__);                                \
        else if (rows_ == 96)                                                                                       \
            hipLaunchKernelGGL((KERNEL<6, 4, false>), grid, dim3(512), 0, st, __VA_ARGS__);                         \
        else                                                                                                        \
            hipLaunchKernelGGL((KERNEL<8, 4, false>), grid, dim3(512), 0, st, __VA_ARGS__);                         \
    } while (0)

extern "C" int nefii_sdf_eval_coarse(const nefii_mlp *h_sdf, const float *x, int64_t n, float *sdf_out, void *stream) {
    if (!h_sdf || h_sdf->n_layers < 1 || h_sdf->n_layers > NEFII_MAX_LAYERS) return NEFII_E_ARG;
    if (!nefii_sdf_coarse_supported(h_sdf)) return NEFII_E_UNSUPPORTED;
    if (n <= 0) return 0;
    if (!x || !sdf_out) return NEFII_E_ARG;
    if (!sdf_net_ok(h_sdf)) return NEFII_E_UNSUPPORTED;
    const int ft = shape16p(h_sdf);
    const dim3 grid = points_grid(n, coarse_rows(ft));
    NEFII_COARSE_LAUNCH(sdf_points_kernel16s, sdf_points_kernel16d, ft, grid, (hipStream_t)stream, *h_sdf, x, n, sdf_out);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_sdf_eval_fp8corr(const nefii_mlp *h_sdf, const float *x, int64_t n, float *sdf_out, void *stream) {
    if (!h_sdf || !x || !sdf_out || n < 0) return NEFII_E_ARG;
    if (!nefii_sdf_fp8corr_supported(h_sdf)) return NEFII_E_UNSUPPORTED;
    for (int l = 0; l < h_sdf->n_layers; ++l)
        if (!h_sdf->layer[l].w_f16x3) return NEFII_E_ARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(sdf_points_kernel16f, points_grid(n, 64), dim3(512), 0, (hipStream_t)stream, *h_sdf, x, n, sdf_out,
                       (const void *)((const char *)h_sdf->w_stream + stream_bytes_1to4(h_sdf)));
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_sdf_eval(const nefii_mlp *h_sdf, const float *x, int64_t n, float *sdf_out, void *stream) {
    if (!h_sdf || h_sdf->n_layers < 1 || h_sdf->n_layers > NEFII_MAX_LAYERS) return NEFII_E_ARG;
    if (n <= 0) return 0;
    if (!x || !sdf_out) return NEFII_E_ARG;
    if (!sdf_net_ok(h_sdf)) return NEFII_E_UNSUPPORTED;
    for (int l = 0; l < h_sdf->n_layers; ++l)
        if (!h_sdf->layer[l].w_f16x3 || !h_sdf->layer[l].bias) return NEFII_E_ARG;
    const dim3 grid = points_grid(n, TILE_W);      // (sized by 64-point tiles for the 96-row kernel too)
    hipStream_t st = (hipStream_t)stream;
    const int ft = fits16p(h_sdf);
    if (ft == 2)
        hipLaunchKernelGGL(sdf_points_kernel16q<2>, grid, dim3(512), 0, st, *h_sdf, x, n, sdf_out);
    else if (ft && h_sdf->reserved == 1)
        hipLaunchKernelGGL(sdf_points_kernel16q<4>, grid, dim3(512), 0, st, *h_sdf, x, n, sdf_out);
    else if (ft)
        hipLaunchKernelGGL(sdf_points_kernel16p<P16W>, grid, dim3(64 * P16W), 0, st, *h_sdf, x, n, sdf_out);
    else
        hipLaunchKernelGGL(sdf_points_kernel16w, grid, dim3(WG_W), 0, st, *h_sdf, x, n, sdf_out);
    HIP_CHECK_LAUNCH();
    return 0;
}

// samples of one ray the coarse pass refines individually (0: coarse pass off)
static int coarse_cap(const nefii_tracer_params *p) {
    if (!(p->coarse_tau > 0.f)) return 0;
    // break-even of refining k samples of a ray (k split evaluations on top of the coarse pass, 1/3 each) against
    // re-evaluating all 100 in split precision is k ~ 67
    const int c = p->coarse_cap <= 0 ? 64 : p->coarse_cap;
    return c > 100 ? 100 : c;
}

// the staged min-SDF search runs (the coarse pass itself may still be refused for the net: then it is simply not used)
static bool minsdf_staged(const nefii_tracer_params *p) {
    return p->coarse_tau > 0.f && p->minsdf_lipschitz > 0.f && p->n_steps >= 16 && p->n_steps <= 128;
}

// rounds of sphere tracing at the most: the initial evaluation, then a step and its back-offs per iteration - twice that
// with the tier (the coarse value, then the exact one)
static int trace_rounds(const nefii_tracer_params *p) {
    const int trace = 1 + p->sphere_tracing_iters * (1 + p->line_step_iters);
    return trace * (p->coarse_tau > 0.f && p->trace_tier ? 2 : 1);
}

// Shared first stage of the staged min-SDF search (minsdf_share): a follower's row is in one round later than its own
// search's would be - it waits for its leader's two stages, then evaluates its candidates - and two rounds later when it
// falls back.  The bound below has room for that: a ray that enters the min-SDF search has !F_SAMP, so it comes straight
// from sphere tracing, in round trace_rounds() at the latest, and has used none of the rounds reserved for the bracket
// search (1, with the coarse pass 3 + 3 + 1 more) and the bisection.  From there its own search takes five rounds (first
// stage, second stage, the two refinement stages, the exact argmin), a follower's at most seven.  Returns whether seven fit
// - they do for every parameter set the bound's coarse terms are counted for; a call for which they do not runs unshared.
static bool minsdf_share_fits(const nefii_tracer_params *p) {
    return nefii_trace_max_rounds(p) - 1 - trace_rounds(p) >= 6;
}

extern "C" int nefii_trace_max_rounds(const nefii_tracer_params *p) {
    if (!p) return 0;
    // initial eval + iters*(step + back-offs) -> sampler -> bisection (L levels per round) -> min-SDF -> bookkeeping
    // with the coarse pass each of the two dense searches takes one round more (coarse samples -> refined samples)
    const int L = p->bisect_levels >= 1 && p->bisect_levels <= 5 ? p->bisect_levels : 3;
    // ... and the bracket search one more for the rays whose leading samples (evaluated exactly first) hold no negative one,
    // up to three more for the quarter rows of its coarse pass, the min-SDF search one more for its two-stage refinement
    // tiered sphere tracing: every sphere-tracing evaluation may take a second round (the coarse value, then the exact one)
    const int trace = 1 + p->sphere_tracing_iters * (1 + p->line_step_iters);
    // staged min-SDF search: its two stages take the place of the one coarse round
    return trace + 1 + (p->n_rootfind_steps + L - 1) / L + 1 + 2 +
           (p->coarse_tau > 0.f ? 3 + 3 + 1 + (p->trace_tier ? trace : 0) : 0) + (minsdf_staged(p) ? 1 : 0);
}

extern "C" size_t nefii_trace_workspace_bytes(int64_t n_rays, const nefii_tracer_params *p) {
    if (!p || n_rays <= 0) return 0;
    RayState s;
    size_t bytes = carve(s, nullptr, n_rays, p->n_steps, coarse_cap(p), minsdf_staged(p) ? minsdf_rows(n_rays, p) : 0);
    bytes += align256(sizeof(int) * NCNT * (size_t)nefii_trace_max_rounds(p));
    return bytes;
}

// One tracer invocation (a ray batch on a stream), split into prepare / one round / finish so that several batches can be
// enqueued round by round on separate streams (nefii_trace_rays_groups).
struct TraceJob {
    Params P;
    const nefii_mlp *sdf;
    int precision, rounds, adv_blocks, eval_blocks, eval_blocks_w;
    int pipelined;      // feature tiles per wave of the pipelined evaluator (4 / 2), 0: generic kernels
    int coarse;         // the coarse pass runs (its kernel is launched every round)
    const void *f8;     // nefii_tracer_params.split_fp8 and the net has the fifth stream copy: the "16f" evaluator's stream, else null
    hipStream_t st;
    int32_t *counters;
};

// the rays of one batch and where their results go
struct RayBatch {
    const float *origins, *dirs;
    const uint8_t *object_mask;
    int64_t n;
    float *out_points;
    uint8_t *out_hit;
    float *out_dists;
    // rays [lo, lo + count) of the batch
    RayBatch chunk(int64_t lo, int64_t count) const {
        return {origins + 3 * lo, dirs + 3 * lo, object_mask + lo, count, out_points + 3 * lo, out_hit + lo, out_dists + lo};
    }
};

// the two mode words of a grid descriptor are checked before anything else, whatever the other arguments
static bool grid_modes_ok(const nefii_trace_grid *g) {
    return !g || (g->training >= 0 && g->training <= 1 && g->certify >= 0 && g->certify <= 3);
}

int prepare_job(TraceJob &J, const nefii_mlp *h_sdf, const nefii_tracer_params *h_params, const RayBatch &B,
                const float *lin_steps, const float *minsdf_steps, void *workspace, size_t workspace_bytes, int32_t *counters,
                bool reset, void *stream, const nefii_trace_grid *grid) {
    const int64_t n_rays = B.n;
    if (!h_sdf || !h_params || !B.origins || !B.dirs || !B.object_mask || !lin_steps || !B.out_points || !B.out_hit ||
        !B.out_dists || !workspace)
        return NEFII_E_ARG;
    if (n_rays <= 0 || n_rays >= (1ll << 29)) return NEFII_E_SHAPE;
    if (h_params->training && !minsdf_steps) return NEFII_E_ARG;
    const int levels = h_params->bisect_levels >= 1 && h_params->bisect_levels <= 5 ? h_params->bisect_levels : 3;
    if (h_params->bisect_levels < 0 || h_params->bisect_levels > 5) return NEFII_E_ARG;
    if (h_params->n_steps < (1 << levels) || h_params->sphere_tracing_iters > 250 || h_params->line_step_iters > 15 ||
        h_params->n_rootfind_steps > 250)
        return NEFII_E_SHAPE;
    // (a negative count would make nefii_trace_max_rounds - the size of the counter block - meaningless)
    if (h_params->sphere_tracing_iters < 0 || h_params->line_step_iters < 0 || h_params->n_rootfind_steps < 0)
        return NEFII_E_SHAPE;
    if (!sdf_net_ok(h_sdf)) return NEFII_E_UNSUPPORTED;
    if (workspace_bytes < nefii_trace_workspace_bytes(n_rays, h_params)) return NEFII_E_SHAPE;
    if (h_params->precision < 0 || h_params->precision > 2) return NEFII_E_ARG;
    if (h_params->precision >= 1)
        for (int l = 0; l < h_sdf->n_layers; ++l)
            if (!h_sdf->layer[l].w_f16x3) return NEFII_E_ARG;
    J.sdf = h_sdf;
    J.st = (hipStream_t)stream;
    J.precision = h_params->precision;
    J.rounds = nefii_trace_max_rounds(h_params);
    J.counters = counters;
    Params &P = J.P;
    P.p = *h_params;
    P.n = n_rays;
    P.o = B.origins;
    P.d = B.dirs;
    P.obj = B.object_mask;
    P.lin = lin_steps;
    P.steps = minsdf_steps ? minsdf_steps : lin_steps;
    if (!minsdf_steps) P.p.minsdf_group = 0;
    P.out_pts = B.out_points;
    P.out_dist = B.out_dists;
    P.out_hit = B.out_hit;
    // coarse pass: needs the single-pass stream (pipelined shapes, 16x16x32 layout), sample ids in 7 bits and ray ids in
    // the other 25 of a refine entry
    J.pipelined = h_params->precision == 2 ? fits16p(h_sdf) : 0;
    if (h_params->split_fp8 < 0 || h_params->split_fp8 > 1) return NEFII_E_ARG;
    J.f8 = (h_params->split_fp8 && J.pipelined == 4 && nefii_sdf_fp8corr_supported(h_sdf))
               ? (const void *)((const char *)h_sdf->w_stream + stream_bytes_1to4(h_sdf)) : nullptr;
    J.coarse = h_params->coarse_tau > 0.f && J.pipelined && nefii_sdf_coarse_supported(h_sdf) &&
               n_rays < (1ll << 25) && h_params->n_steps <= 128;
    if (h_params->coarse_tau < 0.f || h_params->coarse_tau > 1.f) return NEFII_E_ARG;
    P.tau = J.coarse ? h_params->coarse_tau : 0.f;
    P.cap = coarse_cap(h_params);
    P.chunk = 0;
    P.chunk_gate = 1e30f;
    P.window = 0;
    P.tier_band = 0.f;
    P.tier_gate = 0.f;
    if (h_params->trace_tier < 0 || h_params->trace_tier > 1 || h_params->tier_kappa < 0.f || h_params->tier_gate < 0.f)
        return NEFII_E_ARG;
    if (J.coarse && h_params->trace_tier) {
        // the band must cover what the recurrence decides: v <= thr and v < 0, given |v16 - v| < tau
        const float kappa = h_params->tier_kappa > 0.f ? h_params->tier_kappa : 2.f;
        const float band = kappa * P.tau, least = P.tau + 2.f * fabsf(h_params->sdf_threshold);
        P.tier_band = band > least ? band : least;
        P.tier_gate = (h_params->tier_gate > 0.f ? h_params->tier_gate : 4.f) * P.tau;
    }
    if (J.coarse && h_params->n_steps >= 16) {      // NEFII_SAMPLER_WINDOW=0: whole rows (A/B switch)
        // bit 0: quarter rows, bit 1: two-stage min-SDF refinement.  Both trade rounds for evaluations: the two-stage
        // refinement pays everywhere (config 2: 3.05 -> 2.95 ms per step), the quarter rows' three extra rounds only where
        // evaluations, not round latency, make the trace (config 3: -4 %; config 2's 4096 rays: +4 %)
        P.window = env_int("NEFII_SAMPLER_WINDOW", 2 | (n_rays >= 32768 ? 1 : 0)) & 3;
    }
    if (J.coarse) {       // NEFII_SAMPLER_CHUNK: leading samples of a bracket search evaluated exactly first (0: off; A/B switch)
        const int c = env_int("NEFII_SAMPLER_CHUNK", 6);       // 4 / 6 / 8 / 16: 195.8 / 196.9 / 197.2 / 203.7 ms per step on config 3 (208.7 without), 2.82 / 2.79 / 2.79 / 2.81 on config 2
        P.chunk = (c >= 2 && c <= 31 && c <= P.cap && c < h_params->n_steps) ? c : 0;
        // 1: the chunk's last sample is within reach of the surface if |grad sdf| <= 1.  Config 3 / 4, ms per step: no gate
        // 197.3 / 174.0, gate 4: 196.7 / 173.2, 2: 195.5 / 172.0, 1: 195.1 / 171.6, 0.7: 193.9 / 171.1, 0.35: 194.2 / 171.5
        P.chunk_gate = env_float("NEFII_SAMPLER_CHUNK_GATE", 1.0f);
    }
    if (h_params->minsdf_lipschitz < 0.f || h_params->minsdf_lipschitz > 1e6f) return NEFII_E_ARG;
    const bool staged = J.coarse && minsdf_staged(h_params);
    P.lip = staged ? h_params->minsdf_lipschitz : 0.f;
    // NEFII_MINSDF_SHARE=0: every ray of a wave runs its own first stage (A/B switch; read per call, so a trace continued by a
    // second call must find the value its first rounds ran with)
    P.share = staged && h_params->training && minsdf_share_fits(h_params) && env_int("NEFII_MINSDF_SHARE", 1) != 0;
    // NEFII_BRACKET_STAGED=0: the bracket search keeps its quarter-row windows (A/B switch)
    static const int stage_bracket = env_int("NEFII_BRACKET_STAGED", 1) != 0;
    P.stage_bracket = stage_bracket;
    if (h_params->unread_misses < 0 || h_params->unread_misses > 1) return NEFII_E_ARG;
    P.miss_argmin = !(h_params->unread_misses && !h_params->training);
    // the SDF interval grid (nefii_trace_grid; none: all zero): read by the staged bracket searches of eval-mode traces and - with
    // nefii_trace_grid.training - of the rays inside the object mask of training-mode ones
    const nefii_trace_grid g = grid ? *grid : nefii_trace_grid{};
    const int grid_n = g.G;
    if (g.cells && (grid_n < 1 || grid_n > NEFII_BOUND_GRID_MAX)) return NEFII_E_SHAPE;
    P.cells = staged ? (const unsigned *)g.cells : nullptr;
    P.grid_n = grid_n;
    P.grid_inv_h = (float)((double)grid_n / (2.0 * (double)h_params->object_bounding_sphere));
    // ... and the vertex values behind it: both arrays or neither, and only with the cells
    if (!g.vertex_g != !g.cell_l || (g.vertex_g && !g.cells)) return NEFII_E_ARG;
    P.vert_g = P.cells ? (const unsigned short *)g.vertex_g : nullptr;
    P.cell_l = P.cells ? (const unsigned short *)g.cell_l : nullptr;
    P.grid_training = g.training;
    P.grid_h = grid_n > 0 ? (float)(2.0 * (double)h_params->object_bounding_sphere / (double)grid_n) : 0.f;
    // NEFII_GRID_WALK_WAVE=0: every ray walks the grid in its own thread (A/B switch and the tests' reference; read per call)
    P.walk_wave = env_int("NEFII_GRID_WALK_WAVE", 1) != 0;
    // the block level and the certificates (nefii_trace_grid.certify): only where the grid itself is read (a net without the
    // staged searches traces as if the call had not asked)
    if (g.certify && (!g.cells || !g.blocks)) return NEFII_E_ARG;
    P.blocks = P.cells ? (const unsigned short *)g.blocks : nullptr;
    P.block_n = nefii_sdf_bound_grid_block_count(grid_n);
    P.certify = (g.certify & 1) && P.blocks && P.block_n > 0 && h_params->training;
    P.certify_free = (g.certify & 2) && P.blocks && P.block_n > 0 && !h_params->training && h_params->unread_misses;
    P.cert_counts = (P.certify || P.certify_free) ? g.certify_counts : nullptr;
    // (the workspace is laid out by the PARAMETERS, as nefii_trace_workspace_bytes sized it, whether or not the net takes the coarse pass)
    const int64_t step_rows = minsdf_staged(h_params) ? minsdf_rows(n_rays, &P.p) : 0;
    size_t off = carve(P.s, (char *)workspace, n_rays, h_params->n_steps, P.cap, step_rows);
    P.counters = (int *)((char *)workspace + off);
    P.levels = levels;
    P.tri_nodes = (1 << levels) - 1;
    if (reset) {      // a continuation keeps the ray state and counters in the workspace
        hipError_t e = hipMemsetAsync(P.counters, 0, sizeof(int) * NCNT * J.rounds, J.st);
        if (e != hipSuccess) return (int)e;
        e = hipMemsetAsync(P.s.flags, 0, sizeof(int) * n_rays, J.st);
        if (e != hipSuccess) return (int)e;
        if (staged && h_params->training) {
            hipLaunchKernelGGL(minsdf_order_kernel, dim3((int)minsdf_rows(n_rays, &P.p)), dim3(128), 0, J.st, P);
            HIP_CHECK_LAUNCH();
        }
    }
    J.adv_blocks = (int)((n_rays + 255) / 256);
    // eval grid: enough workgroups for the largest possible round, capped at 2 per CU (grid-stride beyond)
    const int64_t max_q = n_rays * (int64_t)h_params->n_steps;   // n_steps >= 2^levels > bisection tree nodes > 2 ends
    const int64_t max_tiles = (max_q + TILE - 1) / TILE;
    J.eval_blocks = (int)(max_tiles < 1024 ? max_tiles : 1024);
    const int64_t max_tiles_w = (max_q + TILE_W - 1) / TILE_W;
    // tile evaluators: up to 2048 workgroups (one resident per CU: LDS), i.e. one or two tiles each for the rounds of the
    // headline workloads - the hardware dispatcher then balances tiles over CUs, also between the kernels of two traces in
    // flight (measured 256 / 512 / 768 / 2048: 4.73 / 4.68 / 4.58.. / -3 % ms per step on config 2, flat on config 3)
    static const int eval_grid = env_int("NEFII_EVAL_GRID", 0);
    const int grid_cap = eval_grid > 0 ? eval_grid : 2048;
    J.eval_blocks_w = (int)(max_tiles_w < grid_cap ? max_tiles_w : grid_cap);
    return 0;
}

int launch_round(const TraceJob &J, int r, bool profile) {
    hipStream_t st = J.st;
    hipLaunchKernelGGL(advance_kernel, dim3(J.adv_blocks), dim3(256), 0, st, J.P, r);
    HIP_CHECK_LAUNCH();
    if (r + 1 < J.rounds) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (profile) {
            e0 = prof_event();
            e1 = prof_event();
            (void)hipEventRecord(e0, st);
        }
        // the pipelined families run as a pair per round: the big-tile instance on the full grid, then the 32-query instance
        // on one workgroup per CU at most; the round's query count (known on the device only) decides which of them works
        const int64_t small_tiles = (J.P.n * 2 + 31) / 32 < 256 ? (J.P.n * 2 + 31) / 32 : 256;   // >= SMALL_ROUND / 32
        const dim3 big_grid(J.eval_blocks_w), small_grid((int)(small_tiles < 1 ? 1 : small_tiles));
        auto pair = [&](auto big, auto small, int block, const auto &...args) -> int {
            hipLaunchKernelGGL(big, big_grid, dim3(block), 0, st, args...);
            HIP_CHECK_LAUNCH();
            hipLaunchKernelGGL(small, small_grid, dim3(block), 0, st, args...);
            return 0;
        };
        int rc = 0;
        const bool split = J.precision == 2, q_layout = J.sdf->reserved == 1;
        if (split && J.pipelined == 2)                  // 256-wide nets (16x16x32 layout only)
            rc = pair(eval_kernel16q<6, 2>, eval_kernel16q<2, 2>, 512, J.P, *J.sdf, r);
        else if (split && J.pipelined && q_layout && J.f8)      // 512-wide, fp8 correction products
            rc = pair(eval_kernel16f<4>, eval_kernel16f<2>, 512, J.P, *J.sdf, r, J.f8);
        else if (split && J.pipelined && q_layout && J.P.n <= 1024)     // 512-wide, few CUs streaming: deep prefetch
            rc = pair(eval_kernel16q<4, 4>, eval_kernel16q<2, 4, true>, 512, J.P, *J.sdf, r);
        else if (split && J.pipelined && q_layout)      // 512-wide
            rc = pair(eval_kernel16q<4, 4>, eval_kernel16q<2, 4>, 512, J.P, *J.sdf, r);
        else if (split && J.pipelined)                  // 512-wide, 32x32x16 layout
            rc = pair(eval_kernel16p<P16W, 2>, eval_kernel16p<P16W, 1>, 64 * P16W, J.P, *J.sdf, r);
        else if (split)                                 // any other shape
            hipLaunchKernelGGL(eval_kernel16w, big_grid, dim3(WG_W), 0, st, J.P, *J.sdf, r);
        else if (J.precision == 1)
            hipLaunchKernelGGL(eval_kernel16, dim3(J.eval_blocks), dim3(WG), 0, st, J.P, *J.sdf, r);
        else
            hipLaunchKernelGGL(eval_kernel, dim3(J.eval_blocks), dim3(WG), 0, st, J.P, *J.sdf, r);
        if (rc) return rc;
        HIP_CHECK_LAUNCH();
        if (J.coarse) {
            const int ft = J.pipelined == 2 ? 2 : 4, rows = coarse_rows(ft);
            const int64_t t = (J.P.n * (int64_t)(4 * coarse_window(J.P.p.n_steps) + 2) + rows - 1) / rows;
            const dim3 grid((int)(t < J.eval_blocks_w ? t : J.eval_blocks_w));
            NEFII_COARSE_LAUNCH(eval_kernel16s, eval_kernel16d, ft, grid, st, J.P, *J.sdf, r);
            HIP_CHECK_LAUNCH();
        }
        if (profile) (void)hipEventRecord(e1, st);
    }
    return 0;
}

int finish_job(const TraceJob &J) {
    if (J.counters) {
        hipError_t e = hipMemcpyAsync(J.counters, J.P.counters, sizeof(int) * NCNT * J.rounds, hipMemcpyDeviceToDevice, J.st);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

extern "C" int nefii_trace_rays_rounds(const nefii_mlp *h_sdf, const nefii_tracer_params *h_params,
                                       const float *origins, const float *dirs, const uint8_t *object_mask,
                                       int64_t n_rays, const float *lin_steps, const float *minsdf_steps,
                                       float *out_points, uint8_t *out_hit, float *out_dists, void *workspace,
                                       size_t workspace_bytes, int32_t *counters, int round_begin, int round_end,
                                       const nefii_trace_grid *grid, void *stream) {
    if (!grid_modes_ok(grid)) return NEFII_E_ARG;
    if (n_rays == 0 && h_sdf && h_params) return 0;
    TraceJob J;
    const RayBatch B = {origins, dirs, object_mask, n_rays, out_points, out_hit, out_dists};
    int rc = prepare_job(J, h_sdf, h_params, B, lin_steps, minsdf_steps, workspace, workspace_bytes, counters, round_begin == 0,
                         stream, grid);
    if (rc) return rc;
    if (round_end <= 0 || round_end > J.rounds) round_end = J.rounds;
    if (round_begin < 0 || round_begin >= round_end) return NEFII_E_ARG;
    if (g_prof.on) {
        if (!g_prof.t0) {
            (void)hipEventCreate(&g_prof.t0);
            (void)hipEventCreate(&g_prof.t1);
        }
        (void)hipEventRecord(g_prof.t0, J.st);
    }
    for (int r = round_begin; r < round_end; ++r) {
        rc = launch_round(J, r, g_prof.on);
        if (rc) return rc;
    }
    if (g_prof.on) {
        (void)hipEventRecord(g_prof.t1, J.st);
        g_prof.have_span = true;
    }
    return finish_job(J);
}

extern "C" int nefii_trace_rays_groups(const nefii_mlp *h_sdf, const nefii_tracer_params *h_params,
                                       const float *origins, const float *dirs, const uint8_t *object_mask,
                                       int n_groups, const int64_t *group_begin, const float *lin_steps,
                                       const float *minsdf_steps, float *out_points, uint8_t *out_hit,
                                       float *out_dists, void *const *workspaces, const size_t *workspace_bytes,
                                       int32_t *counters, int round_begin, int round_end, const nefii_trace_grid *grid,
                                       void *const *streams) {
    if (!grid_modes_ok(grid)) return NEFII_E_ARG;
    if (n_groups < 1 || n_groups > 16 || !group_begin || !workspaces || !workspace_bytes || !streams) return NEFII_E_ARG;
    if (!h_params) return NEFII_E_ARG;
    TraceJob J[16];
    const int rounds = nefii_trace_max_rounds(h_params);
    if (round_end <= 0 || round_end > rounds) round_end = rounds;
    if (round_begin < 0 || round_begin >= round_end) return NEFII_E_ARG;
    const RayBatch B = {origins, dirs, object_mask, 0, out_points, out_hit, out_dists};
    for (int g = 0; g < n_groups; ++g) {
        const int64_t lo = group_begin[g], n = group_begin[g + 1] - lo;
        if (lo < 0 || n <= 0) return NEFII_E_ARG;
        int rc = prepare_job(J[g], h_sdf, h_params, B.chunk(lo, n), lin_steps, minsdf_steps, workspaces[g], workspace_bytes[g],
                             counters ? counters + (size_t)g * rounds * NCNT : nullptr, round_begin == 0, streams[g], grid);
        if (rc) return rc;
    }
    for (int r = round_begin; r < round_end; ++r)       // round-major: every chunk advances together
        for (int g = 0; g < n_groups; ++g) {
            int rc = launch_round(J[g], r, false);
            if (rc) return rc;
        }
    for (int g = 0; g < n_groups; ++g) {
        int rc = finish_job(J[g]);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int nefii_trace_rays(const nefii_mlp *h_sdf, const nefii_tracer_params *h_params, const float *origins,
                                const float *dirs, const uint8_t *object_mask, int64_t n_rays, const float *lin_steps,
                                const float *minsdf_steps, float *out_points, uint8_t *out_hit, float *out_dists,
                                void *workspace, size_t workspace_bytes, int32_t *counters, void *stream) {
    return nefii_trace_rays_rounds(h_sdf, h_params, origins, dirs, object_mask, n_rays, lin_steps, minsdf_steps,
                                   out_points, out_hit, out_dists, workspace, workspace_bytes, counters, 0, 0, nullptr, stream);
}

// ------------------------------------------------------------------------------------------------
// camera rays (rend_util.py:90-142)
// ------------------------------------------------------------------------------------------------
__global__ void camera_rays_kernel(const float *__restrict__ uv, const float *__restrict__ pose,
                                   const float *__restrict__ K, int batch, int64_t samples, float *__restrict__ dirs,
                                   float *__restrict__ origins) {
    const int64_t total = (int64_t)batch * samples;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / samples);
        const float *Kb = K + b * 16, *Pb = pose + b * 16;
        const float fx = Kb[0], sk = Kb[1], cx = Kb[2], fy = Kb[5], cy = Kb[6];
        const float u = uv[i * 2], v = uv[i * 2 + 1];
        // x = (u - cx + cy*sk/fy - sk*v/fy) / fx * z ; y = (v - cy)/fy * z ; z = 1   (lift, :129-142)
        const float x = __fdiv_rn(fsub(fadd(fsub(u, cx), __fdiv_rn(fmul(cy, sk), fy)), __fdiv_rn(fmul(sk, v), fy)), fx);
        const float y = __fdiv_rn(fsub(v, cy), fy);
        float w[3];
        for (int c = 0; c < 3; ++c) {
            // world = pose * [x, y, 1, 1]; dirs = world - cam
            const float wc = fadd(fadd(fadd(fmul(Pb[c * 4], x), fmul(Pb[c * 4 + 1], y)), Pb[c * 4 + 2]), Pb[c * 4 + 3]);
            w[c] = fsub(wc, Pb[c * 4 + 3]);
        }
        const float nrm = fmaxf(sqrtf(fadd(fadd(fmul(w[0], w[0]), fmul(w[1], w[1])), fmul(w[2], w[2]))), 1e-12f);
        for (int c = 0; c < 3; ++c) {
            dirs[i * 3 + c] = __fdiv_rn(w[c], nrm);
            origins[i * 3 + c] = Pb[c * 4 + 3];
        }
    }
}

extern "C" int nefii_camera_rays(const float *uv, const float *pose, const float *intrinsics, int batch,
                                 int64_t samples, float *out_dirs, float *out_origins, void *stream) {
    if (!uv || !pose || !intrinsics || !out_dirs || !out_origins) return NEFII_E_ARG;
    const int64_t total = (int64_t)batch * samples;
    if (total <= 0) return 0;
    int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(camera_rays_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, uv, pose, intrinsics, batch,
                       samples, out_dirs, out_origins);
    HIP_CHECK_LAUNCH();
    return 0;
}
