// nefii_meshcc.hip - connected components of a triangle mesh by min-label hooking and pointer jumping.
// Replaces trimesh's Trimesh.split of the reference's get_surface_high_res_mesh (code/utils/plots.py:186-189) for meshes
// that already live on the GPU.
//
// parent [V] int32 is a forest over the vertices.  INVARIANT, at all times and for every value an entry ever takes:
//     parent[x] <= x,   parent[x] is a vertex of x's component,   and an entry only ever decreases.
// init:  parent[v] = v.
// hook:  one thread per face (a, b, c).  With p. = parent[.] and g = the least of parent[pa], parent[pb], parent[pc], the
//        entries parent[pa], parent[pb], parent[pc], parent[a], parent[b], parent[c] are lowered to g by atomicMin (one vector
//        atomic on global memory each; issued only where the value read is above g - the entry cannot have risen since).  A
//        thread whose atomic returned a value above g has lowered something and stores 1 to flags[0].
// jump:  one thread per vertex follows parent to its root and stores the root.
// A load may return an older value than the entry holds by then (another thread's atomic in flight, a cached line): an older
// value is a larger one that the entry did hold, so the invariant covers it, and the round merely lowers less.  Every chase
// therefore descends strictly (parent[x] < x or it stops) and ends after fewer than V steps; the loops also stop on any
// value that does not descend, so that no content of `parent` can make a thread spin.  There is no compare-and-swap loop
// and no waiting on another thread anywhere.
//
// The caller repeats rounds (hook + jump) until a round leaves flags[0] == 0.  In that round no entry changed while the hook
// kernel ran, so what it read was exact: for every face the six entries already equalled g, which makes g a root
// (parent[g] == g) that the three vertices point at directly.  Faces sharing a vertex share that root, so a whole
// edge-connected component has ONE root r.  Its least vertex m has parent[m] <= m inside the component, hence parent[m] == m,
// and parent[m] == r: the root is m.  label[v] = the smallest vertex index of v's component, whatever the schedule.
//
// A face with an index outside [0, V) is never followed: it sets flags[1] and is skipped.
#include <hip/hip_runtime.h>
#include "../../include/nefii_amd.h"

#include "hip_check.h"

namespace {

constexpr int BLOCK = 256;
constexpr int64_t MAX_COUNT = 0x7fffffffll;          // n_verts, n_faces < 2^31

__global__ __launch_bounds__(BLOCK) void meshcc_init_kernel(int *__restrict__ parent, int n_verts, int *__restrict__ flags) {
    const int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (v == 0) {
        flags[0] = 0;
        flags[1] = 0;
    }
    if (v < n_verts) parent[v] = (int)v;
}

__global__ __launch_bounds__(BLOCK) void meshcc_clear_changed_kernel(int *__restrict__ flags) { flags[0] = 0; }

// lowers *entry to g where `seen`, a value the entry held, is above g; true when this thread's atomic did the lowering
__device__ __forceinline__ bool lower(int *entry, int seen, int g) { return seen > g && atomicMin(entry, g) > g; }

__global__ __launch_bounds__(BLOCK) void meshcc_hook_kernel(const int *__restrict__ faces, int64_t n_faces, int *parent,
                                                             int n_verts, int *flags) {
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const unsigned V = (unsigned)n_verts;
    if ((unsigned)a >= V || (unsigned)b >= V || (unsigned)c >= V) {        // negative indices wrap above V
        flags[1] = 1;
        return;
    }
    // every value below was stored by init, a hook or a jump: a vertex index in [0, V).  A `parent` that was never
    // initialised breaks that; it is not followed either.
    const int pa = parent[a], pb = parent[b], pc = parent[c];
    if ((unsigned)pa > (unsigned)a || (unsigned)pb > (unsigned)b || (unsigned)pc > (unsigned)c) {
        flags[1] = 1;
        return;
    }
    const int ga = parent[pa], gb = parent[pb], gc = parent[pc];
    const int g = min(ga, min(gb, gc));                                     // g <= g. <= p. <= the vertex (the invariant)
    bool changed = lower(parent + pa, ga, g);
    changed |= lower(parent + pb, gb, g);
    changed |= lower(parent + pc, gc, g);
    changed |= lower(parent + a, pa, g);
    changed |= lower(parent + b, pb, g);
    changed |= lower(parent + c, pc, g);
    if (changed) flags[0] = 1;
}

__global__ __launch_bounds__(BLOCK) void meshcc_jump_kernel(int *parent, int n_verts) {
    const int64_t v = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (v >= n_verts) return;
    const int p = parent[v];
    if ((unsigned)p > (unsigned)v) return;           // not a value this file stores: never followed
    int r = p;
    while (r > 0) {                                  // parent[x] <= x: r descends strictly or the chase stops
        const int q = parent[r];
        if (q >= r || q < 0) break;
        r = q;
    }
    if (r < p) parent[v] = r;                        // only this thread stores to parent[v] in this kernel
}

unsigned blocks(int64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

int check(const void *faces, int64_t n_faces, const void *parent, int64_t n_verts, const void *flags) {
    if (!parent || !flags || (!faces && n_faces != 0)) return NEFII_E_ARG;
    if (n_verts < 0 || n_verts >= MAX_COUNT + 1 || n_faces < 0 || n_faces >= MAX_COUNT + 1) return NEFII_E_SHAPE;
    return 0;
}

}  // namespace

extern "C" int nefii_mesh_cc_init(int32_t *parent, int64_t n_verts, int32_t *flags, void *stream) {
    const int rc = check(nullptr, 0, parent, n_verts, flags);
    if (rc) return rc;
    if (n_verts == 0) return 0;
    hipLaunchKernelGGL(meshcc_init_kernel, dim3(blocks(n_verts)), dim3(BLOCK), 0, (hipStream_t)stream, parent,
                       (int)n_verts, flags);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_mesh_cc_round(const int32_t *faces, int64_t n_faces, int32_t *parent, int64_t n_verts, int32_t *flags,
                                   void *stream) {
    if (!faces) return NEFII_E_ARG;
    const int rc = check(faces, n_faces, parent, n_verts, flags);
    if (rc) return rc;
    if (n_verts == 0) return 0;
    hipLaunchKernelGGL(meshcc_clear_changed_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, flags);
    HIP_CHECK_LAUNCH();
    if (n_faces == 0) return 0;
    hipLaunchKernelGGL(meshcc_hook_kernel, dim3(blocks(n_faces)), dim3(BLOCK), 0, (hipStream_t)stream, faces, n_faces, parent,
                       (int)n_verts, flags);
    HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(meshcc_jump_kernel, dim3(blocks(n_verts)), dim3(BLOCK), 0, (hipStream_t)stream, parent, (int)n_verts);
    HIP_CHECK_LAUNCH();
    return 0;
}
