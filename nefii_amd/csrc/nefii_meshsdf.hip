// nefii_meshsdf.hip - exact signed distance from query points to a triangle mesh through a bounding-volume hierarchy
// (DESIGN.md 6k).  Replaces the queries x faces products of datasets/sdf_dataset.py:MeshSDF.__call__ (reference
// code/datasets/sdf_dataset.py:18-77, where mesh-to-sdf answers the query from a scanned point cloud).
//
// The tree (nefii_amd/mesh_bvh.py) is an implicit complete binary tree in heap order over N = n_leaves_pow2 leaves: node i has
// the children 2 i + 1 and 2 i + 2, the leaves are the nodes N - 1 .. 2 N - 2, leaf j holds the faces [j leaf_size,
// min((j + 1) leaf_size, n_tris)) of the sorted triangle array.  node_box [2 N - 1][6] = (lo.xyz, hi.xyz) in fp64; an empty
// (padding) node has lo = +inf, hi = -inf.  Points, triangles and boxes share one frame (MeshSDF's skewed frame).
//
// One thread per query, two depth-first traversals with an explicit stack:
//   A  distance: at an inner node both children's box distances d^2 are computed, the nearer child is entered first, the
//      other is pushed; a node is skipped only when  d^2 (1 - 2^-40) > best d^2 so far  (strictly; the factor keeps the box
//      test on the safe side of the few ulps by which the triangle formulas and the box formula may disagree, so that the
//      minimum is the minimum over ALL faces whatever the shape of the tree) or when it is empty (d^2 = inf).  A pushed node
//      is tested again when it is popped: best has usually shrunk by then.  Leaves evaluate MeshSDF's point-triangle
//      distance: the plane distance inside the prism over the face, else the least of the three clamped segment distances.
//   B  sign: crossings of the ray q + t z, t > 0.  A node is entered only if q.xy lies inside its xy box and its hi.z > q.z;
//      leaves apply MeshSDF's edge functions, its `covers` rule, area2 != 0 and z > q.z term for term (the library is built
//      with -ffp-contract=off: no product is fused into a sum), and count in an integer.
// Both results are order-independent - an exact minimum, an integer count - so a query's result is the same bits wherever it
// sits in the batch, from run to run, and for any order of the faces.
//
// The stack holds node indices only (4 bytes) and lives in LDS as stack[level][thread]: a runtime-indexed per-thread array
// would be placed in scratch memory.  Bank = thread, so no access conflicts.  A path of the tree pushes at most one node per
// inner level: 26 levels for N <= 2^26, 26 KiB per 256-thread workgroup.
//
// A second kernel on the same tree gives the generalized winding number, whose sign needs no closed mesh: see below.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/nefii_amd.h"

#include "hip_check.h"

namespace {

constexpr int BLOCK = 256;
constexpr int STACK = 26;                           // inner levels of the deepest tree accepted
constexpr int64_t MAX_TRIS = (1ll << 26) - 1;
constexpr int64_t MAX_LEAVES = 1ll << STACK;
constexpr int MAX_LEAF = 8;
constexpr double BOX_SHRINK = 1.0 - 0x1p-40;

struct V3 {
    double x, y, z;
};
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 load3(const double *__restrict__ p) { return {p[0], p[1], p[2]}; }

__device__ __forceinline__ void load_box(const double2 *__restrict__ node_box, int node, V3 &lo, V3 &hi) {
    const double2 *p = node_box + 3 * (size_t)node;
    const double2 a = p[0], b = p[1], c = p[2];
    lo = {a.x, a.y, b.x};
    hi = {b.y, c.x, c.y};
}

__device__ __forceinline__ double box_d2(V3 lo, V3 hi, V3 q) {
    const double dx = fmax(fmax(lo.x - q.x, q.x - hi.x), 0.0);
    const double dy = fmax(fmax(lo.y - q.y, q.y - hi.y), 0.0);
    const double dz = fmax(fmax(lo.z - q.z, q.z - hi.z), 0.0);
    return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ double node_d2(const double2 *__restrict__ node_box, int node, V3 q) {
    V3 lo, hi;
    load_box(node_box, node, lo, hi);
    return box_d2(lo, hi, q);
}

// pass A's rule: true when nothing inside a box at squared distance d2 can improve on best
__device__ __forceinline__ bool cannot_improve(double d2, double best) { return d2 * BOX_SHRINK > best || !(d2 < INFINITY); }

// MeshSDF._segment_d2
__device__ __forceinline__ double segment_d2(V3 p, V3 a, V3 ab) {
    double t = dot(p - a, ab) / fmax(dot(ab, ab), 1e-300);
    t = fmin(fmax(t, 0.0), 1.0);
    const V3 d = {p.x - (a.x + t * ab.x), p.y - (a.y + t * ab.y), p.z - (a.z + t * ab.z)};
    return dot(d, d);
}

// squared distance of p to the triangle a b c, as MeshSDF.__call__ forms it
__device__ __forceinline__ double triangle_d2(V3 p, V3 a, V3 b, V3 c) {
    const V3 ab = b - a, bc = c - b, ca = a - c;
    const V3 n = cross(ab, c - a);
    const V3 ap = p - a, bp = p - b, cp = p - c;
    const bool inside = dot(cross(ab, ap), n) >= 0.0 && dot(cross(bc, bp), n) >= 0.0 && dot(cross(ca, cp), n) >= 0.0;
    const double h = dot(ap, n);
    const double d_plane = h * h / dot(n, n);
    const double d_edge = fmin(fmin(segment_d2(p, a, ab), segment_d2(p, b, bc)), segment_d2(p, c, ca));
    return inside ? d_plane : d_edge;
}

// 2-D edge function of q against u -> v
__device__ __forceinline__ double edge_fn(V3 u, V3 v, V3 q) { return (v.x - u.x) * (q.y - u.y) - (v.y - u.y) * (q.x - u.x); }

// 1 when the ray q + t z, t > 0, crosses the triangle a b c (MeshSDF.__call__'s parity terms)
__device__ __forceinline__ int ray_crosses(V3 q, V3 a, V3 b, V3 c) {
    const double e0 = edge_fn(a, b, q), e1 = edge_fn(b, c, q), e2 = edge_fn(c, a, q);
    const bool covers = (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
    const double area2 = e0 + e1 + e2;
    const double z = (e1 * a.z + e2 * b.z + e0 * c.z) / (area2 == 0.0 ? 1.0 : area2);
    return covers && area2 != 0.0 && z > q.z;
}

// pass B's rule: may a face inside this box be crossed by the ray from q ?
__device__ __forceinline__ bool ray_may_cross(const double2 *__restrict__ node_box, int node, V3 q) {
    V3 lo, hi;
    load_box(node_box, node, lo, hi);
    return q.x >= lo.x && q.x <= hi.x && q.y >= lo.y && q.y <= hi.y && hi.z > q.z;
}

__global__ __launch_bounds__(BLOCK) void mesh_sdf_query_kernel(const double2 *__restrict__ node_box, int n_leaves,
                                                                const double *__restrict__ tris, int n_tris, int leaf_size,
                                                                const double *__restrict__ points, int64_t n_points,
                                                                int want_sign, double *__restrict__ out) {
    __shared__ int stack[STACK][BLOCK];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + tid;
    if (i >= n_points) return;
    const V3 q = load3(points + 3 * i);
    const int first_leaf = n_leaves - 1;

    // pass A
    double best = INFINITY;
    int sp = 0, node = 0;
    for (;;) {
        bool descend = false;
        if (node >= first_leaf) {
            const int f0 = (node - first_leaf) * leaf_size, f1 = min(f0 + leaf_size, n_tris);
            for (int f = f0; f < f1; ++f) {
                const double *t = tris + 9 * (size_t)f;
                best = fmin(best, triangle_d2(q, load3(t), load3(t + 3), load3(t + 6)));
            }
        } else {
            const int c0 = 2 * node + 1;
            const double d0 = node_d2(node_box, c0, q), d1 = node_d2(node_box, c0 + 1, q);
            const bool second = d1 < d0;
            const int near = second ? c0 + 1 : c0, far = second ? c0 : c0 + 1;
            if (!cannot_improve(second ? d1 : d0, best)) {
                if (!cannot_improve(second ? d0 : d1, best)) stack[sp++][tid] = far;
                node = near;
                descend = true;
            }
        }
        if (descend) continue;
        bool found = false;
        while (sp > 0) {
            const int c = stack[--sp][tid];
            if (!cannot_improve(node_d2(node_box, c, q), best)) {
                node = c;
                found = true;
                break;
            }
        }
        if (!found) break;
    }
    double d = sqrt(best);

    // pass B
    if (want_sign) {
        int crossings = 0;
        sp = 0;
        node = 0;
        bool live = ray_may_cross(node_box, 0, q);
        while (live) {
            bool descend = false;
            if (node >= first_leaf) {
                const int f0 = (node - first_leaf) * leaf_size, f1 = min(f0 + leaf_size, n_tris);
                for (int f = f0; f < f1; ++f) {
                    const double *t = tris + 9 * (size_t)f;
                    crossings += ray_crosses(q, load3(t), load3(t + 3), load3(t + 6));
                }
            } else {
                const int c0 = 2 * node + 1;
                const bool m0 = ray_may_cross(node_box, c0, q), m1 = ray_may_cross(node_box, c0 + 1, q);
                if (m0 && m1) stack[sp++][tid] = c0 + 1;
                if (m0 || m1) {
                    node = m0 ? c0 : c0 + 1;
                    descend = true;
                }
            }
            if (descend) continue;
            if (sp == 0) break;
            node = stack[--sp][tid];
        }
        if (crossings & 1) d = -d;
    }
    out[i] = d;
}

// ---- generalized winding number -----------------------------------------------------------------------
// w(q) = the sum over the faces of their signed solid angles seen from q, over 4 pi: 1 inside a closed outward-oriented mesh,
// 0 outside, 2 where two closed parts overlap, and smooth across a hole.  The sign it gives does not ask for a closed mesh.
//
// One thread per query, one depth-first traversal of the same tree, the left child first.  node_moment [2 N - 1][8] =
// (p.xyz, r, n.xyz, area) per node (mesh_bvh.py:build_moments): the dipole moment n of the node's faces about their
// area-weighted centre p, and a radius r within which every vertex of the node lies.  At a node:
//   area == 0                               empty: skipped;
//   a leaf                                  the exact solid angle of each of its faces is added (Van Oosterom & Strackee);
//   beta > 0 and |p - q|^2 > (beta r)^2     the dipole term n . d / |d|^3, d = p - q, is added; the node is not descended;
//   else                                    the left child is entered, the right one pushed.
// beta == 0 never approximates: the exact sum over all faces.  The order of the additions is fixed per query, so a query's
// result is the same bits from run to run and wherever it sits in the batch - but, a floating-point sum, NOT for another
// order of the faces (another tree, another order of additions), unlike the two results above.
//
// Workgroups of 64 threads: the stack is stack[27][64] ints, 6 912 bytes - against 27 648 for 256 threads - so the registers,
// not the LDS, bound the waves per SIMD, and a Step-1 batch of 16 384 queries is 256 workgroups, one per CU, instead of 64.
// A row of the stack is 64 dwords, one per bank.  Entering the left child directly, a path pushes one node per inner level,
// 26 at the most; popping a node and pushing both its children would need 27, which is what the array holds.
constexpr int WBLOCK = 64;
constexpr int WSTACK = STACK + 1;

// signed solid angle of the triangle A B C (corners relative to the query): 2 atan2(A . (B x C), |A||B||C| + (A.B)|C| +
// (B.C)|A| + (C.A)|B|).  Finite for every finite input: atan2(0, 0) = 0 on a vertex, +-pi in the face's plane inside it.
__device__ __forceinline__ double solid_angle(V3 A, V3 B, V3 C) {
    const double la = sqrt(dot(A, A)), lb = sqrt(dot(B, B)), lc = sqrt(dot(C, C));
    const double num = dot(A, cross(B, C));
    const double den = la * lb * lc + dot(A, B) * lc + dot(B, C) * la + dot(C, A) * lb;
    return 2.0 * atan2(num, den);
}

__global__ __launch_bounds__(WBLOCK) void mesh_winding_query_kernel(const double2 *__restrict__ node_moment, int n_leaves,
                                                                     const double *__restrict__ tris, int n_tris,
                                                                     int leaf_size, const double *__restrict__ points,
                                                                     int64_t n_points, double beta,
                                                                     double *__restrict__ out_w) {
    __shared__ int stack[WSTACK][WBLOCK];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * WBLOCK + tid;
    if (i >= n_points) return;
    const V3 q = load3(points + 3 * i);
    const int first_leaf = n_leaves - 1;
    double sum = 0.0;
    int sp = 0, node = 0;
    for (;;) {
        bool descend = false;
        if (node >= first_leaf) {
            const int f0 = (node - first_leaf) * leaf_size, f1 = min(f0 + leaf_size, n_tris);
            for (int f = f0; f < f1; ++f) {
                const double *t = tris + 9 * (size_t)f;
                sum += solid_angle(load3(t) - q, load3(t + 3) - q, load3(t + 6) - q);
            }
        } else {
            const double2 *m = node_moment + 4 * (size_t)node;
            const double2 m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3];
            if (m3.y != 0.0) {                                              // area: 0 marks an empty node
                const V3 d = {m0.x - q.x, m0.y - q.y, m1.x - q.z};
                const double dd = dot(d, d), br = beta * m1.y;
                if (beta > 0.0 && dd > br * br) {
                    const V3 n = {m2.x, m2.y, m3.x};
                    sum += dot(n, d) / (dd * sqrt(dd));
                } else {
                    stack[sp++][tid] = 2 * node + 2;
                    node = 2 * node + 1;
                    descend = true;
                }
            }
        }
        if (descend) continue;
        if (sp == 0) break;
        node = stack[--sp][tid];
    }
    out_w[i] = sum / (4.0 * M_PI);
}

}  // namespace

extern "C" int nefii_mesh_winding_query(const double *node_box, const double *node_moment, int64_t n_leaves_pow2,
                                        const double *tris, int64_t n_tris, int leaf_size, const double *points,
                                        int64_t n_points, double beta, double *out_w, void *stream) {
    if (!node_box || !node_moment || !tris || !points || !out_w) return NEFII_E_ARG;
    if (((uintptr_t)node_box & 15) != 0 || ((uintptr_t)node_moment & 15) != 0) return NEFII_E_ARG;
    if (!(beta >= 0.0) || (beta > 0.0 && beta < 1.0)) return NEFII_E_ARG;          // NaN, negative, inside the bounding sphere
    if (n_tris < 1 || n_tris > MAX_TRIS) return NEFII_E_SHAPE;
    if (leaf_size < 1 || leaf_size > MAX_LEAF) return NEFII_E_SHAPE;
    if (n_leaves_pow2 < 1 || n_leaves_pow2 > MAX_LEAVES || (n_leaves_pow2 & (n_leaves_pow2 - 1)) != 0) return NEFII_E_SHAPE;
    if (n_leaves_pow2 * leaf_size < n_tris) return NEFII_E_SHAPE;
    if (n_points < 0 || n_points > 0x7fffffffll) return NEFII_E_SHAPE;
    if (n_points == 0) return 0;
    // the boxes are part of the tree's description and are held to its alignment; the traversal reads the moments only (r
    // already bounds the node about p)
    const unsigned grid = (unsigned)((n_points + WBLOCK - 1) / WBLOCK);
    hipLaunchKernelGGL(mesh_winding_query_kernel, dim3(grid), dim3(WBLOCK), 0, (hipStream_t)stream,
                       (const double2 *)node_moment, (int)n_leaves_pow2, tris, (int)n_tris, leaf_size, points, n_points, beta,
                       out_w);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_mesh_sdf_query(const double *node_box, int64_t n_leaves_pow2, const double *tris, int64_t n_tris,
                                    int leaf_size, const double *points, int64_t n_points, int want_sign, double *out,
                                    void *stream) {
    if (!node_box || !tris || !points || !out) return NEFII_E_ARG;
    if (((uintptr_t)node_box & 15) != 0) return NEFII_E_ARG;                       // boxes are read as 16-byte pairs
    if (n_tris < 1 || n_tris > MAX_TRIS) return NEFII_E_SHAPE;
    if (leaf_size < 1 || leaf_size > MAX_LEAF) return NEFII_E_SHAPE;
    if (n_leaves_pow2 < 1 || n_leaves_pow2 > MAX_LEAVES || (n_leaves_pow2 & (n_leaves_pow2 - 1)) != 0) return NEFII_E_SHAPE;
    if (n_leaves_pow2 * leaf_size < n_tris) return NEFII_E_SHAPE;
    if (n_points < 0 || n_points > 0x7fffffffll) return NEFII_E_SHAPE;
    if (n_points == 0) return 0;
    const unsigned grid = (unsigned)((n_points + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(mesh_sdf_query_kernel, dim3(grid), dim3(BLOCK), 0, (hipStream_t)stream, (const double2 *)node_box,
                       (int)n_leaves_pow2, tris, (int)n_tris, leaf_size, points, n_points, want_sign, out);
    HIP_CHECK_LAUNCH();
    return 0;
}
