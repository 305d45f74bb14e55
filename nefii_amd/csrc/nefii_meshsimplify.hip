// nefii_meshsimplify.hip - the representative vertex of every cluster of a vertex-clustering simplification, as the
// Tikhonov-regularised minimiser of the cluster's quadric error (Lindstrom 2000, "Out-of-core simplification of large
// polygonal models").  The clustering, the corner sort and the face bookkeeping are torch code
// (nefii_amd/mesh.py); this file holds the one pass over the geometry.
//
// A corner is t = 3 face + k.  `corners` lists all 3 F of them sorted (stably) by the cluster of the corner's vertex, and
// seg[c] .. seg[c + 1] is cluster c's run in that list.  GROUP = 8 consecutive lanes own one cluster: lane j takes the
// run's entries j, j + 8, j + 16, ... in that order into 12 fp64 sums (the 6 distinct entries of A, b, s), then a fixed
// xor tree over the 8 lanes (distances 1, 2, 4) adds them up.  The order of every addition is therefore a function of
// the run alone: no float atomics, and nothing depends on the launch geometry beyond "8 lanes of one wave".  A run of
// thousands of corners is walked by the same 8 lanes, only longer.
//
// Everything is fp64 in the cluster's local coordinates p' = (p - centre_c) / h; the position is rounded to fp32 once.
// This file is compiled without fp contraction (build.py), so a x a is exactly 0 and a face with a repeated vertex has
// exactly zero area.
//
// Bad input never leads an access astray: every index is compared with its range before it is used, a corner that fails
// is skipped, and the failure is recorded in flags (vector stores of the constant 1).
#include <hip/hip_runtime.h>
#include "../../include/nefii_amd.h"

#include "hip_check.h"

namespace {

constexpr int BLOCK = 256;
constexpr int GROUP = 8;                             // lanes per cluster: a typical run holds a few dozen corners
constexpr int CLUSTERS_PER_BLOCK = BLOCK / GROUP;
constexpr int64_t MAX_COUNT = 0x7fffffffll;          // n_verts, n_faces, n_clusters < 2^31
constexpr int N_SUMS = 12;                           // A00 A01 A02 A11 A12 A22 | b0 b1 b2 | s0 s1 s2

__global__ void simplify_clear_kernel(int *__restrict__ flags) {
    flags[0] = 0;
    flags[1] = 0;
}

// one thread per face: every index in [0, V), and every vertex a face uses in a cluster in [0, C)
__global__ __launch_bounds__(BLOCK) void simplify_validate_kernel(const int *__restrict__ faces, int64_t n_faces,
                                                                   const int *__restrict__ cluster, int n_verts,
                                                                   int n_clusters, int *__restrict__ flags) {
    const int64_t f = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    for (int k = 0; k < 3; ++k) {
        const int v = faces[3 * f + k];
        if ((unsigned)v >= (unsigned)n_verts) {      // negative indices wrap above V
            flags[0] = 1;
        } else if ((unsigned)cluster[v] >= (unsigned)n_clusters) {
            flags[1] = 1;
        }
    }
}

__global__ __launch_bounds__(BLOCK) void simplify_quadrics_kernel(
    const float *__restrict__ verts, int n_verts, const int *__restrict__ faces, int64_t n_faces,
    const int *__restrict__ cluster, const int *__restrict__ corners, const int64_t *__restrict__ seg,
    const double *__restrict__ centre, int n_clusters, double h, double eps, double clamp, float *__restrict__ pos,
    int *__restrict__ flags) {
    const int64_t c = (int64_t)blockIdx.x * CLUSTERS_PER_BLOCK + threadIdx.x / GROUP;
    const int lane = threadIdx.x % GROUP;
    const bool active = c < n_clusters;              // the whole group shares c: a group is active or idle as one
    const int64_t n_corners = 3 * n_faces;

    double sum[N_SUMS];
    for (int i = 0; i < N_SUMS; ++i) sum[i] = 0.0;
    double cx = 0.0, cy = 0.0, cz = 0.0;
    int64_t lo = 0, hi = 0;
    if (active) {
        cx = centre[3 * c], cy = centre[3 * c + 1], cz = centre[3 * c + 2];
        lo = seg[c], hi = seg[c + 1];
        if (lo < 0 || hi < lo || hi > n_corners) {   // not a run of the corner list: treated as empty
            if (lane == 0) flags[1] = 1;
            lo = hi = 0;
        }
    }
    const double inv_h = 1.0 / h;
    bool bad_index = false, bad_cluster = false;
    for (int64_t i = lo + lane; i < hi; i += GROUP) {
        const int t = corners[i];
        if ((unsigned)t >= (uint64_t)n_corners) {
            bad_index = true;
            continue;
        }
        const int f = t / 3, k = t - 3 * f;
        const int i0 = faces[3 * (int64_t)f], i1 = faces[3 * (int64_t)f + 1], i2 = faces[3 * (int64_t)f + 2];
        if ((unsigned)i0 >= (unsigned)n_verts || (unsigned)i1 >= (unsigned)n_verts || (unsigned)i2 >= (unsigned)n_verts) {
            bad_index = true;
            continue;
        }
        const int iv = k == 0 ? i0 : (k == 1 ? i1 : i2);
        if (cluster[iv] != (int)c) {                 // the corner list does not belong to this clustering
            bad_cluster = true;
            continue;
        }
        const double a0x = ((double)verts[3 * (int64_t)i0] - cx) * inv_h, a0y = ((double)verts[3 * (int64_t)i0 + 1] - cy) * inv_h,
                     a0z = ((double)verts[3 * (int64_t)i0 + 2] - cz) * inv_h;
        const double a1x = ((double)verts[3 * (int64_t)i1] - cx) * inv_h, a1y = ((double)verts[3 * (int64_t)i1 + 1] - cy) * inv_h,
                     a1z = ((double)verts[3 * (int64_t)i1 + 2] - cz) * inv_h;
        const double a2x = ((double)verts[3 * (int64_t)i2] - cx) * inv_h, a2y = ((double)verts[3 * (int64_t)i2 + 1] - cy) * inv_h,
                     a2z = ((double)verts[3 * (int64_t)i2 + 2] - cz) * inv_h;
        sum[9] += k == 0 ? a0x : (k == 1 ? a1x : a2x);
        sum[10] += k == 0 ? a0y : (k == 1 ? a1y : a2y);
        sum[11] += k == 0 ? a0z : (k == 1 ? a1z : a2z);
        const double ux = a1x - a0x, uy = a1y - a0y, uz = a1z - a0z;
        const double vx = a2x - a0x, vy = a2y - a0y, vz = a2z - a0z;
        const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
        const double len = sqrt(nx * nx + ny * ny + nz * nz);
        if (!(len > 0.0) || !(len < INFINITY)) continue;             // zero area (or non-finite input): s only
        const double w = 0.5 * len;                                  // area / h^2
        const double ex = nx / len, ey = ny / len, ez = nz / len;    // the unit normal
        const double d = -(ex * a0x + ey * a0y + ez * a0z);
        sum[0] += w * ex * ex, sum[1] += w * ex * ey, sum[2] += w * ex * ez;
        sum[3] += w * ey * ey, sum[4] += w * ey * ez, sum[5] += w * ez * ez;
        sum[6] += w * d * ex, sum[7] += w * d * ey, sum[8] += w * d * ez;
    }
    if (bad_index) flags[0] = 1;
    if (bad_cluster) flags[1] = 1;

    // the fixed tree: every lane of the wave takes part (idle groups add zeros), after it all 8 lanes hold the total
    for (int dist = 1; dist < GROUP; dist <<= 1)
        for (int i = 0; i < N_SUMS; ++i) sum[i] += __shfl_xor(sum[i], dist, GROUP);

    if (!active || lane != 0) return;
    const int64_t m = hi - lo;
    double x = 0.0, y = 0.0, z = 0.0;                // an empty run: the cell's centre
    if (m > 0) {
        const double x0 = sum[9] / (double)m, y0 = sum[10] / (double)m, z0 = sum[11] / (double)m;
        x = x0, y = y0, z = z0;
        const double trace = sum[0] + sum[3] + sum[5];
        if (trace > 0.0) {
            const double lam = eps * trace;
            const double m00 = sum[0] + lam, m10 = sum[1], m20 = sum[2], m11 = sum[3] + lam, m21 = sum[4], m22 = sum[5] + lam;
            const double r0 = -(sum[6] + (sum[0] * x0 + sum[1] * y0 + sum[2] * z0));
            const double r1 = -(sum[7] + (sum[1] * x0 + sum[3] * y0 + sum[4] * z0));
            const double r2 = -(sum[8] + (sum[2] * x0 + sum[4] * y0 + sum[5] * z0));
            // Cholesky M = L L^T; a pivot that is not positive (eps == 0 on a rank-deficient A, or overflow) keeps x0
            const double p0 = m00;
            const double l00 = sqrt(p0), l10 = m10 / l00, l20 = m20 / l00;
            const double p1 = m11 - l10 * l10;
            const double l11 = sqrt(p1), l21 = (m21 - l20 * l10) / l11;
            const double p2 = m22 - l20 * l20 - l21 * l21;
            const double l22 = sqrt(p2);
            if (p0 > 0.0 && p1 > 0.0 && p2 > 0.0) {
                const double f0 = r0 / l00, f1 = (r1 - l10 * f0) / l11, f2 = (r2 - l20 * f0 - l21 * f1) / l22;
                const double dz = f2 / l22, dy = (f1 - l21 * dz) / l11, dx = (f0 - l10 * dy - l20 * dz) / l00;
                if (fabs(dx) < INFINITY && fabs(dy) < INFINITY && fabs(dz) < INFINITY) x = x0 + dx, y = y0 + dy, z = z0 + dz;
            }
        }
        x = fmin(fmax(x, -clamp), clamp), y = fmin(fmax(y, -clamp), clamp), z = fmin(fmax(z, -clamp), clamp);
    }
    pos[3 * c] = (float)(cx + h * x);
    pos[3 * c + 1] = (float)(cy + h * y);
    pos[3 * c + 2] = (float)(cz + h * z);
}

}  // namespace

extern "C" int nefii_mesh_cluster_quadrics(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces,
                                           const int32_t *cluster, const int32_t *corners, const int64_t *seg,
                                           const double *centre, int64_t n_clusters, double h, double eps, double clamp,
                                           float *pos, int32_t *flags, void *stream) {
    if (!verts || !faces || !cluster || !corners || !seg || !centre || !pos || !flags) return NEFII_E_ARG;
    if (!(h > 0.0) || !(h < INFINITY) || !(eps >= 0.0) || !(eps < INFINITY) || !(clamp > 0.0) || !(clamp < INFINITY))
        return NEFII_E_ARG;
    if (n_verts < 0 || n_verts > MAX_COUNT || n_faces < 0 || n_faces > MAX_COUNT || n_clusters < 0 || n_clusters > MAX_COUNT)
        return NEFII_E_SHAPE;
    if (3 * n_faces > MAX_COUNT) return NEFII_E_SHAPE;           // a corner is an int32
    if (n_clusters == 0 || n_faces == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(simplify_clear_kernel, dim3(1), dim3(1), 0, s, flags);
    HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(simplify_validate_kernel, dim3((unsigned)((n_faces + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, faces,
                       n_faces, cluster, (int)n_verts, (int)n_clusters, flags);
    HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(simplify_quadrics_kernel, dim3((unsigned)((n_clusters + CLUSTERS_PER_BLOCK - 1) / CLUSTERS_PER_BLOCK)),
                       dim3(BLOCK), 0, s, verts, (int)n_verts, faces, n_faces, cluster, corners, seg, centre, (int)n_clusters,
                       h, eps, clamp, pos, flags);
    HIP_CHECK_LAUNCH();
    return 0;
}
