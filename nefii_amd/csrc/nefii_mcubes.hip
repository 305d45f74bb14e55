// ================================================================================================
// nefii_mcubes.hip - marching cubes over a dense fp32 volume, welded vertices, deterministic output order.
//
//   reference path  utils/plots.py get_surface_trace / get_surface_high_res_mesh (skimage marching_cubes_lewiner)
//
// vol[nx][ny][nz] (C order, z fastest); grid point p = (ix * ny + iy) * nz + iz; inside when v < level.  Every crossing
// grid edge carries one vertex, owned by its lower grid point and numbered by (owner p, axis x < y < z); triangles come
// in cell order (a cell is named by its lower grid point), then in table order (mc_tables.h).
//
// Each workgroup owns MC_TILE consecutive grid points; thread t handles points tile0 + k * MC_THREADS + t, k < MC_ITEMS,
// so every load of a wave is one contiguous run along z.  Four launches, all stream-ordered:
//   mc_count_kernel   pass 1: per point, the crossing edges it owns (0..3) and the triangles of the cell it anchors
//                     (0..5); one (vertex, triangle) count pair per workgroup.
//   mc_scan_kernel    one workgroup: exclusive prefix of the pairs (int64) and the totals (n_verts, n_tris).
//   mc_verts_kernel   pass 2: recomputes the edge crossings, ranks them within the workgroup (ballot / popcount per
//                     count bit), writes the vertices and vbase[p], the index of the first vertex p owns.
//   mc_faces_kernel   pass 3: recomputes the case, ranks the triangles the same way and writes them; an edge's vertex is
//                     vbase[owner] + the owner's crossing edges along lower axes, so edges owned by points of other
//                     workgroups resolve through vbase alone.
// Ranks come from ballots and a fixed workgroup-then-tile order: no atomics, bitwise identical output run to run.
// The ranks, the vertex expression and the table decoding are mc_cell.h's, shared with nefii_mcubes_sparse.hip.
#include "../../include/nefii_amd.h"
#include "mc_cell.h"

#include "hip_check.h"

namespace {

constexpr int MC_ITEMS = 8;                     // grid points per thread
constexpr int MC_TILE = MC_THREADS * MC_ITEMS;  // grid points per workgroup
constexpr int SCAN_THREADS = 1024;

struct Grid {
    int nx, ny, nz;
    int n;              // nx * ny * nz < 2^31
    float level;
};

__device__ inline void coords(const Grid &g, int p, int &ix, int &iy, int &iz) {
    const unsigned up = (unsigned)p;
    iz = (int)(up % (unsigned)g.nz);
    const unsigned r = up / (unsigned)g.nz;
    iy = (int)(r % (unsigned)g.ny);
    ix = (int)(r / (unsigned)g.ny);
}

// bit a: the edge of grid point p along axis a crosses the level (and exists)
__device__ inline int edge_mask(const float *__restrict__ vol, const Grid &g, int p, int ix, int iy, int iz) {
    const bool in0 = vol[p] < g.level;
    int m = 0;
    if (ix + 1 < g.nx) m |= (int)((vol[p + g.ny * g.nz] < g.level) != in0);
    if (iy + 1 < g.ny) m |= (int)((vol[p + g.nz] < g.level) != in0) << 1;
    if (iz + 1 < g.nz) m |= (int)((vol[p + 1] < g.level) != in0) << 2;
    return m;
}

// case index of the cell anchored at p (0 when p anchors no cell)
__device__ inline int cell_case(const float *__restrict__ vol, const Grid &g, int p, int ix, int iy, int iz) {
    if (ix + 1 >= g.nx || iy + 1 >= g.ny || iz + 1 >= g.nz) return 0;
    const int sx = g.ny * g.nz, sy = g.nz;
    int c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) c |= (int)(vol[p + (k & 1) * sx + ((k >> 1) & 1) * sy + ((k >> 2) & 1)] < g.level) << k;
    return c;
}

__global__ __launch_bounds__(MC_THREADS) void mc_count_kernel(const float *__restrict__ vol, Grid g,
                                                              int2 *__restrict__ blk_cnt) {
    __shared__ int red[2][MC_WAVES];
    const int tile0 = blockIdx.x * MC_TILE;
    int nv = 0, nt = 0;
#pragma unroll 2
    for (int k = 0; k < MC_ITEMS; ++k) {
        const int p = tile0 + k * MC_THREADS + (int)threadIdx.x;
        if (p < g.n) {
            int ix, iy, iz;
            coords(g, p, ix, iy, iz);
            nv += __popc(edge_mask(vol, g, p, ix, iy, iz));
            nt += nefii_mc_ntri[cell_case(vol, g, p, ix, iy, iz)];
        }
    }
    if (block_sum_pair(nv, nt, red)) blk_cnt[blockIdx.x] = make_int2(nv, nt);
}

__global__ __launch_bounds__(SCAN_THREADS) void mc_scan_kernel(const int2 *__restrict__ blk_cnt, int nblk,
                                                               long long *__restrict__ blk_off,
                                                               long long *__restrict__ counts) {
    __shared__ long long sv[SCAN_THREADS], st[SCAN_THREADS];
    const int tid = threadIdx.x;
    const int per = (nblk + SCAN_THREADS - 1) / SCAN_THREADS;
    const int b0 = min(tid * per, nblk), b1 = min(b0 + per, nblk);
    long long v = 0, t = 0;
    for (int b = b0; b < b1; ++b) {
        const int2 c = blk_cnt[b];
        v += c.x;
        t += c.y;
    }
    sv[tid] = v;
    st[tid] = t;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {        // inclusive scan of the per-thread sums
        const long long a = tid >= d ? sv[tid - d] : 0, c = tid >= d ? st[tid - d] : 0;
        __syncthreads();
        sv[tid] += a;
        st[tid] += c;
        __syncthreads();
    }
    long long ev = sv[tid] - v, et = st[tid] - t;
    for (int b = b0; b < b1; ++b) {
        const int2 c = blk_cnt[b];
        blk_off[2 * (long long)b] = ev;
        blk_off[2 * (long long)b + 1] = et;
        ev += c.x;
        et += c.y;
    }
    if (tid == SCAN_THREADS - 1) {
        counts[0] = sv[tid];
        counts[1] = st[tid];
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_verts_kernel(const float *__restrict__ vol, Grid g, float ox, float oy,
                                                              float oz, float sx, float sy, float sz,
                                                              const long long *__restrict__ blk_off,
                                                              int *__restrict__ vbase, float *__restrict__ verts,
                                                              long long max_verts) {
    __shared__ int wave_tot[MC_WAVES];
    const int tile0 = blockIdx.x * MC_TILE;
    long long carry = blk_off[2 * (long long)blockIdx.x];
    for (int k = 0; k < MC_ITEMS; ++k) {
        const int p = tile0 + k * MC_THREADS + (int)threadIdx.x;
        int ix = 0, iy = 0, iz = 0, m = 0;
        if (p < g.n) {
            coords(g, p, ix, iy, iz);
            m = edge_mask(vol, g, p, ix, iy, iz);
        }
        int total;
        const int rank = block_rank<2>(__popc(m), wave_tot, total);
        if (p < g.n) {
            long long vi = carry + rank;
            vbase[p] = (int)vi;
            if (m) {
                const float v0 = vol[p];
                const float fx = (float)ix, fy = (float)iy, fz = (float)iz;
                const int stride[3] = {g.ny * g.nz, g.nz, 1};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if (!((m >> a) & 1) || vi >= max_verts) continue;
                    const float3 x = edge_vertex(a, fx, fy, fz, v0, vol[p + stride[a]], g.level, make_float3(ox, oy, oz),
                                                 make_float3(sx, sy, sz));
                    float *o = verts + 3 * vi;
                    o[0] = x.x, o[1] = x.y, o[2] = x.z;
                    ++vi;
                }
            }
        }
        carry += total;
    }
}

// does the edge of grid point (qx, qy, qz) = linear q along `axis` cross?
__device__ inline int crosses(const float *__restrict__ vol, const Grid &g, int q, int qx, int qy, int qz, int axis) {
    const int lim = axis == 0 ? g.nx : (axis == 1 ? g.ny : g.nz);
    const int c = axis == 0 ? qx : (axis == 1 ? qy : qz);
    if (c + 1 >= lim) return 0;
    const int s = axis == 0 ? g.ny * g.nz : (axis == 1 ? g.nz : 1);
    return (int)((vol[q] < g.level) != (vol[q + s] < g.level));
}

__global__ __launch_bounds__(MC_THREADS) void mc_faces_kernel(const float *__restrict__ vol, Grid g,
                                                              const long long *__restrict__ blk_off,
                                                              const int *__restrict__ vbase, int *__restrict__ faces,
                                                              long long max_tris) {
    __shared__ int wave_tot[MC_WAVES];
    const int tile0 = blockIdx.x * MC_TILE;
    long long carry = blk_off[2 * (long long)blockIdx.x + 1];
    for (int k = 0; k < MC_ITEMS; ++k) {
        const int p = tile0 + k * MC_THREADS + (int)threadIdx.x;
        int ix = 0, iy = 0, iz = 0, c = 0;
        if (p < g.n) {
            coords(g, p, ix, iy, iz);
            c = cell_case(vol, g, p, ix, iy, iz);
        }
        const int nt = nefii_mc_ntri[c];
        int total;
        const int rank = block_rank<3>(nt, wave_tot, total);
        if (nt && carry + rank + nt <= max_tris) {
            int *o = faces + 3 * (carry + rank);
            for (int j = 0; j < 3 * nt; ++j) {
                const int e = nefii_mc_tri[c][j];
                int a, qx, qy, qz;
                edge_owner(e, ix, iy, iz, a, qx, qy, qz);
                const int q = (qx * g.ny + qy) * g.nz + qz;
                int id = vbase[q];
                if (a >= 1) id += crosses(vol, g, q, qx, qy, qz, 0);
                if (a >= 2) id += crosses(vol, g, q, qx, qy, qz, 1);
                o[j] = id;
            }
        }
        carry += total;
    }
}

bool bad_shape(int nx, int ny, int nz) {
    return nx < 2 || ny < 2 || nz < 2 || (int64_t)nx * ny * nz >= ((int64_t)1 << 31);
}

int n_tiles(int nx, int ny, int nz) { return (int)(((int64_t)nx * ny * nz + MC_TILE - 1) / MC_TILE); }

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: vbase [n] int32 | blk_cnt [tiles] int2 | blk_off [tiles][2] int64
void carve(void *ws, int nx, int ny, int nz, int *&vbase, int2 *&blk_cnt, long long *&blk_off) {
    const size_t n = (size_t)nx * ny * nz;
    char *b = (char *)ws;
    vbase = (int *)b;
    blk_cnt = (int2 *)(b + align256(n * sizeof(int)));
    blk_off = (long long *)((char *)blk_cnt + align256((size_t)n_tiles(nx, ny, nz) * sizeof(int2)));
}

Grid make_grid(int nx, int ny, int nz, float level) {
    Grid g;
    g.nx = nx;
    g.ny = ny;
    g.nz = nz;
    g.n = nx * ny * nz;
    g.level = level;
    return g;
}

}  // namespace

extern "C" int64_t nefii_mcubes_workspace_bytes(int nx, int ny, int nz) {
    if (bad_shape(nx, ny, nz)) return 0;
    const size_t n = (size_t)nx * ny * nz, t = (size_t)n_tiles(nx, ny, nz);
    return (int64_t)(align256(n * sizeof(int)) + align256(t * sizeof(int2)) + t * 2 * sizeof(long long));
}

extern "C" int nefii_mcubes_count(const float *vol, int nx, int ny, int nz, float level, void *workspace,
                                  int64_t *counts, void *stream) {
    if (!vol || !workspace || !counts || !isfinite(level)) return NEFII_E_ARG;
    if (bad_shape(nx, ny, nz)) return NEFII_E_SHAPE;
    int *vbase;
    int2 *blk_cnt;
    long long *blk_off;
    carve(workspace, nx, ny, nz, vbase, blk_cnt, blk_off);
    const Grid g = make_grid(nx, ny, nz, level);
    const int tiles = n_tiles(nx, ny, nz);
    hipLaunchKernelGGL(mc_count_kernel, dim3(tiles), dim3(MC_THREADS), 0, (hipStream_t)stream, vol, g, blk_cnt);
    HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)stream, blk_cnt, tiles, blk_off,
                       (long long *)counts);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_mcubes_emit(const float *vol, int nx, int ny, int nz, float level, float origin_x, float origin_y,
                                 float origin_z, float spacing_x, float spacing_y, float spacing_z, void *workspace,
                                 float *verts, int64_t max_verts, int *faces, int64_t max_tris, void *stream) {
    if (!vol || !workspace || !verts || !faces) return NEFII_E_ARG;
    if (!mc_placement_finite(level, origin_x, origin_y, origin_z, spacing_x, spacing_y, spacing_z)) return NEFII_E_ARG;
    if (max_verts < 0 || max_tris < 0) return NEFII_E_ARG;
    if (bad_shape(nx, ny, nz)) return NEFII_E_SHAPE;
    int *vbase;
    int2 *blk_cnt;
    long long *blk_off;
    carve(workspace, nx, ny, nz, vbase, blk_cnt, blk_off);
    const Grid g = make_grid(nx, ny, nz, level);
    const int tiles = n_tiles(nx, ny, nz);
    hipLaunchKernelGGL(mc_verts_kernel, dim3(tiles), dim3(MC_THREADS), 0, (hipStream_t)stream, vol, g, origin_x,
                       origin_y, origin_z, spacing_x, spacing_y, spacing_z, blk_off, vbase, verts, (long long)max_verts);
    HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(mc_faces_kernel, dim3(tiles), dim3(MC_THREADS), 0, (hipStream_t)stream, vol, g, blk_off, vbase,
                       faces, (long long)max_tris);
    HIP_CHECK_LAUNCH();
    return 0;
}
