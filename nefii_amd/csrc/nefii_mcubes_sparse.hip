// ================================================================================================
// nefii_mcubes_sparse.hip - marching cubes over the bricks of a fine grid that an SDF interval grid cannot rule out
// (DESIGN.md 6f "Sparse export"; the dense kernels and every convention: nefii_mcubes.hip).
//
// The fine grid of nx x ny x nz points is cut into bricks of B cells per edge.  Two index spaces:
//   cell bricks   [cbx][cby][cbz], cb = ceil((n - 1) / B): brick (I, J, K) holds the cells anchored at grid points I B .. I B + B - 1
//                 (clipped to the grid).  Classification and the active set live here.
//   point bricks  [pbx][pby][pbz], pb = (n - 1) / B + 1: brick (I, J, K) OWNS the grid points I B .. I B + B - 1 (clipped), so
//                 every grid point has exactly one owner and pb = cb, or cb + 1 where the last plane starts a brick of its
//                 own.  Values are stored per evaluated point brick, B^3 floats at slot_map[brick] * B^3 + (lx B + ly) B + lz.
//
//   classify_thread_kernel / classify_wave_kernel   one byte per cell brick: may it hold a crossing?  The brick's 8 corner points
//                 (fp64, rounded once to fp32) give a world box, widened by one ulp of its largest coordinate; lo_b / hi_b are
//                 the least lo / greatest hi over the interval cells it overlaps.  A thread serves a brick where the host's
//                 bound on that count is small, a wave (lanes stride over the cells, shuffles reduce) where it is large;
//                 min and max are exact, so both give the same bytes.
//   smc_count_kernel   one workgroup per active cell brick: the (B+1)^3 corner values are gathered through slot_map into LDS;
//                 (crossing edges, triangles) per brick.
//   smc_emit_kernel    the same gather; ranks by ballots in a fixed order (no atomics: two runs are bitwise equal) and writes,
//                 per crossing edge of the brick's cells, the 64-bit key owner_linear * 3 + axis and the position
//                 (edge_vertex of mc_cell.h, the dense kernel's too), and per triangle the cell's linear index and three vertex keys.
//                 An edge on a face two active bricks share is written by both, from the same stored values - bit-equal
//                 copies that the caller's sort folds into one.
// ================================================================================================
#include "../../include/nefii_amd.h"
#include "mc_cell.h"

#include "hip_check.h"

namespace {

constexpr int SMC_MAX_B = 8;
constexpr int SMC_MAX_CORNERS = (SMC_MAX_B + 1) * (SMC_MAX_B + 1) * (SMC_MAX_B + 1);
constexpr int CLS_THREADS = 256;
constexpr int SMC_MAX_AXIS = 4096;

// ---- classification -------------------------------------------------------------------------------------------------------
struct BrickFrame {
    int nx, ny, nz;         // fine grid points
    int bx, by, bz;         // cell bricks
    int B, G;
    double p0[3];           // world position of grid point (0, 0, 0)
    double s[3][3];         // s[a]: world step of one grid index along axis a
    float radius, inv_h, level;
};

// the interval cells [c0, c1] per axis that brick b's widened box overlaps; false: the box leaves the cube (or is not finite)
__device__ inline bool brick_cells(const BrickFrame &f, int b, int c0[3], int c1[3]) {
    const int k = b % f.bz, r = b / f.bz;
    const int j = r % f.by, i = r / f.by;
    const int i0 = i * f.B, j0 = j * f.B, k0 = k * f.B;
    const int i1 = min(i0 + f.B, f.nx - 1), j1 = min(j0 + f.B, f.ny - 1), k1 = min(k0 + f.B, f.nz - 1);
    float lo[3], hi[3], m = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = __builtin_inff(), hi[a] = -__builtin_inff();
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const double di = (double)((c & 1) ? i1 : i0), dj = (double)((c & 2) ? j1 : j0), dk = (double)((c & 4) ? k1 : k0);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x = (float)(((f.p0[a] + di * f.s[0][a]) + dj * f.s[1][a]) + dk * f.s[2][a]);
            lo[a] = fminf(lo[a], x);
            hi[a] = fmaxf(hi[a], x);
            m = fmaxf(m, fabsf(x));
        }
    }
    const float u = nextafterf(m, __builtin_inff()) - m;        // one ulp of the largest coordinate
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = lo[a] - u, h = hi[a] + u;
        inside = inside && (l >= -f.radius) && (h <= f.radius);    // (NaN: outside)
        const float fl = (l + f.radius) * f.inv_h, fh = (h + f.radius) * f.inv_h;
        c0[a] = min(max((int)fl, 0), f.G - 1);
        c1[a] = min(max((int)fh, 0), f.G - 1);
    }
    return inside;
}

__device__ inline void fold_word(unsigned w, float &lo, float &hi, bool &bad) {
    const float l = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu));
    const float h = (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
    bad = bad || !isfinite(l) || !isfinite(h);
    lo = fminf(lo, l);
    hi = fmaxf(hi, h);
}

__global__ __launch_bounds__(CLS_THREADS) void classify_thread_kernel(const unsigned *__restrict__ cells, BrickFrame f,
                                                                      int n_bricks, unsigned char *__restrict__ out) {
    const int b = blockIdx.x * CLS_THREADS + (int)threadIdx.x;
    if (b >= n_bricks) return;
    int c0[3], c1[3];
    if (!brick_cells(f, b, c0, c1)) {
        out[b] = 1;
        return;
    }
    float lo = __builtin_inff(), hi = -__builtin_inff();
    bool bad = false;
    for (int x = c0[0]; x <= c1[0]; ++x)
        for (int y = c0[1]; y <= c1[1]; ++y) {
            const unsigned *row = cells + ((size_t)x * f.G + (size_t)y) * f.G;
            for (int z = c0[2]; z <= c1[2]; ++z) fold_word(row[z], lo, hi, bad);
        }
    out[b] = (bad || !(lo > f.level || hi < f.level)) ? 1 : 0;
}

__global__ __launch_bounds__(CLS_THREADS) void classify_wave_kernel(const unsigned *__restrict__ cells, BrickFrame f,
                                                                    int n_bricks, unsigned char *__restrict__ out) {
    // the brick is the wave's: its index, box and cell range are wave-uniform (scalar registers)
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x * (CLS_THREADS / 64) + ((int)threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    if (b >= n_bricks) return;
    int c0[3], c1[3];
    if (!brick_cells(f, b, c0, c1)) {
        if (lane == 0) out[b] = 1;
        return;
    }
    const int dy = c1[1] - c0[1] + 1, dz = c1[2] - c0[2] + 1;
    const int n = (c1[0] - c0[0] + 1) * dy * dz;                // <= G^3 <= 640^3 < 2^31
    float lo = __builtin_inff(), hi = -__builtin_inff();
    bool bad = false;
    for (int c = lane; c < n; c += 64) {
        const int z = c % dz, r = c / dz;
        const int y = r % dy, x = r / dy;
        fold_word(cells[((size_t)(c0[0] + x) * f.G + (size_t)(c0[1] + y)) * f.G + (size_t)(c0[2] + z)], lo, hi, bad);
    }
    int ibad = bad ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
        ibad |= __shfl_xor(ibad, o);
    }
    if (lane == 0) out[b] = (ibad || !(lo > f.level || hi < f.level)) ? 1 : 0;
}

// ---- sparse marching cubes ------------------------------------------------------------------------------------------------
struct SparseGrid {
    int nx, ny, nz;
    int B;
    int cbx, cby, cbz;      // cell bricks
    int pbx, pby, pbz;      // point bricks
    int n_slots;
    float level;
};

// the brick of this workgroup: false when the list entry names no brick.  (i0, j0, k0): its first grid point.
__device__ inline bool brick_origin(const SparseGrid &g, const int *__restrict__ active_list, int &i0, int &j0, int &k0) {
    const int b = active_list[blockIdx.x];
    if (b < 0 || b >= g.cbx * g.cby * g.cbz) return false;
    const int k = b % g.cbz, r = b / g.cbz;
    k0 = k * g.B;
    j0 = (r % g.cby) * g.B;
    i0 = (r / g.cby) * g.B;
    return true;
}

// corner values of the brick, (B+1)^3, into LDS; +inf for a point outside the grid or in a brick that was not evaluated
// (neither is ever read as a crossing: edges and cells are tested against the grid's shape first, and the caller
// evaluates every point brick an active cell brick touches)
__device__ inline void gather_corners(const float *__restrict__ vals, const int *__restrict__ slot_map, const SparseGrid &g,
                                      int i0, int j0, int k0, float *sv) {
    const int E = g.B + 1, n = E * E * E, B3 = g.B * g.B * g.B;
    for (int t = threadIdx.x; t < n; t += MC_THREADS) {
        const int k = t % E, r = t / E;
        const int j = r % E, i = r / E;
        const int gx = i0 + i, gy = j0 + j, gz = k0 + k;
        float v = __builtin_inff();
        if (gx < g.nx && gy < g.ny && gz < g.nz) {
            const int px = gx / g.B, py = gy / g.B, pz = gz / g.B;
            const int slot = slot_map[((size_t)px * g.pby + (size_t)py) * g.pbz + (size_t)pz];
            if (slot >= 0 && slot < g.n_slots)
                v = vals[(size_t)slot * B3 + (size_t)(((gx - px * g.B) * g.B + (gy - py * g.B)) * g.B + (gz - pz * g.B))];
        }
        sv[t] = v;
    }
    __syncthreads();
}

// item t of the brick: its local and global coordinates, the crossing edges it owns among the brick's cells (bit a: axis a)
// and the case of the cell it anchors (0: none)
struct Item {
    int gx, gy, gz, m, c;
};

__device__ inline Item brick_item(const SparseGrid &g, const float *sv, int i0, int j0, int k0, int t) {
    const int E = g.B + 1;
    Item it = {0, 0, 0, 0, 0};
    if (t >= E * E * E) return it;
    const int k = t % E, r = t / E;
    const int j = r % E, i = r / E;
    it.gx = i0 + i, it.gy = j0 + j, it.gz = k0 + k;
    if (it.gx >= g.nx || it.gy >= g.ny || it.gz >= g.nz) return it;
    const bool ex = i < g.B && it.gx + 1 < g.nx, ey = j < g.B && it.gy + 1 < g.ny, ez = k < g.B && it.gz + 1 < g.nz;
    const int sx = E * E, sy = E;
    const bool in0 = sv[t] < g.level;
    if (ex) it.m |= (int)((sv[t + sx] < g.level) != in0);
    if (ey) it.m |= (int)((sv[t + sy] < g.level) != in0) << 1;
    if (ez) it.m |= (int)((sv[t + 1] < g.level) != in0) << 2;
    if (ex && ey && ez) {
#pragma unroll
        for (int q = 0; q < 8; ++q) it.c |= (int)(sv[t + (q & 1) * sx + ((q >> 1) & 1) * sy + ((q >> 2) & 1)] < g.level) << q;
    }
    return it;
}

__global__ __launch_bounds__(MC_THREADS) void smc_count_kernel(const float *__restrict__ vals, const int *__restrict__ slot_map,
                                                                SparseGrid g, const int *__restrict__ active_list,
                                                                int *__restrict__ cnt) {
    __shared__ float sv[SMC_MAX_CORNERS];
    __shared__ int red[2][MC_WAVES];
    int i0 = 0, j0 = 0, k0 = 0;
    const bool ok = brick_origin(g, active_list, i0, j0, k0);       // workgroup-uniform
    int nv = 0, nt = 0;
    if (ok) {
        gather_corners(vals, slot_map, g, i0, j0, k0, sv);
        const int E = g.B + 1, n = E * E * E;
        for (int t = threadIdx.x; t < n; t += MC_THREADS) {
            const Item it = brick_item(g, sv, i0, j0, k0, t);
            nv += __popc(it.m);
            nt += nefii_mc_ntri[it.c];
        }
    }
    if (block_sum_pair(nv, nt, red)) {
        cnt[2 * (size_t)blockIdx.x] = nv;
        cnt[2 * (size_t)blockIdx.x + 1] = nt;
    }
}

__global__ __launch_bounds__(MC_THREADS) void smc_emit_kernel(const float *__restrict__ vals, const int *__restrict__ slot_map,
                                                               SparseGrid g, const int *__restrict__ active_list, float ox,
                                                               float oy, float oz, float spx, float spy, float spz,
                                                               const long long *__restrict__ off, long long *__restrict__ vkeys,
                                                               float *__restrict__ vpos, long long max_verts,
                                                               long long *__restrict__ fcell, long long *__restrict__ fkeys,
                                                               long long max_tris) {
    __shared__ float sv[SMC_MAX_CORNERS];
    __shared__ int wave_tot[MC_WAVES];
    int i0 = 0, j0 = 0, k0 = 0;
    if (!brick_origin(g, active_list, i0, j0, k0)) return;          // workgroup-uniform
    gather_corners(vals, slot_map, g, i0, j0, k0, sv);
    const int E = g.B + 1, n = E * E * E;
    const int sx = E * E, sy = E;
    long long vcarry = off[2 * (size_t)blockIdx.x], tcarry = off[2 * (size_t)blockIdx.x + 1];
    for (int t0 = 0; t0 < n; t0 += MC_THREADS) {
        const int t = t0 + (int)threadIdx.x;
        const Item it = brick_item(g, sv, i0, j0, k0, t);
        int vtotal, ttotal;
        const int vrank = block_rank<2>(__popc(it.m), wave_tot, vtotal);
        const int nt = nefii_mc_ntri[it.c];
        const int trank = block_rank<3>(nt, wave_tot, ttotal);
        const long long p = ((long long)it.gx * g.ny + it.gy) * g.nz + it.gz;
        if (it.m) {
            long long vi = vcarry + vrank;
            const float v0 = sv[t];
            const float fx = (float)it.gx, fy = (float)it.gy, fz = (float)it.gz;
            const int stride[3] = {sx, sy, 1};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!((it.m >> a) & 1) || vi >= max_verts) continue;
                const float3 x = edge_vertex(a, fx, fy, fz, v0, sv[t + stride[a]], g.level, make_float3(ox, oy, oz),
                                             make_float3(spx, spy, spz));
                float *o = vpos + 3 * vi;
                o[0] = x.x, o[1] = x.y, o[2] = x.z;
                vkeys[vi] = p * 3 + a;
                ++vi;
            }
        }
        if (nt && tcarry + trank + nt <= max_tris) {
            const long long ti = tcarry + trank;
            for (int q = 0; q < nt; ++q) fcell[ti + q] = p;
            long long *o = fkeys + 3 * ti;
            for (int jj = 0; jj < 3 * nt; ++jj) {
                const int e = nefii_mc_tri[it.c][jj];
                int a, qx, qy, qz;
                edge_owner(e, it.gx, it.gy, it.gz, a, qx, qy, qz);
                o[jj] = (((long long)qx * g.ny + qy) * g.nz + qz) * 3 + a;
            }
        }
        vcarry += vtotal;
        tcarry += ttotal;
    }
}

bool bad_sparse_shape(int nx, int ny, int nz, int B) {
    return nx < 2 || ny < 2 || nz < 2 || nx > SMC_MAX_AXIS || ny > SMC_MAX_AXIS || nz > SMC_MAX_AXIS || B < 2 || B > SMC_MAX_B;
}

int64_t n_cell_bricks(int nx, int ny, int nz, int B) {
    return (int64_t)((nx - 2) / B + 1) * ((ny - 2) / B + 1) * ((nz - 2) / B + 1);
}

SparseGrid make_sparse_grid(int nx, int ny, int nz, int B, int n_slots, float level) {
    SparseGrid g;
    g.nx = nx, g.ny = ny, g.nz = nz, g.B = B;
    g.cbx = (nx - 2) / B + 1, g.cby = (ny - 2) / B + 1, g.cbz = (nz - 2) / B + 1;
    g.pbx = (nx - 1) / B + 1, g.pby = (ny - 1) / B + 1, g.pbz = (nz - 1) / B + 1;
    g.n_slots = n_slots;
    g.level = level;
    return g;
}

}  // namespace

extern "C" int nefii_mcubes_classify_bricks(const void *cells, int G, float radius, int nx, int ny, int nz,
                                            const double *frame, float level, int B, uint8_t *out_active, void *stream) {
    if (!cells || !frame || !out_active || !isfinite(level) || !isfinite(radius) || !(radius > 0.f)) return NEFII_E_ARG;
    for (int q = 0; q < 12; ++q)
        if (!isfinite(frame[q])) return NEFII_E_ARG;
    if (G < 2 || G > NEFII_BOUND_GRID_MAX || bad_sparse_shape(nx, ny, nz, B)) return NEFII_E_SHAPE;
    const int64_t nb = n_cell_bricks(nx, ny, nz, B);
    if (nb >= ((int64_t)1 << 31)) return NEFII_E_SHAPE;
    BrickFrame f;
    f.nx = nx, f.ny = ny, f.nz = nz, f.B = B, f.G = G;
    f.bx = (nx - 2) / B + 1, f.by = (ny - 2) / B + 1, f.bz = (nz - 2) / B + 1;
    for (int a = 0; a < 3; ++a) {
        f.p0[a] = frame[a];
        for (int c = 0; c < 3; ++c) f.s[a][c] = frame[3 + 3 * a + c];
    }
    f.radius = radius;
    f.inv_h = (float)((double)G / (2.0 * (double)radius));
    f.level = level;
    // the most interval cells a brick can overlap: per world axis its extent is at most B (|s0| + |s1| + |s2|), and an
    // extent of e cells touches at most floor(e) + 2 of them (the ulp widening stays far inside the slack of 1e-3 cell)
    double cap = 1.0;
    for (int c = 0; c < 3; ++c) {
        const double ext = (double)B * (fabs(f.s[0][c]) + fabs(f.s[1][c]) + fabs(f.s[2][c])) * (double)f.inv_h;
        cap *= floor(ext + 1e-3) + 2.0;
    }
    if (cap <= 64.0) {
        const unsigned blocks = (unsigned)((nb + CLS_THREADS - 1) / CLS_THREADS);
        hipLaunchKernelGGL(classify_thread_kernel, dim3(blocks), dim3(CLS_THREADS), 0, (hipStream_t)stream,
                           (const unsigned *)cells, f, (int)nb, out_active);
    } else {
        const int per = CLS_THREADS / 64;
        const unsigned blocks = (unsigned)((nb + per - 1) / per);
        hipLaunchKernelGGL(classify_wave_kernel, dim3(blocks), dim3(CLS_THREADS), 0, (hipStream_t)stream,
                           (const unsigned *)cells, f, (int)nb, out_active);
    }
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_mcubes_sparse_count(const float *vals, const int *slot_map, int n_slots, int nx, int ny, int nz, int B,
                                         const int *active_list, int n_active, float level, int *counts, void *stream) {
    if (!vals || !slot_map || !active_list || !counts || !isfinite(level) || n_slots < 1 || n_active < 1) return NEFII_E_ARG;
    if (bad_sparse_shape(nx, ny, nz, B) || n_cell_bricks(nx, ny, nz, B) >= ((int64_t)1 << 31)) return NEFII_E_SHAPE;
    const SparseGrid g = make_sparse_grid(nx, ny, nz, B, n_slots, level);
    hipLaunchKernelGGL(smc_count_kernel, dim3(n_active), dim3(MC_THREADS), 0, (hipStream_t)stream, vals, slot_map, g,
                       active_list, counts);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_mcubes_sparse_emit(const float *vals, const int *slot_map, int n_slots, int nx, int ny, int nz, int B,
                                        const int *active_list, int n_active, float level, float origin_x, float origin_y,
                                        float origin_z, float spacing_x, float spacing_y, float spacing_z,
                                        const int64_t *offsets, int64_t *vert_keys, float *vert_pos, int64_t max_verts,
                                        int64_t *face_cell, int64_t *face_keys, int64_t max_tris, void *stream) {
    if (!vals || !slot_map || !active_list || !offsets || !vert_keys || !vert_pos || !face_cell || !face_keys ||
        n_slots < 1 || n_active < 1 || max_verts < 0 || max_tris < 0)
        return NEFII_E_ARG;
    if (!mc_placement_finite(level, origin_x, origin_y, origin_z, spacing_x, spacing_y, spacing_z)) return NEFII_E_ARG;
    if (bad_sparse_shape(nx, ny, nz, B) || n_cell_bricks(nx, ny, nz, B) >= ((int64_t)1 << 31)) return NEFII_E_SHAPE;
    const SparseGrid g = make_sparse_grid(nx, ny, nz, B, n_slots, level);
    hipLaunchKernelGGL(smc_emit_kernel, dim3(n_active), dim3(MC_THREADS), 0, (hipStream_t)stream, vals, slot_map, g,
                       active_list, origin_x, origin_y, origin_z, spacing_x, spacing_y, spacing_z,
                       (const long long *)offsets, (long long *)vert_keys, vert_pos, (long long)max_verts,
                       (long long *)face_cell, (long long *)face_keys, (long long)max_tris);
    HIP_CHECK_LAUNCH();
    return 0;
}
