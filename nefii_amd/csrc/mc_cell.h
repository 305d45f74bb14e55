// mc_cell.h - what the dense and the sparse marching cubes (nefii_mcubes.hip, nefii_mcubes_sparse.hip) share: the workgroup
// shape, the ballot ranks, the count-pair reduction, the position of an edge's vertex, the decoding of a triangle-table
// entry and the host's finite check.  The sparse export is bitwise the dense one because both call these, not copies.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#define NEFII_MC_STORAGE __constant__ static const
#include "mc_tables.h"

constexpr int MC_THREADS = 256;                 // workgroup size of every counting and emitting pass
constexpr int MC_WAVES = MC_THREADS / 64;

// exclusive prefix over the workgroup of x in [0, 2^BITS), and the workgroup's total (one ballot per bit)
template <int BITS>
__device__ inline int block_rank(int x, int *wave_tot, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int pre = 0, wsum = 0;
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        const unsigned long long m = __ballot((x >> b) & 1);
        pre += __popcll(m & lt) << b;
        wsum += __popcll(m) << b;
    }
    __syncthreads();                            // the previous call's totals are read
    if (lane == 0) wave_tot[wave] = wsum;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < MC_WAVES; ++w) {
        const int t = wave_tot[w];
        before += w < wave ? t : 0;
        total += t;
    }
    return before + pre;
}

// the workgroup's sums of the (vertex, triangle) counts nv, nt, left in them on thread 0 - true there alone
__device__ inline bool block_sum_pair(int &nv, int &nt, int (*red)[MC_WAVES]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nv += __shfl_xor(nv, o);
        nt += __shfl_xor(nt, o);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = nv;
        red[1][threadIdx.x >> 6] = nt;
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    nv = nt = 0;
    for (int w = 0; w < MC_WAVES; ++w) {
        nv += red[0][w];
        nt += red[1][w];
    }
    return true;
}

// the vertex on the edge along axis a of grid point (fx, fy, fz), whose ends hold v0 (at the point) and v1: fp32, this
// operation order, no fused multiply-add (-ffp-contract=off) - the bits of ABI 17 (tests/mc_ref.py states them again)
__device__ inline float3 edge_vertex(int a, float fx, float fy, float fz, float v0, float v1, float level, float3 o,
                                     float3 s) {
    const float t = (level - v0) / (v1 - v0);
    return make_float3(o.x + (a == 0 ? fx + t : fx) * s.x, o.y + (a == 1 ? fy + t : fy) * s.y,
                       o.z + (a == 2 ? fz + t : fz) * s.z);
}

// table entry e of the cell anchored at (ix, iy, iz): the edge's axis a and its lower corner (qx, qy, qz), the grid point
// that owns its vertex.  e = 4 a + the corner's offsets along the two other axes (lower axis in bit 0)
__device__ inline void edge_owner(int e, int ix, int iy, int iz, int &a, int &qx, int &qy, int &qz) {
    a = e >> 2;
    const int o0 = e & 1, o1 = (e & 3) >> 1;
    qx = ix + (a == 0 ? 0 : o0);
    qy = iy + (a == 1 ? 0 : (a == 0 ? o0 : o1));
    qz = iz + (a == 2 ? 0 : o1);
}

inline bool mc_placement_finite(float level, float ox, float oy, float oz, float sx, float sy, float sz) {
    return isfinite(level) && isfinite(ox) && isfinite(oy) && isfinite(oz) && isfinite(sx) && isfinite(sy) && isfinite(sz);
}
