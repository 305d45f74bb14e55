// nefii_metrics.hip - PSNR / SSIM / MS-SSIM statistics of image pairs in fp64 (Wang et al. 2003 / 2004 as
// scripts/evaluate.py restates them: 11-tap Gaussian window, 'valid' separable filtering, five scales with 2 x 2 average
// pooling between them).
//
// x, y: fp32 [B][H][W][C] (channels interleaved).  Everything after the load is fp64.  For a level image h x w:
//
//   mu1, mu2, e11, e22, e12 = the 11 x 11 separable 'valid' filterings of x, y, x x, y y, x y (along H, then along W)
//   s11 = e11 - mu1 mu1,  s22 = e22 - mu2 mu2,  s12 = e12 - mu1 mu2
//   cs   = (2 s12 + C2) / (s11 + s22 + C2)
//   ssim = (2 mu1 mu2 + C1) / (mu1 mu1 + mu2 mu2 + C1) cs
//   stats[b][level][c] = (mean ssim, mean cs) over the (h - 10) x (w - 10) valid positions
//
// and, from level 0, sq_err[b][c] = sum (x - y)^2 over all H W pixels.  Level l + 1 is the 2 x 2 average of level l with
// the divisor 4: an even side pairs the inputs (2 i, 2 i + 1), an odd side (2 i - 1, 2 i) with what lies outside read as 0
// (torch's avg_pool2d with padding = side % 2).  Levels 1 .. 4 are kept in fp64 in the workspace.
//
// Three kernels, one stream, no atomics:
//   level_kernel<T>  one workgroup = one TILE_H x TILE_W tile of valid positions of one channel of one image.  The two
//                    (TILE_H + 10) x (TILE_W + 10) input patches are staged in LDS as doubles (what lies outside the image
//                    is staged as 0 and only feeds positions that are not counted); the pass along H writes the five moment
//                    rows to LDS, the pass along W reads them; a thread forms ssim and cs of its two positions; the
//                    workgroup sums them, and the squared differences of the pixels the tile owns, by a tree in LDS and writes
//                    one slab of three doubles with plain stores.
//   pool_kernel<T>   one thread per element of the next level.
//   reduce_kernel    one workgroup per (level, image, channel): sums that entry's slabs in a fixed order, divides by the
//                    count.  The slab count depends on the shape alone: two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nefii_amd.h"

#include "hip_check.h"

namespace {

constexpr int WIN = 11, HALO = WIN - 1;
constexpr int TILE_W = 32, TILE_H = 16;             // valid positions of a workgroup
constexpr int PATCH_W = TILE_W + HALO, PATCH_H = TILE_H + HALO;
constexpr int THREADS = 256;                        // 32 x 8: a thread owns the positions (ty, tx) and (ty + 8, tx)
constexpr int MAX_SIDE = 16384, MAX_LEVELS = 5, MAX_BATCH = 65535;
constexpr int SLAB = 3;                             // doubles per tile: sum ssim, sum cs, sum of squared differences

struct Window {
    double g[WIN];
};

struct Plan {                                       // what the shape alone decides
    int levels;
    int h[MAX_LEVELS], w[MAX_LEVELS];
    int tiles_x[MAX_LEVELS], tiles[MAX_LEVELS];
    size_t image[MAX_LEVELS];                       // offset (doubles) of x's level in the workspace; y follows it (level 0: unused)
    size_t slabs[MAX_LEVELS];                       // offset (doubles) of the level's slabs
    size_t total;                                   // doubles
};

bool make_plan(int B, int H, int W, int C, int levels, Plan *p) {
    p->levels = levels;
    size_t at = 0;
    int h = H, w = W;
    for (int l = 0; l < levels; ++l) {
        if (h < WIN || w < WIN) return false;
        p->h[l] = h;
        p->w[l] = w;
        p->tiles_x[l] = (w - HALO + TILE_W - 1) / TILE_W;
        p->tiles[l] = p->tiles_x[l] * ((h - HALO + TILE_H - 1) / TILE_H);
        p->image[l] = at;
        if (l > 0) at += 2 * (size_t)B * h * w * C;
        h = (h + 1) / 2;
        w = (w + 1) / 2;
    }
    for (int l = 0; l < levels; ++l) {
        p->slabs[l] = at;
        at += (size_t)B * C * p->tiles[l] * SLAB;
    }
    p->total = at;
    return true;
}

// the sum of v over the workgroup, in a fixed order, in thread 0
__device__ __forceinline__ double block_sum(double v, double *red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

template <typename T>
__global__ __launch_bounds__(THREADS) void level_kernel(const T *__restrict__ x, const T *__restrict__ y, int h, int w, int C,
                                                        int tiles_x, int tiles, Window win, double c1, double c2,
                                                        double *__restrict__ slabs) {
    __shared__ double px[PATCH_H][PATCH_W], py[PATCH_H][PATCH_W];
    __shared__ double mom[5][TILE_H][PATCH_W];
    __shared__ double red[THREADS];
    const int tid = threadIdx.x, tile = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
    const int y0 = tile_y * TILE_H, x0 = tile_x * TILE_W;
    // the pixels whose squared difference this tile sums: its own TILE_H x TILE_W block and, for the last tile of a row or a
    // column, the rest of the image (which its patch covers: y0 + TILE_H >= h - HALO there)
    const bool last_y = y0 + TILE_H >= h - HALO, last_x = x0 + TILE_W >= w - HALO;
    const size_t image = (size_t)b * h * w;

    double sq = 0.;
    for (int i = tid; i < PATCH_H * PATCH_W; i += THREADS) {
        const int r = i / PATCH_W, q = i - r * PATCH_W;
        const int gy = y0 + r, gx = x0 + q;
        double xv = 0., yv = 0.;
        if (gy < h && gx < w) {
            const size_t at = (image + (size_t)gy * w + gx) * C + c;
            xv = (double)x[at];
            yv = (double)y[at];
            if ((r < TILE_H || last_y) && (q < TILE_W || last_x)) {
                const double d = xv - yv;
                sq += d * d;
            }
        }
        px[r][q] = xv;
        py[r][q] = yv;
    }
    __syncthreads();

    for (int i = tid; i < TILE_H * PATCH_W; i += THREADS) {                     // along H
        const int r = i / PATCH_W, q = i - r * PATCH_W;
        double m1 = 0., m2 = 0., e11 = 0., e22 = 0., e12 = 0.;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const double xv = px[r + k][q], yv = py[r + k][q], g = win.g[k];
            m1 += g * xv;
            m2 += g * yv;
            e11 += g * (xv * xv);
            e22 += g * (yv * yv);
            e12 += g * (xv * yv);
        }
        mom[0][r][q] = m1;
        mom[1][r][q] = m2;
        mom[2][r][q] = e11;
        mom[3][r][q] = e22;
        mom[4][r][q] = e12;
    }
    __syncthreads();

    double sum_ssim = 0., sum_cs = 0.;
    const int tx = tid % TILE_W;
#pragma unroll
    for (int j = 0; j < TILE_H / (THREADS / TILE_W); ++j) {                     // along W
        const int ty = tid / TILE_W + j * (THREADS / TILE_W);
        double m1 = 0., m2 = 0., e11 = 0., e22 = 0., e12 = 0.;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const double g = win.g[k];
            m1 += g * mom[0][ty][tx + k];
            m2 += g * mom[1][ty][tx + k];
            e11 += g * mom[2][ty][tx + k];
            e22 += g * mom[3][ty][tx + k];
            e12 += g * mom[4][ty][tx + k];
        }
        const double s11 = e11 - m1 * m1, s22 = e22 - m2 * m2, s12 = e12 - m1 * m2;
        const double cs = (2. * s12 + c2) / (s11 + s22 + c2);
        const double ssim = (2. * m1 * m2 + c1) / (m1 * m1 + m2 * m2 + c1) * cs;
        if (y0 + ty < h - HALO && x0 + tx < w - HALO) {
            sum_ssim += ssim;
            sum_cs += cs;
        }
    }
    const double a = block_sum(sum_ssim, red), d = block_sum(sum_cs, red), e = block_sum(sq, red);
    if (tid == 0) {
        double *out = slabs + (((size_t)b * C + c) * tiles + tile) * SLAB;
        out[0] = a;
        out[1] = d;
        out[2] = e;
    }
}

template <typename T>
__global__ __launch_bounds__(THREADS) void pool_kernel(const T *__restrict__ in, double *__restrict__ out, int h, int w, int C,
                                                       int ho, int wo) {
    const size_t n = (size_t)ho * wo * C, i = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int b = blockIdx.y;
    const int c = (int)(i % C), ox = (int)(i / C % wo), oy = (int)(i / C / wo);
    const int iy = 2 * oy - (h & 1), ix = 2 * ox - (w & 1);                     // an odd side is padded by one in front
    const T *img = in + (size_t)b * h * w * C;
    double v[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int yy = iy + dy, xx = ix + dx;
            v[dy][dx] = (yy >= 0 && xx >= 0) ? (double)img[((size_t)yy * w + xx) * C + c] : 0.;     // yy < h, xx < w always
        }
    out[(size_t)b * n + i] = (v[0][0] + v[0][1] + v[1][0] + v[1][1]) * 0.25;
}

struct ReducePlan {
    int levels, C;
    int tiles[MAX_LEVELS];
    double count[MAX_LEVELS];
    size_t slabs[MAX_LEVELS];
};

__global__ __launch_bounds__(THREADS) void reduce_kernel(const double *__restrict__ ws, ReducePlan p, double *__restrict__ stats,
                                                         double *__restrict__ sq_err) {
    __shared__ double red[THREADS];
    const int tid = threadIdx.x, l = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int tiles = p.tiles[l];
    const double *s = ws + p.slabs[l] + ((size_t)b * p.C + c) * tiles * SLAB;
    double a = 0., d = 0., e = 0.;
    for (int t = tid; t < tiles; t += THREADS) {
        a += s[(size_t)t * SLAB];
        d += s[(size_t)t * SLAB + 1];
        e += s[(size_t)t * SLAB + 2];
    }
    a = block_sum(a, red);
    d = block_sum(d, red);
    e = block_sum(e, red);
    if (tid == 0) {
        double *o = stats + (((size_t)b * p.levels + l) * p.C + c) * 2;
        o[0] = a / p.count[l];
        o[1] = d / p.count[l];
        if (l == 0) sq_err[(size_t)b * p.C + c] = e;
    }
}

int check_shape(int B, int H, int W, int C, int levels) {
    if (levels != 1 && levels != MAX_LEVELS) return NEFII_E_ARG;
    if (C < 1 || C > 4 || B < 1 || B > MAX_BATCH) return NEFII_E_SHAPE;
    if (H < WIN || W < WIN || H > MAX_SIDE || W > MAX_SIDE) return NEFII_E_SHAPE;
    if (levels == MAX_LEVELS && (H <= HALO * 16 || W <= HALO * 16)) return NEFII_E_SHAPE;
    return 0;
}

}  // namespace

extern "C" int64_t nefii_image_metrics_workspace_bytes(int B, int H, int W, int C, int levels) {
    const int rc = check_shape(B, H, W, C, levels);
    if (rc) return rc;
    Plan p;
    if (!make_plan(B, H, W, C, levels, &p)) return NEFII_E_SHAPE;
    return (int64_t)(p.total * sizeof(double));
}

extern "C" int nefii_image_metrics(const float *x, const float *y, int B, int H, int W, int C, int levels, const double *window,
                                   double c1, double c2, void *workspace, double *stats, double *sq_err, void *stream) {
    if (!x || !y || !window || !workspace || !stats || !sq_err) return NEFII_E_ARG;
    const int rc = check_shape(B, H, W, C, levels);
    if (rc) return rc;
    Plan p;
    if (!make_plan(B, H, W, C, levels, &p)) return NEFII_E_SHAPE;
    Window win;
    for (int k = 0; k < WIN; ++k) win.g[k] = window[k];
    double *ws = (double *)workspace;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(THREADS);
    for (int l = 0; l < levels; ++l) {
        const int h = p.h[l], w = p.w[l];
        const dim3 grid(p.tiles[l], C, B);
        const size_t n = (size_t)B * h * w * C;
        const double *lx = ws + p.image[l], *ly = lx + n;
        if (l == 0)
            hipLaunchKernelGGL(level_kernel<float>, grid, block, 0, st, x, y, h, w, C, p.tiles_x[l], p.tiles[l], win, c1, c2,
                               ws + p.slabs[l]);
        else
            hipLaunchKernelGGL(level_kernel<double>, grid, block, 0, st, lx, ly, h, w, C, p.tiles_x[l], p.tiles[l], win, c1, c2,
                               ws + p.slabs[l]);
        HIP_CHECK_LAUNCH();
        if (l + 1 < levels) {
            const int ho = p.h[l + 1], wo = p.w[l + 1];
            const size_t no = (size_t)ho * wo * C;
            const dim3 pgrid((unsigned)((no + THREADS - 1) / THREADS), B);
            double *ox = ws + p.image[l + 1], *oy = ox + (size_t)B * no;
            if (l == 0) {
                hipLaunchKernelGGL(pool_kernel<float>, pgrid, block, 0, st, x, ox, h, w, C, ho, wo);
                hipLaunchKernelGGL(pool_kernel<float>, pgrid, block, 0, st, y, oy, h, w, C, ho, wo);
            } else {
                hipLaunchKernelGGL(pool_kernel<double>, pgrid, block, 0, st, lx, ox, h, w, C, ho, wo);
                hipLaunchKernelGGL(pool_kernel<double>, pgrid, block, 0, st, ly, oy, h, w, C, ho, wo);
            }
            HIP_CHECK_LAUNCH();
        }
    }
    ReducePlan r;
    r.levels = levels;
    r.C = C;
    for (int l = 0; l < MAX_LEVELS; ++l) {
        r.tiles[l] = l < levels ? p.tiles[l] : 0;
        r.count[l] = l < levels ? (double)(p.h[l] - HALO) * (double)(p.w[l] - HALO) : 1.;
        r.slabs[l] = l < levels ? p.slabs[l] : 0;
    }
    hipLaunchKernelGGL(reduce_kernel, dim3(levels, C, B), block, 0, st, ws, r, stats, sq_err);
    HIP_CHECK_LAUNCH();
    return 0;
}
