// nefii_adaptive.hip - adaptive sampling of Monte-Carlo frames: a pilot round estimates each pixel's noise from
// its own rays, a fixed budget of further rounds goes to the pixels that need it (two-stage Neyman allocation), the rounds
// are merged.  A round is R rays per pixel; every sum below is fp64, nothing is contracted, no float atomics, no LDS-order
// dependence, nothing depends on the launch geometry: the same bits from run to run and for any split into calls.
//
// 1. nefii_ray_luminance_moments.  Row p R + r of rgb [P R, 3] is ray r of pixel p.  out[p] = (ebar, M2), ebar = Y(mean_r
//    rgb_r) with the Rec. 709 Y, M2 = sum_r (Y(rgb_r) - ebar)^2: two passes in fp64, one rounding to fp32.  Y is linear, so with R
//    equal samples the fp64 sums are exact (24-bit values, R <= 4096), ebar is Y(rgb_r) bit for bit and M2 exactly 0; so it is
//    for R = 1.  A NaN or inf sample leaves both lanes non-finite.  GROUP = 16 lanes of a wave64 share a pixel (lane g takes
//    the rays g, g + 16, ...), a butterfly adds the lanes' sums: nefii_denoise.hip section 3's scheme, the order a function of
//    R alone.
//
// 2. nefii_adaptive_merge.  rows [m, C + 2] are a round's packed outputs over m pixels: C columns that are means over the
//    round's R rays, then that round's (ebar, M2).  Row i belongs to pixel pixel[i] (NULL: i).  Per pixel, listed once:
//
//      sum[p][c] += R rows[i][c]                 (the product is exact: 24 bits x R <= 4096)
//      delta = ebar - mean;  n' = n + R;  mean' = mean + (delta R) / n';  M2' = (M2 + M2_b) + (delta delta) ((n R) / n')
//
//    on stat[p] = (n, mean, M2), the pairwise rule of Chan, Golub and LeVeque (1979), in this order of operations.  With n = 0
//    the result is (R, ebar, M2_b) exactly.  One thread per (row, column), the last of a row takes stat: plain loads and stores.
//    An index outside [0, P) writes nothing.
//
// 3. nefii_adaptive_score.  s = sqrt(M2 / (n - 1)) / (|mean| + eps) in fp64, rounded once; n < 2 or a rounded s that is not
//    finite gives 0 (a NaN pixel must not soak up the budget).  With dilate the score is the maximum of s over the 3 x 3 pixels
//    around p that lie in the image.
//
// 4. nefii_adaptive_count / nefii_adaptive_targets.  k_p(lambda) = min(K, max(1, ceil(fl32(lambda s_p)))), written so that a NaN
//    product gives 1: x > 1 ? (x >= K ? K : ceil(x)) : 1.  T = sum_p k_p is added to *total (the caller zeroes it): 64-bit integer
//    partial sums per thread, wave and workgroup, one integer atomic per workgroup - integer addition commutes.
//
// 5. nefii_adaptive_finalise.  out = fl32(sum / n); a column named in mask_columns is 1 where sum == n (every ray of every round
//    had it set) else 0; rays = n; variance = M2 / (n (n - 1)), the variance of the mean luminance, 0 for n < 2.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/nefii_amd.h"

#include "hip_check.h"

namespace {

constexpr int GROUP = 16;                   // lanes per pixel (1)
constexpr int BLOCK = 256;
constexpr int MAX_RAYS = 4096;
constexpr int MAX_COLUMNS = 64;             // mask_columns is one 64-bit word
constexpr int MAX_ROUNDS = 65536;
constexpr int MAX_SIDE = 16384;
constexpr int COUNT_ITEMS = 8;              // scores per thread of the count kernel

__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int m = GROUP / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, GROUP);
    return v;
}

__device__ __forceinline__ double luminance64(double r, double g, double b) { return 0.2126 * r + 0.7152 * g + 0.0722 * b; }

// ---- 1 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void ray_moments_kernel(const float *__restrict__ rgb, long long P, int R,
                                                            float2 *__restrict__ out) {
    const int g = threadIdx.x % GROUP;
    const long long slot = (long long)blockIdx.x * (BLOCK / GROUP) + threadIdx.x / GROUP;
    const long long p = slot < P ? slot : P - 1;            // a group past the end repeats the last pixel and stores nothing
    const size_t base = (size_t)p * R;
    double sum[3] = {0., 0., 0.};
    for (int r = g; r < R; r += GROUP) {
        const size_t at = (base + r) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) sum[k] += (double)rgb[at + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) sum[k] = group_sum(sum[k]) / (double)R;
    const double ebar = luminance64(sum[0], sum[1], sum[2]);
    double dev = 0.;
    for (int r = g; r < R; r += GROUP) {
        const size_t at = (base + r) * 3;
        const double e = luminance64((double)rgb[at], (double)rgb[at + 1], (double)rgb[at + 2]);
        dev += (e - ebar) * (e - ebar);
    }
    dev = group_sum(dev);
    if (slot >= P || g != 0) return;
    out[p] = make_float2((float)ebar, (float)dev);
}

// ---- 2 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void merge_kernel(const float *__restrict__ rows, const int *__restrict__ pixel, long long m,
                                                      long long P, int C, int R, double *__restrict__ sum,
                                                      double *__restrict__ stat) {
    const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= m * (C + 1)) return;
    const long long i = t / (C + 1);
    const int c = (int)(t % (C + 1));
    const long long p = pixel ? (long long)pixel[i] : i;
    if (p < 0 || p >= P) return;
    const float *row = rows + (size_t)i * (C + 2);
    const double rays = (double)R;
    if (c < C) {
        double *s = sum + (size_t)p * C + c;
        *s = *s + rays * (double)row[c];
        return;
    }
    double *st = stat + (size_t)p * 3;
    const double n = st[0], mean = st[1], m2 = st[2];
    const double ebar = (double)row[C], m2_b = (double)row[C + 1];
    const double delta = ebar - mean;
    const double n_new = n + rays;
    st[0] = n_new;
    st[1] = mean + (delta * rays) / n_new;
    st[2] = (m2 + m2_b) + (delta * delta) * ((n * rays) / n_new);
}

// ---- 3 ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float pixel_score(const double *__restrict__ stat, size_t p, double eps) {
    const double n = stat[p * 3], mean = stat[p * 3 + 1], m2 = stat[p * 3 + 2];
    const float s = (float)(sqrt(m2 / (n - 1.)) / (fabs(mean) + eps));
    return n >= 2. && isfinite(s) ? s : 0.f;               // a NaN n fails the comparison
}

__global__ __launch_bounds__(BLOCK) void score_kernel(const double *__restrict__ stat, int H, int W, double eps, int dilate,
                                                      float *__restrict__ score) {
    const long long p = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (p >= (long long)H * W) return;
    float s = pixel_score(stat, (size_t)p, eps);
    if (dilate) {
        const int y = (int)(p / W), x = (int)(p % W);
        for (int j = -1; j <= 1; ++j)
            for (int i = -1; i <= 1; ++i) {
                const int qy = y + j, qx = x + i;
                if (qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
                s = fmaxf(s, pixel_score(stat, (size_t)qy * W + qx, eps));
            }
    }
    score[p] = s;
}

// ---- 4 ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int rounds_of(float s, float lambda, int K) {
    const float x = lambda * s;
    return x > 1.f ? (x >= (float)K ? K : (int)ceilf(x)) : 1;
}

__global__ __launch_bounds__(BLOCK) void count_kernel(const float *__restrict__ score, long long P, float lambda, int K,
                                                      unsigned long long *__restrict__ total) {
    __shared__ unsigned long long part[BLOCK / 64];
    const long long first = (long long)blockIdx.x * (BLOCK * COUNT_ITEMS) + threadIdx.x;
    unsigned long long t = 0;
#pragma unroll
    for (int k = 0; k < COUNT_ITEMS; ++k) {
        const long long p = first + (long long)k * BLOCK;
        if (p < P) t += (unsigned long long)rounds_of(score[p], lambda, K);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
    if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long b = 0;
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) b += part[w];
        atomicAdd(total, b);
    }
}

__global__ __launch_bounds__(BLOCK) void targets_kernel(const float *__restrict__ score, long long P, float lambda, int K,
                                                        int *__restrict__ k) {
    const long long p = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (p < P) k[p] = rounds_of(score[p], lambda, K);
}

// ---- 5 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void finalise_kernel(const double *__restrict__ sum, const double *__restrict__ stat,
                                                         long long P, int C, unsigned long long mask_columns,
                                                         float *__restrict__ out, int *__restrict__ rays,
                                                         float *__restrict__ variance) {
    const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (t >= P * (C + 1)) return;
    const long long p = t / (C + 1);
    const int c = (int)(t % (C + 1));
    const double n = stat[(size_t)p * 3];
    if (c < C) {
        const double s = sum[(size_t)p * C + c];
        out[(size_t)p * C + c] = (mask_columns >> c) & 1ull ? (s == n ? 1.f : 0.f) : (float)(s / n);
        return;
    }
    rays[p] = (int)n;
    variance[p] = n >= 2. ? (float)(stat[(size_t)p * 3 + 2] / (n * (n - 1.))) : 0.f;
}

bool blocks_for(long long threads, unsigned *blocks) {
    const long long b = (threads + BLOCK - 1) / BLOCK;
    if (b < 1 || b > 2147483647LL) return false;
    *blocks = (unsigned)b;
    return true;
}

bool misaligned(const void *p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

bool bad_lambda(float v) { return !(v >= 0.f) || isinf(v); }

}  // namespace

extern "C" int nefii_ray_luminance_moments(const float *rgb, int64_t n_pixels, int rays, float *out, void *stream) {
    if (!rgb || !out || misaligned(rgb, 4) || misaligned(out, 8)) return NEFII_E_ARG;
    if (rays < 1 || rays > MAX_RAYS || n_pixels < 1 || n_pixels >= (1LL << 31)) return NEFII_E_SHAPE;
    unsigned blocks;
    if (!blocks_for(n_pixels * GROUP, &blocks)) return NEFII_E_SHAPE;
    hipLaunchKernelGGL(ray_moments_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, rgb, (long long)n_pixels, rays,
                       (float2 *)out);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_adaptive_merge(const float *rows, const int32_t *pixel, int64_t m, int64_t n_pixels, int columns, int rays,
                                    double *sum, double *stat, void *stream) {
    if (!rows || !sum || !stat || misaligned(rows, 4) || misaligned(pixel, 4) || misaligned(sum, 8) || misaligned(stat, 8))
        return NEFII_E_ARG;
    if (columns < 1 || columns > MAX_COLUMNS || rays < 1 || rays > MAX_RAYS) return NEFII_E_SHAPE;
    if (n_pixels < 1 || n_pixels >= (1LL << 31) || m < 1 || m > n_pixels || (!pixel && m != n_pixels)) return NEFII_E_SHAPE;
    unsigned blocks;
    if (!blocks_for(m * (columns + 1), &blocks)) return NEFII_E_SHAPE;
    hipLaunchKernelGGL(merge_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, rows, (const int *)pixel, (long long)m,
                       (long long)n_pixels, columns, rays, sum, stat);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_adaptive_score(const double *stat, int height, int width, double eps, int dilate, float *score,
                                    void *stream) {
    if (!stat || !score || misaligned(stat, 8) || misaligned(score, 4)) return NEFII_E_ARG;
    if (!(eps > 0.) || isinf(eps) || dilate < 0 || dilate > 1) return NEFII_E_ARG;
    if (height < 1 || height > MAX_SIDE || width < 1 || width > MAX_SIDE) return NEFII_E_SHAPE;
    unsigned blocks;
    if (!blocks_for((long long)height * width, &blocks)) return NEFII_E_SHAPE;
    hipLaunchKernelGGL(score_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, stat, height, width, eps, dilate, score);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_adaptive_count(const float *score, int64_t n_pixels, float lambda, int max_rounds, uint64_t *total,
                                    void *stream) {
    if (!score || !total || misaligned(score, 4) || misaligned(total, 8) || bad_lambda(lambda)) return NEFII_E_ARG;
    if (n_pixels < 1 || n_pixels >= (1LL << 31) || max_rounds < 1 || max_rounds > MAX_ROUNDS) return NEFII_E_SHAPE;
    const long long per_block = BLOCK * COUNT_ITEMS;
    hipLaunchKernelGGL(count_kernel, dim3((unsigned)((n_pixels + per_block - 1) / per_block)), dim3(BLOCK), 0,
                       (hipStream_t)stream, score, (long long)n_pixels, lambda, max_rounds, (unsigned long long *)total);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_adaptive_targets(const float *score, int64_t n_pixels, float lambda, int max_rounds, int32_t *k,
                                      void *stream) {
    if (!score || !k || misaligned(score, 4) || misaligned(k, 4) || bad_lambda(lambda)) return NEFII_E_ARG;
    if (n_pixels < 1 || n_pixels >= (1LL << 31) || max_rounds < 1 || max_rounds > MAX_ROUNDS) return NEFII_E_SHAPE;
    unsigned blocks;
    if (!blocks_for(n_pixels, &blocks)) return NEFII_E_SHAPE;
    hipLaunchKernelGGL(targets_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, score, (long long)n_pixels, lambda,
                       max_rounds, (int *)k);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_adaptive_finalise(const double *sum, const double *stat, int64_t n_pixels, int columns,
                                       uint64_t mask_columns, float *out, int32_t *rays, float *variance, void *stream) {
    if (!sum || !stat || !out || !rays || !variance) return NEFII_E_ARG;
    if (misaligned(sum, 8) || misaligned(stat, 8) || misaligned(out, 4) || misaligned(rays, 4) || misaligned(variance, 4))
        return NEFII_E_ARG;
    if (columns < 1 || columns > MAX_COLUMNS || n_pixels < 1 || n_pixels >= (1LL << 31)) return NEFII_E_SHAPE;
    if (columns < 64 && (mask_columns >> columns)) return NEFII_E_ARG;
    unsigned blocks;
    if (!blocks_for(n_pixels * (columns + 1), &blocks)) return NEFII_E_SHAPE;
    hipLaunchKernelGGL(finalise_kernel, dim3(blocks), dim3(BLOCK), 0, (hipStream_t)stream, sum, stat, (long long)n_pixels,
                       columns, (unsigned long long)mask_columns, out, rays, variance);
    HIP_CHECK_LAUNCH();
    return 0;
}
