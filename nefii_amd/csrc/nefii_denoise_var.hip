// nefii_denoise_var.hip - per-pixel variance of a Monte-Carlo frame from its rays, and the a-trous level that is guided by it
// (the variance-guided luminance stop of Schied et al. 2017, "Spatiotemporal variance-guided filtering", on the
// geometric guides of nefii_denoise.hip).
//
// 1. nefii_pixel_moments.  Row p R + r of diffuse, albedo, specular [P R, 3] and hit [P R] is ray r of pixel p.  For a pixel
//    whose R rays all hit, with abar the mean albedo per channel and a = max(abar, NEFII_ALBEDO_FLOOR):
//
//      signals[0][p] = (mean_r diffuse_r / a,  sum_r (e_r - ebar)^2 / (R (R - 1))),   e_r = Y(diffuse_r / a)
//      signals[1][p] = (mean_r specular_r,     the same with                          e_r = Y(specular_r))
//
//    Y = Rec. 709 luminance.  The fourth lane is the variance of the MEAN of the luminance.  Every sum is fp64, in two passes
//    (means, then squared deviations); results are rounded to fp32 once.  Y is linear, so ebar is formed as Y of the mean
//    colour: with R equal samples the fp64 sums are exact (24-bit values, R <= 4096), ebar is e_r bit for bit and the
//    variance exactly 0.  A NaN or inf sample (albedo included) leaves the lanes it enters non-finite; a pixel with a ray
//    that missed is four zeros in both signals.
//    GROUP = 16 lanes of a wave64 share a pixel: lane g takes the rays g, g + 16, ..., so the lanes of a group read
//    neighbouring 12-byte rows of the pixel's contiguous 3 R floats; a butterfly over the group adds the lanes' sums.  The
//    order of every sum depends on R alone.  No atomics, no LDS, 16-byte vector stores.
//
// 2. nefii_denoise_atrous_variance.  nefii_denoise.hip's level - guides, tile, tap order, B3 spline, w_n, w_x, valid, "an
//    invalid centre copies its input", "out-of-image taps read a clamped legal address" - on signals C_s[p] = (r, g, b, v)
//    with the luminance stop scaled by the local standard deviation and the variance carried along.  Every use of v is
//    max(v, 0).
//
//      vbar_s(p) = sum g_ij v_s(q) / sum g_ij over the 3 x 3 pixels at UNIT offsets around p that are in the image, valid
//                  and finite, g = [1 2 1] x [1 2 1] / 16
//      w_l,s = exp(-|Y_s(p) - Y_s(q)| / (sigma_l sqrt(vbar_s(p)) + 1e-12))
//      w = h_i h_j valid(q) finite(q) w_n w_x w_l,s
//      out_s(p).rgb = sum w c_s(q) / sum w,   out_s(p).v = sum w^2 v_s(q) / (sum w)^2,   out_s(p) = in_s(p) where sum w = 0
//
//    finite(q) = 0 when any of the four lanes of any signal at q is NaN or inf.  Closed as in 6j: equal luminances give
//    w_l = 1 whatever the denominator, and a centre that is not finite, or one without a pixel in vbar, has w_l = 1 for every
//    tap.  sigma_l = inf switches the stop off (w_l = 1; inf * sqrt(0) is not formed).  sigma_l is the same at every level:
//    the carried variance shrinks instead.
//    One thread per pixel, 32 x 8 tile, 16-byte loads and stores, taps summed in raster order by one thread, no LDS, no
//    atomics.  Beside 6j's taps a pixel reads the 3 x 3 neighbourhood once more: nine loads per signal and the nine guide
//    elements that hold their validity.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/nefii_amd.h"

#include "hip_check.h"

namespace {

// ---- 1. moments ------------------------------------------------------------------------------------------------------
constexpr int GROUP = 16;                   // lanes per pixel
constexpr int MOMENTS_BLOCK = 256;          // 16 pixels
constexpr int MAX_RAYS = 4096;

__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int m = GROUP / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, GROUP);
    return v;
}

__device__ __forceinline__ double luminance64(double r, double g, double b) { return 0.2126 * r + 0.7152 * g + 0.0722 * b; }

__global__ __launch_bounds__(MOMENTS_BLOCK) void pixel_moments_kernel(const float *__restrict__ diffuse,
                                                                      const float *__restrict__ albedo,
                                                                      const float *__restrict__ specular,
                                                                      const unsigned char *__restrict__ hit, long long P, int R,
                                                                      float4 *__restrict__ signals) {
    const int g = threadIdx.x % GROUP;
    const long long slot = (long long)blockIdx.x * (MOMENTS_BLOCK / GROUP) + threadIdx.x / GROUP;
    const long long p = slot < P ? slot : P - 1;            // a group past the end repeats the last pixel and stores nothing
    const size_t base = (size_t)p * R;
    double sum[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) sum[k] = 0.;
    int all_hit = 1;
    for (int r = g; r < R; r += GROUP) {
        const size_t at = (base + r) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            sum[k] += (double)albedo[at + k];
            sum[3 + k] += (double)diffuse[at + k];
            sum[6 + k] += (double)specular[at + k];
        }
        all_hit &= hit[base + r] != 0;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) sum[k] = group_sum(sum[k]) / (double)R;
#pragma unroll
    for (int m = GROUP / 2; m >= 1; m >>= 1) all_hit &= __shfl_xor(all_hit, m, GROUP);
    double a[3], light[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = sum[k] < (double)NEFII_ALBEDO_FLOOR ? (double)NEFII_ALBEDO_FLOOR : sum[k];       // a NaN mean stays NaN
        light[k] = sum[3 + k] / a[k];
    }
    const double poison = 0. * (sum[0] + sum[1] + sum[2]);          // NaN when an albedo is NaN or inf, else 0
    const double ebar0 = luminance64(light[0], light[1], light[2]);
    const double ebar1 = luminance64(sum[6], sum[7], sum[8]);
    double dev0 = 0., dev1 = 0.;
    for (int r = g; r < R; r += GROUP) {
        const size_t at = (base + r) * 3;
        const double e0 = luminance64((double)diffuse[at] / a[0], (double)diffuse[at + 1] / a[1], (double)diffuse[at + 2] / a[2]);
        const double e1 = luminance64((double)specular[at], (double)specular[at + 1], (double)specular[at + 2]);
        dev0 += (e0 - ebar0) * (e0 - ebar0);
        dev1 += (e1 - ebar1) * (e1 - ebar1);
    }
    const double per_mean = (double)R * (double)(R - 1);
    dev0 = group_sum(dev0) / per_mean;
    dev1 = group_sum(dev1) / per_mean;
    if (slot >= P || g > 1) return;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (all_hit) {
        if (g == 0)
            o = make_float4((float)(light[0] + poison), (float)(light[1] + poison), (float)(light[2] + poison),
                            (float)(dev0 + poison));
        else
            o = make_float4((float)sum[6], (float)sum[7], (float)sum[8], (float)dev1);
    }
    signals[(size_t)g * P + p] = o;
}

// ---- 2. the variance-guided level ------------------------------------------------------------------------------------
constexpr int TILE_W = 32, TILE_H = 8;      // pixels of a workgroup
constexpr int MAX_SIDE = 16384;

__device__ __forceinline__ float luminance(float4 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }
__device__ __forceinline__ bool finite4(float4 c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z) && isfinite(c.w); }

template <int S>
__global__ __launch_bounds__(TILE_W *TILE_H) void atrous_variance_kernel(const float4 *__restrict__ g0,
                                                                         const float4 *__restrict__ g1,
                                                                         const float4 *__restrict__ in, float4 *__restrict__ out,
                                                                         int H, int W, int step, float sigma_n, float sigma_x,
                                                                         float sigma_l) {
    const int x = blockIdx.x * TILE_W + threadIdx.x, y = blockIdx.y * TILE_H + threadIdx.y;
    if (x >= W || y >= H) return;
    const size_t n = (size_t)H * W, p = (size_t)y * W + x;
    const float4 np = g0[p];
    float4 cp[S];
#pragma unroll
    for (int s = 0; s < S; ++s) cp[s] = in[s * n + p];
    if (!(np.w > 0.5f)) {
#pragma unroll
        for (int s = 0; s < S; ++s) out[s * n + p] = cp[s];
        return;
    }
    const float4 xp = g1[p];
    bool p_finite = true;
    float yp[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        p_finite = p_finite && finite4(cp[s]);
        yp[s] = luminance(cp[s]);
    }
    // the 3 x 3 prefilter of the variance at unit offsets, whatever the step
    const float g3[3] = {0.25f, 0.5f, 0.25f};
    float vsum[S], gsum = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) vsum[s] = 0.f;
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
        const int qy = y + j;
        const bool row_in = qy >= 0 && qy < H;
        const size_t row = (size_t)(row_in ? qy : y) * W;
        float4 nq[3], cq[3][S];
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            const int qx = x + i;
            const size_t q = row + (size_t)(qx >= 0 && qx < W ? qx : x);
            nq[i + 1] = g0[q];
#pragma unroll
            for (int s = 0; s < S; ++s) cq[i + 1][s] = in[s * n + q];
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int qx = x + t - 1;
            bool ok = row_in && qx >= 0 && qx < W && nq[t].w > 0.5f;
#pragma unroll
            for (int s = 0; s < S; ++s) ok = ok && finite4(cq[t][s]);
            if (!ok) continue;
            const float g = g3[j + 1] * g3[t];
#pragma unroll
            for (int s = 0; s < S; ++s) vsum[s] += g * fmaxf(cq[t][s].w, 0.f);
            gsum += g;
        }
    }
    const bool stop_on = p_finite && gsum > 0.f && !isinf(sigma_l);
    float scale[S];                         // sigma_l sqrt(vbar) + 1e-12
#pragma unroll
    for (int s = 0; s < S; ++s) scale[s] = stop_on ? sigma_l * sqrtf(vsum[s] / gsum) + 1e-12f : 1.f;

    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float acc[S][4], wsum[S];
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s][0] = acc[s][1] = acc[s][2] = acc[s][3] = wsum[s] = 0.f;

    for (int j = -2; j <= 2; ++j) {
        const long long qy = (long long)y + (long long)j * step;
        const bool row_in = qy >= 0 && qy < H;
        const size_t row = (size_t)(row_in ? qy : y) * W;
        float4 nq[5], xq[5], cq[5][S];
        bool in_image[5];
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const long long qx = (long long)x + (long long)i * step;
            in_image[i + 2] = row_in && qx >= 0 && qx < W;
            const size_t q = row + (size_t)(qx >= 0 && qx < W ? qx : x);
            nq[i + 2] = g0[q];
            xq[i + 2] = g1[q];
#pragma unroll
            for (int s = 0; s < S; ++s) cq[i + 2][s] = in[s * n + q];
        }
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            bool ok = in_image[t] && nq[t].w > 0.5f;
#pragma unroll
            for (int s = 0; s < S; ++s) ok = ok && finite4(cq[t][s]);
            if (!ok) continue;
            const float d = np.x * nq[t].x + np.y * nq[t].y + np.z * nq[t].z;
            const float wn = d > 0.f ? exp2f(sigma_n * log2f(d)) : (sigma_n == 0.f ? 1.f : 0.f);
            const float dx = xq[t].x - xp.x, dy = xq[t].y - xp.y, dz = xq[t].z - xp.z;
            const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
            const float off = fabsf(np.x * dx + np.y * dy + np.z * dz);
            const float wx = expf(-off / (sigma_x * dist + 1e-12f));
            const float geo = h[j + 2] * h[t] * wn * wx;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const float diff = fabsf(yp[s] - luminance(cq[t][s]));
                float wl = 1.f;
                if (stop_on && diff != 0.f) wl = expf(-diff / scale[s]);
                const float w = geo * wl;
                acc[s][0] += w * cq[t][s].x;
                acc[s][1] += w * cq[t][s].y;
                acc[s][2] += w * cq[t][s].z;
                acc[s][3] += w * w * fmaxf(cq[t][s].w, 0.f);
                wsum[s] += w;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < S; ++s) {
        float4 o = cp[s];
        if (wsum[s] > 0.f) {
            o.x = acc[s][0] / wsum[s];
            o.y = acc[s][1] / wsum[s];
            o.z = acc[s][2] / wsum[s];
            o.w = acc[s][3] / (wsum[s] * wsum[s]);
        }
        out[s * n + p] = o;
    }
}

bool bad_sigma(float v) { return !(v >= 0.f); }      // negative or NaN; +inf passes (an infinite sigma_n has no power: refused)

}  // namespace

extern "C" int nefii_pixel_moments(const float *diffuse, const float *albedo, const float *specular, const unsigned char *hit,
                                   int64_t n_pixels, int rays, float *signals, void *stream) {
    if (!diffuse || !albedo || !specular || !hit || !signals || ((uintptr_t)signals & 15)) return NEFII_E_ARG;
    if (rays < 2 || rays > MAX_RAYS || n_pixels < 1) return NEFII_E_SHAPE;
    const int64_t per_block = MOMENTS_BLOCK / GROUP, blocks = (n_pixels + per_block - 1) / per_block;
    if (blocks > 2147483647LL) return NEFII_E_SHAPE;
    hipLaunchKernelGGL(pixel_moments_kernel, dim3((unsigned)blocks), dim3(MOMENTS_BLOCK), 0, (hipStream_t)stream, diffuse, albedo,
                       specular, hit, (long long)n_pixels, rays, (float4 *)signals);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_denoise_atrous_variance(const void *guides0, const void *guides1, const void *in, void *out, int n_signals,
                                             int height, int width, int step, float sigma_n, float sigma_x, float sigma_l,
                                             void *stream) {
    if (!guides0 || !guides1 || !in || !out || in == out) return NEFII_E_ARG;
    if (n_signals < 1 || n_signals > 2) return NEFII_E_ARG;
    if (height < 1 || height > MAX_SIDE || width < 1 || width > MAX_SIDE) return NEFII_E_SHAPE;
    if (step < 1) return NEFII_E_ARG;
    if (bad_sigma(sigma_n) || bad_sigma(sigma_x) || bad_sigma(sigma_l) || isinf(sigma_n)) return NEFII_E_ARG;
    const dim3 grid((width + TILE_W - 1) / TILE_W, (height + TILE_H - 1) / TILE_H), block(TILE_W, TILE_H);
    const float4 *a = (const float4 *)guides0, *b = (const float4 *)guides1, *c = (const float4 *)in;
    if (n_signals == 1)
        hipLaunchKernelGGL(atrous_variance_kernel<1>, grid, block, 0, (hipStream_t)stream, a, b, c, (float4 *)out, height, width,
                           step, sigma_n, sigma_x, sigma_l);
    else
        hipLaunchKernelGGL(atrous_variance_kernel<2>, grid, block, 0, (hipStream_t)stream, a, b, c, (float4 *)out, height, width,
                           step, sigma_n, sigma_x, sigma_l);
    HIP_CHECK_LAUNCH();
    return 0;
}
