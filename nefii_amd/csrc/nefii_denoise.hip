// nefii_denoise.hip - the a-trous denoiser of Monte-Carlo frames: one level of the feature-guided wavelet filter (DESIGN.md 6j;
// Dammertz, Sewtz, Hanika, Lensch: "Edge-avoiding a-trous wavelet transform for fast global illumination filtering", 2010),
// its variance-guided variant (the luminance stop of Schied et al. 2017, "Spatiotemporal variance-guided
// filtering") and the per-pixel variance of a frame from its rays that the variant reads.
//
// 1. The level (nefii_denoise_atrous).  Frame H x W, row-major.  Guides G0[p] = (n.x, n.y, n.z, valid), G1[p] = (x.x, x.y, x.z,
//    0); signals C[s][p] = (r, g, b, -), s < S, S = 1 or 2.  For a valid centre p (G0.w > 0.5) and step s the taps are
//    q = p + s (i, j), i, j in -2 .. 2, inside the image, with the B3 spline h = [1 4 6 4 1] / 16:
//
//      w_s(p,q) = h_i h_j valid(q) finite(q) w_n w_x w_c,s
//      w_n   = max(0, n_p . n_q)^sigma_n
//      w_x   = exp(-|n_p . (x_q - x_p)| / (sigma_x |x_q - x_p| + 1e-12))
//      w_c,s = exp(-|Y_s(p) - Y_s(q)| / ((|Y_s(p)| + |Y_s(q)| + 1e-12) sigma_c_level)),   Y = Rec. 709 luminance of the input
//      out_s(p).rgb = sum_q w_s c_s(q) / sum_q w_s,  out_s(p) = in_s(p) where the sum of weights is 0
//
//    finite(q) = 0 when any of r, g, b of any signal at q is NaN or inf; the fourth lane is not looked at, and out_s(p)'s is
//    in_s(p)'s.  Two cases the formula leaves open are closed here, the same way as in tests/denoise_ref.py: equal luminances
//    give w_c = 1 whatever the denominator (sigma_c = 0 would divide 0 by 0), and a centre that is not finite has no
//    luminance, so its w_c is 1 for every tap (it becomes the guided average of its finite neighbours).  An invalid centre
//    copies its input.  The geometric part h_i h_j w_n w_x is computed once per tap and shared by the signals.
//
//    One thread per pixel, a workgroup is a 32 x 8 pixel tile (a wave covers two 512-byte row segments of every array); every
//    access is a 16-byte load or store, 2 + S loads per tap.  No LDS: from step 4 on the taps of a tile do not overlap, and
//    the frame's working set sits in the Infinity Cache.  The taps are summed in raster order by one thread: no atomics, no
//    workspace, bitwise reproducible.  Out-of-image taps read a clamped (legal) address and are dropped by a select, so the
//    loads of a row of taps are issued together.
//
// 2. The variance-guided level (nefii_denoise_atrous_variance) is that level on signals C_s[p] = (r, g, b, v), v the variance
//    of the mean of the luminance, every use of v being max(v, 0).  It differs in four places (V in the kernel):
//
//      a. finite(q) = 0 when any of the FOUR lanes of any signal at q is NaN or inf.
//      b. A prefilter: vbar_s(p) = sum g_ij v_s(q) / sum g_ij over the 3 x 3 pixels at UNIT offsets around p, whatever the
//         step, that are in the image, valid and finite, g = [1 2 1] x [1 2 1] / 16.  Beside the taps a pixel so reads nine
//         more elements per signal and the nine guide elements that hold their validity.
//      c. The luminance stop is scaled by the local standard deviation, with a sigma_l that is the same at every level (the
//         carried variance shrinks instead):  w_l,s = exp(-|Y_s(p) - Y_s(q)| / (sigma_l sqrt(vbar_s(p)) + 1e-12)) in place of
//         w_c,s.  Closed as above: equal luminances give 1, and so does a centre that is not finite or has no pixel in vbar.
//         sigma_l = inf switches the stop off (w_l = 1; inf * sqrt(0) is not formed).
//      d. A fourth accumulator carries the variance along: out_s(p).v = sum w^2 v_s(q) / (sum w)^2.
//
// 3. The moments (nefii_pixel_moments).  Row p R + r of diffuse, albedo, specular [P R, 3] and hit [P R] is ray r of pixel p.
//    For a pixel whose R rays all hit, with abar the mean albedo per channel and a = max(abar, NEFII_ALBEDO_FLOOR):
//
//      signals[0][p] = (mean_r diffuse_r / a,  sum_r (e_r - ebar)^2 / (R (R - 1))),   e_r = Y(diffuse_r / a)
//      signals[1][p] = (mean_r specular_r,     the same with                          e_r = Y(specular_r))
//
//    The fourth lane is the variance of the MEAN of the luminance.  Every sum is fp64, in two passes (means, then squared
//    deviations); results are rounded to fp32 once.  Y is linear, so ebar is formed as Y of the mean colour: with R equal
//    samples the fp64 sums are exact (24-bit values, R <= 4096), ebar is e_r bit for bit and the variance exactly 0.  A NaN
//    or inf sample (albedo included) leaves the lanes it enters non-finite; a pixel with a ray that missed is four zeros in
//    both signals.
//    GROUP = 16 lanes of a wave64 share a pixel: lane g takes the rays g, g + 16, ..., so the lanes of a group read
//    neighbouring 12-byte rows of the pixel's contiguous 3 R floats; a butterfly over the group adds the lanes' sums.  The
//    order of every sum depends on R alone.  No atomics, no LDS, 16-byte vector stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/nefii_amd.h"

#include "hip_check.h"

namespace {

// ---- 1, 2. the level ---------------------------------------------------------------------------------------------------
constexpr int TILE_W = 32, TILE_H = 8;      // pixels of a workgroup
constexpr int MAX_SIDE = 16384;

__device__ __forceinline__ float luminance(float4 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }

template <bool V>                           // 2a: lane w is looked at by the variance-guided level only
__device__ __forceinline__ bool finite_lanes(float4 c) {
    if constexpr (V) return isfinite(c.x) && isfinite(c.y) && isfinite(c.z) && isfinite(c.w);
    return isfinite(c.x) && isfinite(c.y) && isfinite(c.z);
}

// sigma_cl: sigma_c_level of the plain level, sigma_l of the variance-guided one
template <int S, bool V>
__global__ __launch_bounds__(TILE_W *TILE_H) void atrous_kernel(const float4 *__restrict__ g0, const float4 *__restrict__ g1,
                                                                const float4 *__restrict__ in, float4 *__restrict__ out,
                                                                int H, int W, int step, float sigma_n, float sigma_x,
                                                                float sigma_cl) {
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
        p_finite = p_finite && finite_lanes<V>(cp[s]);
        yp[s] = luminance(cp[s]);
    }
    bool stop_on = p_finite;                // the luminance stop acts at this centre
    float scale[S];                         // 2c: sigma_l sqrt(vbar) + 1e-12
    if constexpr (V) {
        // 2b: the 3 x 3 prefilter of the variance at unit offsets, whatever the step
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
                for (int s = 0; s < S; ++s) ok = ok && finite_lanes<V>(cq[t][s]);
                if (!ok) continue;
                const float g = g3[j + 1] * g3[t];
#pragma unroll
                for (int s = 0; s < S; ++s) vsum[s] += g * fmaxf(cq[t][s].w, 0.f);
                gsum += g;
            }
        }
        stop_on = p_finite && gsum > 0.f && !isinf(sigma_cl);
#pragma unroll
        for (int s = 0; s < S; ++s) scale[s] = stop_on ? sigma_cl * sqrtf(vsum[s] / gsum) + 1e-12f : 1.f;
    }

    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float acc[S][V ? 4 : 3], wsum[S];       // acc[s][3] is 2d's
#pragma unroll
    for (int s = 0; s < S; ++s) {
        acc[s][0] = acc[s][1] = acc[s][2] = wsum[s] = 0.f;
        if constexpr (V) acc[s][3] = 0.f;
    }

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
            for (int s = 0; s < S; ++s) ok = ok && finite_lanes<V>(cq[t][s]);
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
                const float yq = luminance(cq[t][s]);
                const float diff = fabsf(yp[s] - yq);
                float wc = 1.f;
                if (stop_on && diff != 0.f) {
                    if constexpr (V) wc = expf(-diff / scale[s]);
                    else wc = expf(-diff / ((fabsf(yp[s]) + fabsf(yq) + 1e-12f) * sigma_cl));
                }
                const float w = geo * wc;
                acc[s][0] += w * cq[t][s].x;
                acc[s][1] += w * cq[t][s].y;
                acc[s][2] += w * cq[t][s].z;
                if constexpr (V) acc[s][3] += w * w * fmaxf(cq[t][s].w, 0.f);
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
            if constexpr (V) o.w = acc[s][3] / (wsum[s] * wsum[s]);
        }
        out[s * n + p] = o;
    }
}

bool bad_sigma(float v) { return !(v >= 0.f); }      // negative or NaN; +inf passes (an infinite sigma_n has no power: refused)

// the refusals and the launch of the two level entry points; sigma_cl as in the kernel
int launch_level(bool variance, const void *guides0, const void *guides1, const void *in, void *out, int n_signals, int height,
                 int width, int step, float sigma_n, float sigma_x, float sigma_cl, void *stream) {
    if (!guides0 || !guides1 || !in || !out || in == out) return NEFII_E_ARG;
    if (n_signals < 1 || n_signals > 2) return NEFII_E_ARG;
    if (height < 1 || height > MAX_SIDE || width < 1 || width > MAX_SIDE) return NEFII_E_SHAPE;
    if (step < 1) return NEFII_E_ARG;
    if (bad_sigma(sigma_n) || bad_sigma(sigma_x) || bad_sigma(sigma_cl) || isinf(sigma_n)) return NEFII_E_ARG;
    const dim3 grid((width + TILE_W - 1) / TILE_W, (height + TILE_H - 1) / TILE_H), block(TILE_W, TILE_H);
    const auto kernel = variance ? (n_signals == 1 ? atrous_kernel<1, true> : atrous_kernel<2, true>)
                                 : (n_signals == 1 ? atrous_kernel<1, false> : atrous_kernel<2, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, (const float4 *)guides0, (const float4 *)guides1,
                       (const float4 *)in, (float4 *)out, height, width, step, sigma_n, sigma_x, sigma_cl);
    HIP_CHECK_LAUNCH();
    return 0;
}

// ---- 3. the moments ----------------------------------------------------------------------------------------------------
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

}  // namespace

extern "C" int nefii_denoise_atrous(const void *guides0, const void *guides1, const void *in, void *out, int n_signals,
                                    int height, int width, int step, float sigma_n, float sigma_x, float sigma_c_level,
                                    void *stream) {
    return launch_level(false, guides0, guides1, in, out, n_signals, height, width, step, sigma_n, sigma_x, sigma_c_level, stream);
}

extern "C" int nefii_denoise_atrous_variance(const void *guides0, const void *guides1, const void *in, void *out, int n_signals,
                                             int height, int width, int step, float sigma_n, float sigma_x, float sigma_l,
                                             void *stream) {
    return launch_level(true, guides0, guides1, in, out, n_signals, height, width, step, sigma_n, sigma_x, sigma_l, stream);
}

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
