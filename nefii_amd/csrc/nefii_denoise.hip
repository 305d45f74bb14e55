// nefii_denoise.hip - one level of the feature-guided a-trous wavelet filter for Monte-Carlo frames (DESIGN.md 6j;
// Dammertz, Sewtz, Hanika, Lensch: "Edge-avoiding a-trous wavelet transform for fast global illumination filtering", 2010).
//
// Frame H x W, row-major.  Guides G0[p] = (n.x, n.y, n.z, valid), G1[p] = (x.x, x.y, x.z, 0); signals C[s][p] = (r, g, b, -),
// s < S, S = 1 or 2.  For a valid centre p (G0.w > 0.5) and step s the taps are q = p + s (i, j), i, j in -2 .. 2, inside the
// image, with the B3 spline h = [1 4 6 4 1] / 16:
//
//   w_s(p,q) = h_i h_j valid(q) finite(q) w_n w_x w_c,s
//   w_n   = max(0, n_p . n_q)^sigma_n
//   w_x   = exp(-|n_p . (x_q - x_p)| / (sigma_x |x_q - x_p| + 1e-12))
//   w_c,s = exp(-|Y_s(p) - Y_s(q)| / ((|Y_s(p)| + |Y_s(q)| + 1e-12) sigma_c_level)),   Y = Rec. 709 luminance of the input
//   out_s(p) = sum_q w_s c_s(q) / sum_q w_s,  out_s(p) = in_s(p) where the sum of weights is 0
//
// finite(q) = 0 when any channel of any signal at q is NaN or inf.  Two cases the formula leaves open are closed here, the
// same way as in tests/denoise_ref.py: equal luminances give w_c = 1 whatever the denominator (sigma_c = 0 would divide 0 by
// 0), and a centre that is not finite has no luminance, so its w_c is 1 for every tap (it becomes the guided average of its
// finite neighbours).  An invalid centre copies its input.  The geometric part h_i h_j w_n w_x is computed once per tap and
// shared by the signals.
//
// One thread per pixel, a workgroup is a 32 x 8 pixel tile (a wave covers two 512-byte row segments of every array); every
// access is a 16-byte load or store, 2 + S loads per tap.  No LDS: from step 4 on the taps of a tile do not overlap, and the
// frame's working set sits in the Infinity Cache.  The taps are summed in raster order by one thread: no atomics, no
// workspace, bitwise reproducible.  Out-of-image taps read a clamped (legal) address and are dropped by a select, so the
// loads of a row of taps are issued together.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/nefii_amd.h"

#include "hip_check.h"

namespace {

constexpr int TILE_W = 32, TILE_H = 8;      // pixels of a workgroup
constexpr int MAX_SIDE = 16384;

__device__ __forceinline__ float luminance(float4 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }
__device__ __forceinline__ bool finite3(float4 c) { return isfinite(c.x) && isfinite(c.y) && isfinite(c.z); }

template <int S>
__global__ __launch_bounds__(TILE_W *TILE_H) void atrous_kernel(const float4 *__restrict__ g0, const float4 *__restrict__ g1,
                                                                const float4 *__restrict__ in, float4 *__restrict__ out,
                                                                int H, int W, int step, float sigma_n, float sigma_x,
                                                                float sigma_c) {
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
        p_finite = p_finite && finite3(cp[s]);
        yp[s] = luminance(cp[s]);
    }
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float acc[S][3], wsum[S];
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s][0] = acc[s][1] = acc[s][2] = wsum[s] = 0.f;

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
            for (int s = 0; s < S; ++s) ok = ok && finite3(cq[t][s]);
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
                if (p_finite && diff != 0.f) wc = expf(-diff / ((fabsf(yp[s]) + fabsf(yq) + 1e-12f) * sigma_c));
                const float w = geo * wc;
                acc[s][0] += w * cq[t][s].x;
                acc[s][1] += w * cq[t][s].y;
                acc[s][2] += w * cq[t][s].z;
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
        }
        out[s * n + p] = o;
    }
}

bool bad_sigma(float v) { return !(v >= 0.f); }      // negative or NaN; +inf passes (an infinite sigma_n has no power: refused)

}  // namespace

extern "C" int nefii_denoise_atrous(const void *guides0, const void *guides1, const void *in, void *out, int n_signals,
                                    int height, int width, int step, float sigma_n, float sigma_x, float sigma_c_level,
                                    void *stream) {
    if (!guides0 || !guides1 || !in || !out || in == out) return NEFII_E_ARG;
    if (n_signals < 1 || n_signals > 2) return NEFII_E_ARG;
    if (height < 1 || height > MAX_SIDE || width < 1 || width > MAX_SIDE) return NEFII_E_SHAPE;
    if (step < 1) return NEFII_E_ARG;
    if (bad_sigma(sigma_n) || bad_sigma(sigma_x) || bad_sigma(sigma_c_level) || isinf(sigma_n)) return NEFII_E_ARG;
    const dim3 grid((width + TILE_W - 1) / TILE_W, (height + TILE_H - 1) / TILE_H), block(TILE_W, TILE_H);
    const float4 *a = (const float4 *)guides0, *b = (const float4 *)guides1, *c = (const float4 *)in;
    if (n_signals == 1)
        hipLaunchKernelGGL(atrous_kernel<1>, grid, block, 0, (hipStream_t)stream, a, b, c, (float4 *)out, height, width, step,
                           sigma_n, sigma_x, sigma_c_level);
    else
        hipLaunchKernelGGL(atrous_kernel<2>, grid, block, 0, (hipStream_t)stream, a, b, c, (float4 *)out, height, width, step,
                           sigma_n, sigma_x, sigma_c_level);
    HIP_CHECK_LAUNCH();
    return 0;
}
