// nefii_patchloss.hip - the patch terms of IDRLoss, value and gradient together: the SSIM term of idr_rgb and
// of sg_rgb against the ground truth (code/model/loss.py:54-120 ssim_loss_fn, :237-253 get_ssim_loss) and the
// roughness-smoothness term (:266-276).  As torch ops the SSIM term is 10 grouped convolutions and an erosion per image, their
// backward passes and a boolean index that synchronises with the host; here it is two launches that a hipGraph can hold.
//
// Rays come in patches of P x P, P = 2 r_patch: patch p owns rows p P^2 .. (p + 1) P^2 - 1, pixel (y, x) of it is row
// p P^2 + y P + x.  m = network_object_mask & object_mask.  Per patch, per channel, at the valid positions [5, P - 5)^2:
//
//   mu1, mu2, exx, eyy, exy = the separable 'valid' 11-tap filterings of X, Y, X X, Y Y, X Y
//   s11 = exx - mu1^2, s22 = eyy - mu2^2, s12 = exy - mu1 mu2
//   l = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1),  cs = (2 s12 + C2) / (s11 + s22 + C2),  S = mean over the channels of l cs
//
// and S = 1 on the ring of 5 pixels around them.  e = m eroded by the 11 x 11 window clipped to the patch, M = sum of e over
// ALL patches; the term is sum(e (1 - S)) / M, 0 when M = 0 (the reference writes 1 - sum(e S) / M; the ring contributes to M
// alone).  The kernel filters X' = X - sx and Y' = Y - sy, sx and sy the patch's centre pixel, so that exx - mu1^2 does not
// cancel the square of the patch's brightness, and puts the shift back exactly: the 11 x 11 window sums to G2 = (sum of the
// taps)^2, which is 1 - 6e-8 and not 1 for the reference's fp32 taps, so with m1, m2 the filtered X', Y' and delta = 1 - G2
//   mu1 = m1 + sx G2,   s11 = exx' - m1^2 + delta (2 sx m1 + sx^2 G2),   s12 = exy' - m1 m2 + delta (sx m2 + sy m1 + sx sy G2)
// are the reference's quantities for any sx, sy (in fp64 the two agree to 1e-15; without the delta terms to 1e-6 only).
//
// Gradient with respect to X: with a, b, c = -e / 3 times the partial derivatives of a channel's l cs with respect to m1,
// exx' and exy' at the valid positions (sx, sy held fixed: the value does not depend on them),
// d X = G^T a + 2 X' G^T b + Y' G^T c (G^T: the transposed, 'full', separable filter) - still to be divided by M, which only
// the whole grid knows.
//
// Roughness: a_p = m over the whole patch; the term is the mean over the patches with a_p of var(roughness) (4 - mean over
// the channels of var(normal_c)), unbiased variances; the normals carry no gradient.
//
//   patch_kernel    one workgroup per patch.  Stages the masks, and per image and channel the shifted X and Y, in LDS; filters
//                   along x, then along y; forms e (1 - l cs) and a, b, c per valid position; runs the adjoint along y, then
//                   along x, and writes the unscaled gradient.  Writes one slab of five doubles with plain stores.
//   finish_kernel   every workgroup sums all slabs in the same fixed order (so all of them hold the same totals), workgroup 0
//                   writes the four losses, and each scales its share of d_idr, d_sg and d_roughness by weight / count.
// No atomics: two runs give the same bits.  No allocation and no host synchronisation: the caller brings the workspace.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nefii_amd.h"

#include "hip_check.h"

namespace {

constexpr int WIN = NEFII_PATCH_WINDOW, RAD = WIN / 2;
constexpr int MIN_SSIM_R = 6, MAX_R = 16;               // P >= 12: at least a 2 x 2 block of valid positions; P <= 32: static LDS
constexpr int MAX_P = 2 * MAX_R, MAX_V = MAX_P - 2 * RAD;
constexpr int THREADS = 256;
constexpr int SLAB = 5;     // doubles per patch: sum e, sum e (1 - l cs) over the channels for idr and for sg, a_p, a_p var var
constexpr int MAX_FINISH_BLOCKS = 128;
constexpr float C1 = 1e-4f, C2 = 9e-4f;                 // (0.01 data_range)^2, (0.03 data_range)^2 with data_range 1

// the sum of v over the workgroup, in a fixed order, in every thread
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

// unbiased variance of K values src[i * stride], by the two-pass formula; *mean_out receives the mean
__device__ __forceinline__ double block_var(const float *__restrict__ src, int stride, int K, double *red, double *mean_out) {
    double s = 0.;
    for (int i = threadIdx.x; i < K; i += THREADS) s += (double)src[(int64_t)i * stride];
    const double mean = block_sum(s, red) / K;
    double q = 0.;
    for (int i = threadIdx.x; i < K; i += THREADS) {
        const double d = (double)src[(int64_t)i * stride] - mean;
        q += d * d;
    }
    *mean_out = mean;
    return block_sum(q, red) / (K - 1);
}

__global__ __launch_bounds__(THREADS) void patch_kernel(nefii_patch_loss_params p, const float *__restrict__ idr,
                                                        const float *__restrict__ sg, const float *__restrict__ gt,
                                                        const uint8_t *__restrict__ net, const uint8_t *__restrict__ obj,
                                                        const float *__restrict__ rough, const float *__restrict__ normals,
                                                        float G2, float delta, double *__restrict__ slabs,
                                                        float *__restrict__ d_idr, float *__restrict__ d_sg,
                                                        float *__restrict__ d_rough) {
    __shared__ float xs[MAX_P * MAX_P], ys[MAX_P * MAX_P];
    __shared__ uint8_t ms[MAX_P * MAX_P], es[MAX_P * MAX_P];
    __shared__ float mom[5][MAX_P][MAX_V];              // the five moments filtered along x; then the adjoint filtered along y
    __shared__ float coef[3][MAX_V][MAX_V];
    __shared__ double red[THREADS];
    const int tid = threadIdx.x;
    const int P = 2 * p.r_patch, K = P * P, V = P - 2 * RAD;
    const int64_t base = (int64_t)blockIdx.x * K;
    const bool ssim = p.idr_ssim_weight != 0.f || p.sg_ssim_weight != 0.f;

    int holes = 0;
    for (int i = tid; i < K; i += THREADS) {
        const uint8_t m = net[base + i] != 0 && obj[base + i] != 0;
        ms[i] = m;
        holes += !m;
    }
    const bool whole = block_sum((double)holes, red) == 0.;     // (its barriers also publish ms)

    double slab[SLAB] = {0., 0., 0., 0., 0.};
    if (ssim) {
        int kept = 0;
        for (int i = tid; i < K; i += THREADS) {
            const int y = i / P, x = i - y * P;
            const int y0 = max(y - RAD, 0), y1 = min(y + RAD, P - 1), x0 = max(x - RAD, 0), x1 = min(x + RAD, P - 1);
            bool e = true;
            if (!whole)
                for (int yy = y0; yy <= y1; ++yy)
                    for (int xx = x0; xx <= x1; ++xx) e = e && ms[yy * P + xx];
            es[i] = e;
            kept += e;
        }
        slab[0] = block_sum((double)kept, red);                 // (publishes es)
        const int centre = (P / 2) * P + P / 2;
        for (int img = 0; img < 2; ++img) {
            const float *__restrict__ X = img ? sg : idr;
            float *__restrict__ dX = img ? d_sg : d_idr;
            const bool adjoint = dX && (img ? p.sg_ssim_weight : p.idr_ssim_weight) != 0.f;    // finish_kernel: the same rule
            float acc = 0.f;
            for (int c = 0; c < 3; ++c) {
                const float sx = X[(base + centre) * 3 + c], sy = gt[(base + centre) * 3 + c];
                __syncthreads();                                // the last channel's readers of xs, ys and mom are done
                for (int i = tid; i < K; i += THREADS) {
                    xs[i] = X[(base + i) * 3 + c] - sx;
                    ys[i] = gt[(base + i) * 3 + c] - sy;
                }
                __syncthreads();
                for (int i = tid; i < P * V; i += THREADS) {                                    // along x
                    const int y = i / V, xv = i - y * V;
                    float m1 = 0.f, m2 = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
                    for (int k = 0; k < WIN; ++k) {
                        const float u = xs[y * P + xv + k], v = ys[y * P + xv + k], g = p.window[k];
                        m1 = fmaf(g, u, m1);
                        m2 = fmaf(g, v, m2);
                        exx = fmaf(g, u * u, exx);
                        eyy = fmaf(g, v * v, eyy);
                        exy = fmaf(g, u * v, exy);
                    }
                    mom[0][y][xv] = m1;
                    mom[1][y][xv] = m2;
                    mom[2][y][xv] = exx;
                    mom[3][y][xv] = eyy;
                    mom[4][y][xv] = exy;
                }
                __syncthreads();
                for (int i = tid; i < V * V; i += THREADS) {                                    // along y, then point by point
                    const int yv = i / V, xv = i - yv * V;
                    float m1 = 0.f, m2 = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
                    for (int k = 0; k < WIN; ++k) {
                        const float g = p.window[k];
                        m1 = fmaf(g, mom[0][yv + k][xv], m1);
                        m2 = fmaf(g, mom[1][yv + k][xv], m2);
                        exx = fmaf(g, mom[2][yv + k][xv], exx);
                        eyy = fmaf(g, mom[3][yv + k][xv], eyy);
                        exy = fmaf(g, mom[4][yv + k][xv], exy);
                    }
                    const float mu1 = m1 + sx * G2, mu2 = m2 + sy * G2;
                    const float s11 = exx - m1 * m1 + delta * (2.f * sx * m1 + sx * sx * G2);
                    const float s22 = eyy - m2 * m2 + delta * (2.f * sy * m2 + sy * sy * G2);
                    const float s12 = exy - m1 * m2 + delta * (sx * m2 + sy * m1 + sx * sy * G2);
                    const float ln = 2.f * mu1 * mu2 + C1, ld = mu1 * mu1 + mu2 * mu2 + C1;
                    const float cn = 2.f * s12 + C2, cd = s11 + s22 + C2;
                    const float l = ln / ld, cs = cn / cd;
                    const float e = es[(yv + RAD) * P + xv + RAD] ? 1.f : 0.f;
                    acc += e * (1.f - l * cs);
                    // d (l cs) / d (exx', exy', m1): m1 moves l through mu1, and s11 and s12 directly
                    const float f_xx = -l * cs / cd, f_xy = 2.f * l / cd;
                    const float f_mu = (2.f * mu2 - 2.f * mu1 * l) / ld * cs - 2.f * (m1 - sx * delta) * f_xx -
                                       (m2 - sy * delta) * f_xy;
                    const float w = e * (-1.f / 3.f);
                    coef[0][yv][xv] = w * f_mu;
                    coef[1][yv][xv] = w * f_xx;
                    coef[2][yv][xv] = w * f_xy;
                }
                if (!adjoint) continue;                         // the same for the whole grid
                __syncthreads();
                for (int i = tid; i < 3 * P * V; i += THREADS) {                                // the adjoint along y
                    const int q = i / (P * V), rest = i - q * (P * V), y = rest / V, xv = rest - y * V;
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < WIN; ++k) {
                        const int yy = y - k;
                        if (yy >= 0 && yy < V) s = fmaf(p.window[k], coef[q][yy][xv], s);
                    }
                    mom[q][y][xv] = s;
                }
                __syncthreads();
                for (int i = tid; i < K; i += THREADS) {                                        // the adjoint along x
                    const int y = i / P, x = i - y * P;
                    float a = 0.f, b = 0.f, cc = 0.f;
#pragma unroll
                    for (int k = 0; k < WIN; ++k) {
                        const int xx = x - k;
                        if (xx >= 0 && xx < V) {
                            const float g = p.window[k];
                            a = fmaf(g, mom[0][y][xx], a);
                            b = fmaf(g, mom[1][y][xx], b);
                            cc = fmaf(g, mom[2][y][xx], cc);
                        }
                    }
                    dX[(base + i) * 3 + c] = a + 2.f * xs[i] * b + ys[i] * cc;
                }
            }
            slab[1 + img] = block_sum((double)acc, red);
        }
    }
    if (p.roughnesssmooth_weight != 0.f) {
        if (whole) {                                            // the same for the whole workgroup
            double mean, unused, nv = 0.;
            for (int c = 0; c < 3; ++c) nv += block_var(normals + base * 3 + c, 3, K, red, &unused);
            const double factor = 4. - nv / 3.;
            slab[3] = 1.;
            slab[4] = block_var(rough + base, 1, K, red, &mean) * factor;
            if (d_rough)
                for (int i = tid; i < K; i += THREADS)
                    d_rough[base + i] = (float)(factor * 2. * ((double)rough[base + i] - mean) / (K - 1));
        } else if (d_rough) {
            for (int i = tid; i < K; i += THREADS) d_rough[base + i] = 0.f;
        }
    }
    if (tid == 0)
        for (int q = 0; q < SLAB; ++q) slabs[(int64_t)blockIdx.x * SLAB + q] = slab[q];
}

__device__ __forceinline__ void scale_in_place(float *__restrict__ d, int64_t count, float s) {
    if (!d) return;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < count; i += (int64_t)gridDim.x * THREADS)
        d[i] = s != 0.f ? d[i] * s : 0.f;                       // s == 0: patch_kernel may not have written d at all
}

__global__ __launch_bounds__(THREADS) void finish_kernel(nefii_patch_loss_params p, const double *__restrict__ slabs,
                                                         int64_t n_patches, int64_t n, float *__restrict__ losses,
                                                         float *__restrict__ d_idr, float *__restrict__ d_sg,
                                                         float *__restrict__ d_rough) {
    __shared__ double red[THREADS];
    double tot[SLAB];
    for (int q = 0; q < SLAB; ++q) {
        double a = 0.;
        for (int64_t t = threadIdx.x; t < n_patches; t += THREADS) a += slabs[t * SLAB + q];
        tot[q] = block_sum(a, red);
    }
    const bool any = tot[0] > 0., any_whole = tot[3] > 0.;
    const float idr_l = any ? (float)(tot[1] / (3. * tot[0])) : 0.f, sg_l = any ? (float)(tot[2] / (3. * tot[0])) : 0.f;
    const float rs_l = any_whole ? (float)(tot[4] / tot[3]) : 0.f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        losses[0] = p.idr_ssim_weight * idr_l + p.sg_ssim_weight * sg_l + p.roughnesssmooth_weight * rs_l;
        losses[1] = idr_l;
        losses[2] = sg_l;
        losses[3] = rs_l;
    }
    scale_in_place(d_idr, n * 3, any ? p.idr_ssim_weight / (float)tot[0] : 0.f);
    scale_in_place(d_sg, n * 3, any ? p.sg_ssim_weight / (float)tot[0] : 0.f);
    scale_in_place(d_rough, n, any_whole ? p.roughnesssmooth_weight / (float)tot[3] : 0.f);
}

// 0, or the refusal: the patch side, the patch count
int check_shape(const nefii_patch_loss_params *p, int64_t n, int64_t *n_patches) {
    if (p->r_patch < 1 || p->r_patch > MAX_R) return NEFII_E_SHAPE;
    if ((p->idr_ssim_weight != 0.f || p->sg_ssim_weight != 0.f) && p->r_patch < MIN_SSIM_R) return NEFII_E_SHAPE;
    const int64_t K = 4ll * p->r_patch * p->r_patch;
    if (n < K || n % K != 0 || n / K > 0x7fffffffll) return NEFII_E_SHAPE;
    *n_patches = n / K;
    return 0;
}

}  // namespace

extern "C" int64_t nefii_idr_patch_loss_workspace_bytes(const nefii_patch_loss_params *h_params, int64_t n) {
    if (!h_params) return NEFII_E_ARG;
    int64_t n_patches;
    const int rc = check_shape(h_params, n, &n_patches);
    return rc ? rc : n_patches * SLAB * (int64_t)sizeof(double);
}

extern "C" int nefii_idr_patch_loss(const nefii_patch_loss_params *h_params, const float *idr_rgb, const float *sg_rgb,
                                    const float *rgb_gt, const uint8_t *network_object_mask, const uint8_t *object_mask,
                                    const float *roughness, const float *normals, int64_t n, void *workspace, float *losses,
                                    float *d_idr_rgb, float *d_sg_rgb, float *d_roughness, void *stream) {
    if (!h_params || !idr_rgb || !sg_rgb || !rgb_gt || !network_object_mask || !object_mask || !roughness || !normals ||
        !workspace || !losses)
        return NEFII_E_ARG;
    int64_t n_patches;
    const int rc = check_shape(h_params, n, &n_patches);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *slabs = (double *)workspace;
    double taps = 0.;
    for (int k = 0; k < WIN; ++k) taps += (double)h_params->window[k];
    hipLaunchKernelGGL(patch_kernel, dim3((unsigned)n_patches), dim3(THREADS), 0, st, *h_params, idr_rgb, sg_rgb, rgb_gt,
                       network_object_mask, object_mask, roughness, normals, (float)(taps * taps), (float)(1. - taps * taps),
                       slabs, d_idr_rgb, d_sg_rgb, d_roughness);
    HIP_CHECK_LAUNCH();
    const int64_t share = (n * 3 + 4 * THREADS - 1) / (4 * THREADS);       // about four elements of a colour gradient per thread
    const unsigned blocks = (unsigned)(share < 1 ? 1 : (share > MAX_FINISH_BLOCKS ? MAX_FINISH_BLOCKS : share));
    hipLaunchKernelGGL(finish_kernel, dim3(blocks), dim3(THREADS), 0, st, *h_params, slabs, n_patches, n, losses, d_idr_rgb,
                       d_sg_rgb, d_roughness);
    HIP_CHECK_LAUNCH();
    return 0;
}
