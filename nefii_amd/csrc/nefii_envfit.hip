// ================================================================================================
// nefii_envfit.hip - fitting spherical-Gaussian lights to an environment map, fused and deterministic.
//
//   objective      envmaps/fit_envmap_with_sg.py (SG2Envmap + mean squared error + Adam)
//
//   rgb(d) = sum_m |mu_m| exp(|lambda_m| (d . a_m - 1)),   a_m = v_m / (|v_m| + eps)
//   loss   = mean over n*3 of (rgb - target)^2
//
// One iteration is two launches:
//   envfit_tile_kernel    one workgroup per tile of ENVFIT_TILE directions.  The lobes are staged in LDS already
//                         normalised; phase A (thread <-> direction) evaluates rgb, the residual r = 2(rgb - t)/(3n)
//                         and the tile's share of the loss; phase B (thread <-> (lobe, direction slice)) recomputes
//                         exp and accumulates, per lobe,
//                             A_c = sum_p r_pc e_pm        B = sum_p q_pm e_pm s_pm        C = sum_p q_pm e_pm d_p
//                         with s = d . a - 1, q = r . |mu|.  Every lane of a wave reads the same direction (LDS
//                         broadcast).  The workgroup stores one slab of M*7 + 1 partials - no atomics.
//   envfit_reduce_kernel  sums the slabs per parameter in a fixed order, applies the per-lobe chain rule (abs with
//                         torch's sign(0) = 0, the axis normalisation's Jacobian) and writes the gradient and the
//                         loss, or applies torch's Adam update in place.
// The slab count depends only on n, so results are bitwise identical from run to run.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/nefii_amd.h"

#include "hip_check.h"

namespace {

constexpr int ENVFIT_TILE = 256;        // directions per workgroup of the tile kernel (= its block size)
constexpr int ENVFIT_MAX_LOBES = NEFII_MAX_LOBES;
constexpr int RED_COLS = 32;            // reduce kernel: 4 lobes (28 parameters) per workgroup ...
constexpr int RED_GROUPS = 16;          // ... x 16 slab groups
constexpr int RED_LOBES = 4;
// exp(x) = exp2(x log2(e)): the sharpness is staged pre-scaled, so each (direction, lobe) pair costs one v_exp_f32 and
// its denormal guard instead of expf's extended-precision range reduction.  Relative error of e: ~|x| 2^-24, i.e.
// 1e-6 where a lobe still contributes (x > -20).
constexpr float LOG2E = 1.4426950408889634f;

__device__ inline float sgnf(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(ENVFIT_TILE) void envfit_tile_kernel(const float *__restrict__ lgt, int M,
                                                                   const float *__restrict__ dirs,
                                                                   const float *__restrict__ target, int64_t n,
                                                                   float eps, float *__restrict__ slabs,
                                                                   float *__restrict__ rgb_out) {
    __shared__ float4 lobe_a[ENVFIT_MAX_LOBES];     // normalised axis xyz, |lambda| log2(e)
    __shared__ float4 lobe_mu[ENVFIT_MAX_LOBES];    // |mu| rgb, 0
    __shared__ float4 pix_d[ENVFIT_TILE];           // direction xyz, 0
    __shared__ float4 pix_r[ENVFIT_TILE];           // residual rgb, 0
    __shared__ float red[ENVFIT_MAX_LOBES * 7 > ENVFIT_TILE * 7 ? ENVFIT_MAX_LOBES * 7 : ENVFIT_TILE * 7];
    __shared__ float wave_loss[ENVFIT_TILE / 64];

    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * ENVFIT_TILE;
    const int cnt = (int)(n - p0 < ENVFIT_TILE ? n - p0 : ENVFIT_TILE);

    for (int m = tid; m < M; m += ENVFIT_TILE) {
        const float *L = lgt + m * 7;
        const float r = sqrtf(L[0] * L[0] + L[1] * L[1] + L[2] * L[2]) + eps;
        lobe_a[m] = make_float4(L[0] / r, L[1] / r, L[2] / r, fabsf(L[3]) * LOG2E);
        lobe_mu[m] = make_float4(fabsf(L[4]), fabsf(L[5]), fabsf(L[6]), 0.f);
    }
    __syncthreads();

    // ---- phase A: thread <-> direction
    const float scale = 2.f / (float)(3 * n);
    float sq = 0.f;
    if (tid < cnt) {
        const int64_t p = p0 + tid;
        const float dx = dirs[p * 3], dy = dirs[p * 3 + 1], dz = dirs[p * 3 + 2];
        float c0 = 0.f, c1 = 0.f, c2 = 0.f;
        for (int m = 0; m < M; ++m) {
            const float4 a = lobe_a[m], mu = lobe_mu[m];
            const float e = exp2f(a.w * ((dx * a.x + dy * a.y + dz * a.z) - 1.f));
            c0 += mu.x * e;
            c1 += mu.y * e;
            c2 += mu.z * e;
        }
        const float e0 = c0 - target[p * 3], e1 = c1 - target[p * 3 + 1], e2 = c2 - target[p * 3 + 2];
        sq = e0 * e0 + e1 * e1 + e2 * e2;
        pix_d[tid] = make_float4(dx, dy, dz, 0.f);
        pix_r[tid] = make_float4(e0 * scale, e1 * scale, e2 * scale, 0.f);
        if (rgb_out) {
            rgb_out[p * 3] = c0;
            rgb_out[p * 3 + 1] = c1;
            rgb_out[p * 3 + 2] = c2;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    if ((tid & 63) == 0) wave_loss[tid >> 6] = sq;
    __syncthreads();

    // ---- phase B: thread <-> (lobe m, direction slice); lanes of a wave share the slice
    const int S = M < ENVFIT_TILE ? ENVFIT_TILE / M : 1;
    for (int pair = tid; pair < M * S; pair += ENVFIT_TILE) {
        const int m = pair % M, slice = pair / M;
        const float4 a = lobe_a[m], mu = lobe_mu[m];
        float A0 = 0.f, A1 = 0.f, A2 = 0.f, B = 0.f, C0 = 0.f, C1 = 0.f, C2 = 0.f;
        for (int q = slice; q < cnt; q += S) {
            const float4 d = pix_d[q], r = pix_r[q];
            const float s = (d.x * a.x + d.y * a.y + d.z * a.z) - 1.f;
            const float e = exp2f(a.w * s);
            A0 += r.x * e;
            A1 += r.y * e;
            A2 += r.z * e;
            const float we = (r.x * mu.x + r.y * mu.y + r.z * mu.z) * e;
            B += we * s;
            C0 += we * d.x;
            C1 += we * d.y;
            C2 += we * d.z;
        }
        float *o = red + (slice * M + m) * 7;
        o[0] = C0; o[1] = C1; o[2] = C2; o[3] = B; o[4] = A0; o[5] = A1; o[6] = A2;
    }
    __syncthreads();

    float *slab = slabs + (int64_t)blockIdx.x * (M * 7 + 1);
    for (int i = tid; i < M * 7; i += ENVFIT_TILE) {
        float acc = red[i];
        for (int s = 1; s < S; ++s) acc += red[s * M * 7 + i];
        slab[i] = acc;
    }
    if (tid == 0) {
        float l = 0.f;
#pragma unroll
        for (int w = 0; w < ENVFIT_TILE / 64; ++w) l += wave_loss[w];
        slab[M * 7] = l;
    }
}

// One workgroup per RED_LOBES lobes (the last one: the loss).  adam == 0: write g_out [M,7] and loss_out [1];
// adam == 1: update lgt / exp_avg / exp_avg_sq in place (torch.optim.Adam's operation order) and write loss_out [1].
__global__ __launch_bounds__(RED_COLS *RED_GROUPS) void envfit_reduce_kernel(
    float *__restrict__ lgt, int M, const float *__restrict__ slabs, int nslab, int64_t n, float eps,
    float *__restrict__ g_out, float *__restrict__ loss_out, int adam, float *__restrict__ exp_avg,
    float *__restrict__ exp_avg_sq, float one_m_beta1, float beta2, float one_m_beta2, float adam_eps, float step_size,
    float bc2_sqrt) {
    __shared__ float part[RED_GROUPS][RED_COLS];
    __shared__ float tot[RED_COLS];
    const int stride = M * 7 + 1;
    const int col = threadIdx.x % RED_COLS, grp = threadIdx.x / RED_COLS;
    const bool loss_block = (int)blockIdx.x * RED_LOBES >= M;
    const int base = loss_block ? M * 7 : blockIdx.x * RED_LOBES * 7;
    const int ncols = loss_block ? 1 : ((M - (int)blockIdx.x * RED_LOBES) < RED_LOBES ? (M - (int)blockIdx.x * RED_LOBES)
                                                                                          : RED_LOBES) * 7;
    float acc0 = 0.f, acc1 = 0.f;
    if (col < ncols) {
        const float *src = slabs + base + col;
        int s = grp;
        for (; s + RED_GROUPS < nslab; s += 2 * RED_GROUPS) {
            acc0 += src[(int64_t)s * stride];
            acc1 += src[(int64_t)(s + RED_GROUPS) * stride];
        }
        if (s < nslab) acc0 += src[(int64_t)s * stride];
    }
    part[grp][col] = acc0 + acc1;
    __syncthreads();
    if (threadIdx.x < RED_COLS) {
        float t = 0.f;
#pragma unroll
        for (int g = 0; g < RED_GROUPS; ++g) t += part[g][threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    if (loss_block) {
        if (threadIdx.x == 0) loss_out[0] = tot[0] / (float)(3 * n);
        return;
    }
    const int c = threadIdx.x;
    float g = 0.f;
    if (c < ncols) {
        const int l = c / 7, k = c % 7;
        const int m = blockIdx.x * RED_LOBES + l;
        const float *L = lgt + m * 7;
        const float *T = tot + l * 7;               // C xyz, B, A rgb
        if (k >= 4) {
            g = T[k] * sgnf(L[k]);
        } else if (k == 3) {
            g = T[3] * sgnf(L[3]);
        } else {
            // a = v / (r + eps): dL/dv = ga / (r + eps) - v (v . ga) / (r (r + eps)^2), the second term 0 at r = 0
            const float lam = fabsf(L[3]);
            const float ga0 = lam * T[0], ga1 = lam * T[1], ga2 = lam * T[2];
            const float r = sqrtf(L[0] * L[0] + L[1] * L[1] + L[2] * L[2]);
            const float re = r + eps;
            const float gk = k == 0 ? ga0 : (k == 1 ? ga1 : ga2);
            g = gk / re;
            if (r > 0.f) g -= (L[0] * ga0 + L[1] * ga1 + L[2] * ga2) / (re * re) * (L[k] / r);
        }
    }
    if (!adam) {
        if (c < ncols) g_out[base + c] = g;
        return;
    }
    __syncthreads();                                // every lobe parameter read before any is written
    if (c < ncols) {
        const int i = base + c;
        const float m1 = exp_avg[i] + one_m_beta1 * (g - exp_avg[i]);       // torch._foreach_lerp_ (weight < 0.5)
        const float v = exp_avg_sq[i] * beta2 + one_m_beta2 * (g * g);      // _foreach_mul_, _foreach_addcmul_
        const float denom = sqrtf(v) / bc2_sqrt + adam_eps;
        exp_avg[i] = m1;
        exp_avg_sq[i] = v;
        lgt[i] = lgt[i] + (-step_size) * (m1 / denom);                      // _foreach_addcdiv_
    }
}

int64_t n_slabs(int64_t n) { return (n + ENVFIT_TILE - 1) / ENVFIT_TILE; }

int launch_iteration(float *lgt, int M, const float *dirs, const float *target, int64_t n, float eps, float *slabs,
                     float *rgb, float *g_out, float *loss_out, int adam, float *exp_avg, float *exp_avg_sq,
                     float one_m_beta1, float beta2, float one_m_beta2, float adam_eps, float step_size, float bc2_sqrt,
                     hipStream_t stream) {
    const int64_t ns = n_slabs(n);
    hipLaunchKernelGGL(envfit_tile_kernel, dim3((unsigned)ns), dim3(ENVFIT_TILE), 0, stream, lgt, M, dirs, target, n,
                       eps, slabs, rgb);
    HIP_CHECK_LAUNCH();
    const int nblk = (M + RED_LOBES - 1) / RED_LOBES + 1;
    hipLaunchKernelGGL(envfit_reduce_kernel, dim3(nblk), dim3(RED_COLS * RED_GROUPS), 0, stream, lgt, M, slabs,
                       (int)ns, n, eps, g_out, loss_out, adam, exp_avg, exp_avg_sq, one_m_beta1, beta2, one_m_beta2,
                       adam_eps, step_size, bc2_sqrt);
    HIP_CHECK_LAUNCH();
    return 0;
}

bool bad_shape(int64_t n, int n_lobes) {
    // the slab count travels as an int and 3n as a float's divisor
    return n <= 0 || n_lobes < 1 || n_lobes > ENVFIT_MAX_LOBES || n > ((int64_t)1 << 31) / 3;
}

}  // namespace

extern "C" int64_t nefii_envfit_workspace_bytes(int64_t n, int n_lobes) {
    if (bad_shape(n, n_lobes)) return 0;
    return n_slabs(n) * (int64_t)(n_lobes * 7 + 1) * (int64_t)sizeof(float);
}

extern "C" int nefii_envfit_loss_grad(const float *lgtSGs, int n_lobes, const float *dirs, const float *target,
                                      int64_t n, float eps, void *workspace, float *loss, float *g_lgtSGs, float *rgb,
                                      void *stream) {
    if (!lgtSGs || !dirs || !target || !workspace || !loss || !g_lgtSGs) return NEFII_E_ARG;
    if (bad_shape(n, n_lobes)) return NEFII_E_SHAPE;
    return launch_iteration(const_cast<float *>(lgtSGs), n_lobes, dirs, target, n, eps, (float *)workspace, rgb,
                            g_lgtSGs, loss, 0, nullptr, nullptr, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, (hipStream_t)stream);
}

extern "C" int nefii_envfit_adam(float *lgtSGs, float *exp_avg, float *exp_avg_sq, int n_lobes, const float *dirs,
                                 const float *target, int64_t n, float eps, double lr, double beta1, double beta2,
                                 double adam_eps, int64_t step0, int iters, void *workspace, float *losses,
                                 void *stream) {
    if (!lgtSGs || !exp_avg || !exp_avg_sq || !dirs || !target || !workspace || !losses) return NEFII_E_ARG;
    if (iters < 0 || step0 < 0) return NEFII_E_ARG;
    if (bad_shape(n, n_lobes)) return NEFII_E_SHAPE;
    for (int i = 0; i < iters; ++i) {
        // the scalars as torch forms them: Python floats (double) handed to the fp32 kernels, bias corrections per step
        const double t = (double)(step0 + i + 1);
        const double bc1 = 1.0 - pow(beta1, t), bc2 = 1.0 - pow(beta2, t);
        const int rc = launch_iteration(lgtSGs, n_lobes, dirs, target, n, eps, (float *)workspace, nullptr, nullptr,
                                        losses + i, 1, exp_avg, exp_avg_sq, (float)(1.0 - beta1), (float)beta2,
                                        (float)(1.0 - beta2), (float)adam_eps, (float)(lr / bc1), (float)pow(bc2, 0.5),
                                        (hipStream_t)stream);
        if (rc) return rc;
    }
    return 0;
}
