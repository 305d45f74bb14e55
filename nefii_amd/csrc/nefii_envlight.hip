// nefii_envlight.hip - a lat-long HDR environment map as the light of the Monte-Carlo renderer.
//
//   constant_2d_light_sampling / pdf_fn_constant_2d_light   code/model/path_tracing_render.py:291-380
//   pt_render_shadow_indirect_mlp_envmap                      code/model/path_tracing_render.py:1496-
//
// Light: map[H][W][3] fp32, texel (i, j) covers v in [i/H, (i+1)/H), u in [j/W, (j+1)/W); phi = pi v.  Radiance is the
// nearest texel.  Distribution (PBRT InfiniteAreaLight): f(i,j) = max(mean(rgb), 0) * sin(pi (i + 0.5) / H), row sums and
// prefix sums in fp64, stored as fp32 CDFs - marginal M[H], conditionals C[H][W], each ending in exactly 1.0f.  A texel's
// probability is taken from the stored floats, P = (M[i] - M[i-1]) (C[i][j] - C[i][j-1]), and the solid-angle pdf is
// P H W / (2 pi^2 sin phi): the density the MIS weights use is the one the sampler produces.  The sampler inverts the CDFs
// continuously (PBRT SampleContinuous) where the reference returns texel corners.
//
// Table (nefii_envlight_table_bytes): M [H] float | C [H][W] float | row sums [H] double, each part 256-byte aligned.  The
// device code that reads it - texel_of, texel_prob, solid_angle_pdf, sample_cdf, direction_of, Rot, to_light, to_world_rot - is
// envlight_table.h, shared with the irradiance bake of nefii_texbake.hip.
#include <hip/hip_runtime.h>
#include "../../include/nefii_amd.h"
#include "mc_sampling.h"
#include "envlight_table.h"

#include "hip_check.h"

namespace {

constexpr int BUILD_T = 256;        // threads of a build workgroup
constexpr int MIS_T = 128;          // nefii_envlight_mis_sample: one thread per surface point
constexpr int LOOKUP_T = 256;       // radiance / pdf: one thread per direction

int64_t s_offset(int H, int W) { return c_offset(H) + align256((int64_t)H * W * 4); }  // row sums after C

// ---- build --------------------------------------------------------------------------------------------------------
// The CDF of n values val(k) into out[0..n): each thread owns one contiguous run of ceil(n / BUILD_T) values, a
// Hillis-Steele scan over the runs' sums gives every run its start.  Fixed order throughout: two builds are bitwise
// equal.  A zero (or non-finite) total gives the uniform CDF.  Returns the total (every thread).
template <class Val>
__device__ double cdf_block(const Val &val, int64_t n, float *__restrict__ out, double *scan) {
    const int t = threadIdx.x;
    const int64_t per = (n + BUILD_T - 1) / BUILD_T;
    const int64_t b = min(n, (int64_t)t * per), e = min(n, b + per);
    double s = 0.0;
    for (int64_t k = b; k < e; ++k) s += val(k);
    scan[t] = s;
    __syncthreads();
    for (int off = 1; off < BUILD_T; off <<= 1) {
        const double add = t >= off ? scan[t - off] : 0.0;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    const double total = scan[BUILD_T - 1];
    const bool uniform = !(total > 0.0) || !isfinite(total);
    double run = t > 0 ? scan[t - 1] : 0.0;
    for (int64_t k = b; k < e; ++k) {
        run += val(k);
        float c = uniform ? (float)((double)(k + 1) / (double)n) : (float)(run / total);
        if (k == n - 1) c = 1.f;
        out[k] = c;
    }
    return total;
}

struct RowF {      // f(i, j) of one row
    const float *row;
    double s;      // sin(pi (i + 0.5) / H)
    __device__ double operator()(int64_t j) const {
        const float *p = row + j * 3;
        const double m = ((double)p[0] + (double)p[1] + (double)p[2]) / 3.0;
        return (m > 0.0 ? m : 0.0) * s;          // negative (or NaN) texels count as zero
    }
};
struct RowSum {
    const double *sums;
    __device__ double operator()(int64_t i) const { return sums[i]; }
};

__global__ __launch_bounds__(BUILD_T) void build_rows_kernel(const float *__restrict__ map, int H, int W,
                                                             float *__restrict__ C, double *__restrict__ sums) {
    __shared__ double scan[BUILD_T];
    const int i = blockIdx.x;
    const RowF f{map + (int64_t)i * W * 3, sin(M_PI * ((double)i + 0.5) / (double)H)};
    const double total = cdf_block(f, W, C + (int64_t)i * W, scan);
    if (threadIdx.x == 0) sums[i] = total > 0.0 && isfinite(total) ? total : 0.0;
}

__global__ __launch_bounds__(BUILD_T) void build_marginal_kernel(int H, const double *__restrict__ sums,
                                                                 float *__restrict__ M) {
    __shared__ double scan[BUILD_T];
    cdf_block(RowSum{sums}, H, M, scan);
}

// ---- the rotated map -------------------------------------------------------------------------------------
// R is world-from-light, row-major: L_R(d) = L(R^T d), a sampled direction is R direction_of(u, v), p_R(d) = p(R^T d) -
// solid angle is rotation invariant, so the one table serves every rotation.  A rotation whose flag is set (the host found
// its nine floats to be exactly the identity) skips the products: 1 x + 0 y + 0 z would turn -0 into +0 and move
// atan2f(side, x) across the seam.  Every kernel below is one body with two instantiations: ROT reads rotation a of
// rot [A][9] / rot_identity [A]; !ROT is that flag set at compile time, and never looks at its (null) rotation arguments.
// They come last in every parameter list: the other arguments then sit at the same kernarg offsets in both.
template <bool ROT>
__device__ __forceinline__ Rot load_rot(const float *__restrict__ rot, const int *__restrict__ identity, int64_t a) {
    Rot R{{}, true};
    if constexpr (ROT) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R.m[k] = rot[a * 9 + k];
        R.identity = identity[a] != 0;
    }
    return R;
}

// the rotation of item p of a lookup or of the bounce: rot_index[p], or rotation 0 for every item
template <bool ROT>
__device__ __forceinline__ Rot load_rot_of(const float *__restrict__ rot, const int *__restrict__ identity,
                                           const int *__restrict__ rot_index, int64_t p) {
    return load_rot<ROT>(rot, identity, ROT && rot_index ? rot_index[p] : 0);
}

// ROT: A rotations at once, blockIdx.y is the rotation and slice a of every output is what a launch with rotation a alone
// writes.  Rows 0 and 1 never see the light: they are the same bits in every slice.
template <bool ROT>
__global__ __launch_bounds__(MIS_T) void envlight_mis_kernel(const float *__restrict__ map, Table tb, int H, int W,
                                                             int coord, const float *__restrict__ rough,
                                                             const float *__restrict__ normal,
                                                             const float *__restrict__ view,
                                                             const float *__restrict__ uni, int64_t n,
                                                             float *__restrict__ wi_out,      // [A][3][n][3]
                                                             float *__restrict__ own_pdf,     // [A][3][n]
                                                             float *__restrict__ pdf_tab,     // [A][3][n][3]
                                                             float *__restrict__ light,       // [A][3][n][3]
                                                             const float *__restrict__ rot,
                                                             const int *__restrict__ rot_identity) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t a = ROT ? blockIdx.y : 0;
    const Rot R = load_rot<ROT>(rot, rot_identity, a);
    const F3 nn = f3(normal[p * 3], normal[p * 3 + 1], normal[p * 3 + 2]);
    const F3 vv = f3(view[p * 3], view[p * 3 + 1], view[p * 3 + 2]);
    const float r = rough[p];
    const float *u = uni + p * 7;
    MC_SAMPLE_BRDF(nn, vv, r, u);       // w0, p0 and w1, p1: the same code as nefii_mis_sample's rows 0 and 1
    // --- the map: row by the marginal (u[4]), column by that row's conditional (u[5]), continuous inside the texel
    float dv, du;
    const int i2 = sample_cdf(tb.M, H, u[4], dv);
    const int j2 = sample_cdf(tb.C + (int64_t)i2 * W, W, u[5], du);
    const float v2 = ((float)i2 + dv) / (float)H, u2 = ((float)j2 + du) / (float)W;
    const F3 w2 = to_world_rot(R, direction_of(u2, v2, coord));
    const float p2 = solid_angle_pdf(texel_prob(tb, W, i2, j2), H, W, sinpif(v2));
    const Texel t0 = texel_of(to_light(R, w0), H, W, coord), t1 = texel_of(to_light(R, w1), H, W, coord);
    const float pm0 = solid_angle_pdf(texel_prob(tb, W, t0.i, t0.j), H, W, t0.sin_phi);
    const float pm1 = solid_angle_pdf(texel_prob(tb, W, t1.i, t1.j), H, W, t1.sin_phi);
    const F3 w[3] = {w0, w1, w2};
    const float own[3] = {fmaxf(p0, TINY), fmaxf(p1, TINY), fmaxf(p2, TINY)};
    const float pmap[3] = {pm0, pm1, own[2]};
    const int ti[3] = {t0.i, t1.i, i2}, tj[3] = {t0.j, t1.j, j2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const size_t q = ((size_t)a * 3 + k) * n + p;
        float *wo = wi_out + q * 3;
        wo[0] = w[k].x, wo[1] = w[k].y, wo[2] = w[k].z;
        own_pdf[q] = own[k];
        float *t = pdf_tab + q * 3;
        t[0] = k == 0 ? own[0] : pdf_cos_fn(w[k], nn);
        t[1] = k == 1 ? own[1] : pdf_ggx_fn(w[k], nn, vv, r);
        t[2] = pmap[k];
        copy_texel(map, W, ti[k], tj[k], light + q * 3);
    }
}

template <bool ROT>
__global__ __launch_bounds__(LOOKUP_T) void envlight_radiance_kernel(const float *__restrict__ map, int H, int W,
                                                                     int coord, const float *__restrict__ dirs,
                                                                     int64_t n, float *__restrict__ rgb,
                                                                     const float *__restrict__ rot,
                                                                     const int *__restrict__ rot_identity,
                                                                     const int *__restrict__ rot_index) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const Rot R = load_rot_of<ROT>(rot, rot_identity, rot_index, p);
    const Texel t = texel_of(to_light(R, f3(dirs[p * 3], dirs[p * 3 + 1], dirs[p * 3 + 2])), H, W, coord);
    copy_texel(map, W, t.i, t.j, rgb + p * 3);
}

template <bool ROT>
__global__ __launch_bounds__(LOOKUP_T) void envlight_pdf_kernel(Table tb, int H, int W, int coord,
                                                                const float *__restrict__ dirs, int64_t n,
                                                                float *__restrict__ pdf,
                                                                const float *__restrict__ rot,
                                                                const int *__restrict__ rot_identity,
                                                                const int *__restrict__ rot_index) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const Rot R = load_rot_of<ROT>(rot, rot_identity, rot_index, p);
    const Texel t = texel_of(to_light(R, f3(dirs[p * 3], dirs[p * 3 + 1], dirs[p * 3 + 2])), H, W, coord);
    pdf[p] = solid_angle_pdf(texel_prob(tb, W, t.i, t.j), H, W, t.sin_phi);
}

// ---- one recomputed bounce under the map ----------------------------------------------------------------
// One thread per secondary hit: ONE direction by one-sample MIS (balance heuristic) over the renderer's three techniques,
// and the hit's reflected radiance estimate along -view for unit visibility, weight = f_r cos L / mix.  The directions are
// envlight_mis_kernel's (MC_SAMPLE_BRDF, the same CDF inversion), the BRDF is nefii_mc_shade_forward's (brdf_geom / ggx_dg
// of mc_sampling.h).  ROT: a rotation per hit - the k = 2 direction is rotated out, texel_of for k < 2 is rotated in.
constexpr int BOUNCE_T = 128;

template <bool ROT>
__global__ __launch_bounds__(BOUNCE_T) void envlight_bounce_kernel(
    const float *__restrict__ map, Table tb, int H, int W, int coord, const float *__restrict__ spec,
    const float *__restrict__ rough, const float *__restrict__ albedo, const float *__restrict__ normal,
    const float *__restrict__ view, const float *__restrict__ uni, int64_t m,
    float *__restrict__ wo_out,      // [m][3]
    float *__restrict__ weight,      // [m][3]
    float *__restrict__ mix_pdf,     // [m] or NULL
    const float *__restrict__ rot, const int *__restrict__ rot_identity, const int *__restrict__ rot_index) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const Rot R = load_rot_of<ROT>(rot, rot_identity, rot_index, p);
    const F3 nn = f3(normal[p * 3], normal[p * 3 + 1], normal[p * 3 + 2]);
    const F3 vv = f3(view[p * 3], view[p * 3 + 1], view[p * 3 + 2]);
    const float r = rough[p];
    const float u0 = uni[p * 3], u1 = uni[p * 3 + 1], u2 = uni[p * 3 + 2];
    const int k = min((int)(3.f * u0), 2);
    F3 wo;
    int ti, tj;
    float p_map;
    if (k == 2) {      // the map: row by the marginal (u1), column by that row's conditional (u2), as envlight_mis_kernel
        float dv, du;
        ti = sample_cdf(tb.M, H, u1, dv);
        tj = sample_cdf(tb.C + (int64_t)ti * W, W, u2, du);
        const float v2 = ((float)ti + dv) / (float)H, uu = ((float)tj + du) / (float)W;
        wo = to_world_rot(R, direction_of(uu, v2, coord));
        p_map = solid_angle_pdf(texel_prob(tb, W, ti, tj), H, W, sinpif(v2));
    } else {
        const float u[4] = {u1, u2, u1, u2};      // cosine reads u[0..1], GGX u[2..3]
        MC_SAMPLE_BRDF(nn, vv, r, u);
        (void)p0, (void)p1;                       // the density here is the mixture's, below
        wo = k == 0 ? w0 : w1;
        const Texel t = texel_of(to_light(R, wo), H, W, coord);
        ti = t.i, tj = t.j;
        p_map = solid_angle_pdf(texel_prob(tb, W, ti, tj), H, W, t.sin_phi);
    }
    // pdf_cos_fn >= TINY / pi, so mix >= TINY / (3 pi): the weight is finite on an all-zero map and at wo = -view
    const float mix = ((pdf_cos_fn(wo, nn) + pdf_ggx_fn(wo, nn, vv, r)) + p_map) / 3.f;
    float L[3];
    copy_texel(map, W, ti, tj, L);
    const BrdfGeom g = brdf_geom(nn, vv, wo);      // nefii_mc_shade_forward's BRDF along wo
    const float dg = ggx_dg<float>(r, g.nh, g.d1, g.d2);
    const float K = g.d2 / mix;      // cos / density
    float *w = weight + p * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float F = spec[c] + (1.f - spec[c]) * g.P;
        const float fs = F * dg / g.den;
        w[c] = fmaxf(K * L[c] * fs, 0.f) + fmaxf(K * L[c] * (albedo[p * 3 + c] / PI_F), 0.f);
    }
    wo_out[p * 3] = wo.x, wo_out[p * 3 + 1] = wo.y, wo_out[p * 3 + 2] = wo.z;
    if (mix_pdf) mix_pdf[p] = mix;
}

unsigned blocks(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }

constexpr int MAX_ROTATIONS = 65535;      // the rotation is the grid's y of the batched sampler
constexpr int LAUNCH = 1;                 // checked(): nothing stands against the launch

struct RotArgs {      // what a _rot entry point takes on top of its unrotated twin, which passes none
    const float *rot = nullptr;
    const int *identity = nullptr;
    int A = 1;
    const int *index = nullptr;
};

// the checks of every sampler and lookup, in the entry points' order; `pointers`: the entry point's own are all there
template <bool ROT>
int checked(bool pointers, int coord, const RotArgs &ra, int64_t n, int H, int W) {
    if (!pointers || (ROT && (!ra.rot || !ra.identity))) return NEFII_E_ARG;
    if (coord != 0 && coord != 1) return NEFII_E_ARG;
    if (ROT && ra.A < 1) return NEFII_E_ARG;
    if (n <= 0) return 0;
    if (bad_shape(H, W)) return NEFII_E_SHAPE;
    return LAUNCH;
}

template <bool ROT>
int mis_sample(const float *map, const void *table, int H, int W, int coord, const RotArgs &ra, const float *roughness,
               const float *normal, const float *view, const float *uniforms, int64_t n, float *wi, float *own_pdf,
               float *pdf_table, float *light, void *stream) {
    const int c = checked<ROT>(map && table && roughness && normal && view && uniforms && wi && own_pdf && pdf_table && light,
                               coord, ra, n, H, W);
    if (c != LAUNCH) return c;
    if (ra.A > MAX_ROTATIONS) return NEFII_E_SHAPE;
    hipLaunchKernelGGL(envlight_mis_kernel<ROT>, dim3(blocks(n, MIS_T), (unsigned)ra.A), dim3(MIS_T), 0,
                       (hipStream_t)stream, map, table_of(table, H), H, W, coord, roughness, normal, view, uniforms, n, wi,
                       own_pdf, pdf_table, light, ra.rot, ra.identity);
    HIP_CHECK_LAUNCH();
    return 0;
}

template <bool ROT>
int bounce_sample(const float *map, const void *table, int H, int W, int coord, const RotArgs &ra, const float *specular,
                  const float *roughness, const float *albedo, const float *normal, const float *view,
                  const float *uniforms, int64_t m, float *wo, float *weight, float *mix_pdf, void *stream) {
    const int c = checked<ROT>(map && table && specular && roughness && albedo && normal && view && uniforms && wo && weight,
                               coord, ra, m, H, W);
    if (c != LAUNCH) return c;
    hipLaunchKernelGGL(envlight_bounce_kernel<ROT>, dim3(blocks(m, BOUNCE_T)), dim3(BOUNCE_T), 0, (hipStream_t)stream, map,
                       table_of(table, H), H, W, coord, specular, roughness, albedo, normal, view, uniforms, m, wo, weight,
                       mix_pdf, ra.rot, ra.identity, ra.index);
    HIP_CHECK_LAUNCH();
    return 0;
}

template <bool ROT>
int radiance(const float *map, int H, int W, int coord, const RotArgs &ra, const float *dirs, int64_t n, float *rgb,
             void *stream) {
    const int c = checked<ROT>(map && dirs && rgb, coord, ra, n, H, W);
    if (c != LAUNCH) return c;
    hipLaunchKernelGGL(envlight_radiance_kernel<ROT>, dim3(blocks(n, LOOKUP_T)), dim3(LOOKUP_T), 0, (hipStream_t)stream,
                       map, H, W, coord, dirs, n, rgb, ra.rot, ra.identity, ra.index);
    HIP_CHECK_LAUNCH();
    return 0;
}

template <bool ROT>
int pdf_of(const void *table, int H, int W, int coord, const RotArgs &ra, const float *dirs, int64_t n, float *pdf,
           void *stream) {
    const int c = checked<ROT>(table && dirs && pdf, coord, ra, n, H, W);
    if (c != LAUNCH) return c;
    hipLaunchKernelGGL(envlight_pdf_kernel<ROT>, dim3(blocks(n, LOOKUP_T)), dim3(LOOKUP_T), 0, (hipStream_t)stream,
                       table_of(table, H), H, W, coord, dirs, n, pdf, ra.rot, ra.identity, ra.index);
    HIP_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int64_t nefii_envlight_table_bytes(int height, int width) {
    if (bad_shape(height, width)) return 0;
    return s_offset(height, width) + align256((int64_t)height * 8);
}

extern "C" int nefii_envlight_build(const float *map, int height, int width, void *table, void *stream) {
    if (!map || !table) return NEFII_E_ARG;
    if (bad_shape(height, width)) return NEFII_E_SHAPE;
    char *b = (char *)table;
    float *M = (float *)b, *C = (float *)(b + c_offset(height));
    double *sums = (double *)(b + s_offset(height, width));
    hipLaunchKernelGGL(build_rows_kernel, dim3(height), dim3(BUILD_T), 0, (hipStream_t)stream, map, height, width, C,
                       sums);
    HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(build_marginal_kernel, dim3(1), dim3(BUILD_T), 0, (hipStream_t)stream, height,
                       (const double *)sums, M);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_envlight_mis_sample(const float *map, const void *table, int height, int width, int coord,
                                         const float *roughness, const float *normal, const float *view,
                                         const float *uniforms, int64_t n, float *wi, float *own_pdf,
                                         float *pdf_table, float *light, void *stream) {
    return mis_sample<false>(map, table, height, width, coord, {}, roughness, normal, view, uniforms, n, wi, own_pdf,
                             pdf_table, light, stream);
}

extern "C" int nefii_envlight_mis_sample_rot(const float *map, const void *table, int height, int width, int coord,
                                             const float *rot, const int *rot_identity, int A, const float *roughness,
                                             const float *normal, const float *view, const float *uniforms, int64_t n,
                                             float *wi, float *own_pdf, float *pdf_table, float *light, void *stream) {
    return mis_sample<true>(map, table, height, width, coord, {rot, rot_identity, A}, roughness, normal, view, uniforms, n,
                            wi, own_pdf, pdf_table, light, stream);
}

extern "C" int nefii_envlight_bounce_sample(const float *map, const void *table, int height, int width, int coord,
                                            const float *specular, const float *roughness, const float *albedo,
                                            const float *normal, const float *view, const float *uniforms, int64_t m,
                                            float *wo, float *weight, float *mix_pdf, void *stream) {
    return bounce_sample<false>(map, table, height, width, coord, {}, specular, roughness, albedo, normal, view, uniforms,
                                m, wo, weight, mix_pdf, stream);
}

extern "C" int nefii_envlight_bounce_sample_rot(const float *map, const void *table, int height, int width, int coord,
                                                const float *rot, const int *rot_identity, int A, const int *rot_index,
                                                const float *specular, const float *roughness, const float *albedo,
                                                const float *normal, const float *view, const float *uniforms,
                                                int64_t m, float *wo, float *weight, float *mix_pdf, void *stream) {
    return bounce_sample<true>(map, table, height, width, coord, {rot, rot_identity, A, rot_index}, specular, roughness,
                               albedo, normal, view, uniforms, m, wo, weight, mix_pdf, stream);
}

extern "C" int nefii_envlight_radiance(const float *map, int height, int width, int coord, const float *dirs, int64_t n,
                                       float *rgb, void *stream) {
    return radiance<false>(map, height, width, coord, {}, dirs, n, rgb, stream);
}

extern "C" int nefii_envlight_radiance_rot(const float *map, int height, int width, int coord, const float *rot,
                                           const int *rot_identity, int A, const int *rot_index, const float *dirs,
                                           int64_t n, float *rgb, void *stream) {
    return radiance<true>(map, height, width, coord, {rot, rot_identity, A, rot_index}, dirs, n, rgb, stream);
}

extern "C" int nefii_envlight_pdf(const void *table, int height, int width, int coord, const float *dirs, int64_t n,
                                  float *pdf, void *stream) {
    return pdf_of<false>(table, height, width, coord, {}, dirs, n, pdf, stream);
}

extern "C" int nefii_envlight_pdf_rot(const void *table, int height, int width, int coord, const float *rot,
                                      const int *rot_identity, int A, const int *rot_index, const float *dirs, int64_t n,
                                      float *pdf, void *stream) {
    return pdf_of<true>(table, height, width, coord, {rot, rot_identity, A, rot_index}, dirs, n, pdf, stream);
}
