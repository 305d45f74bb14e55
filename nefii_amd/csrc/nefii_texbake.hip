// nefii_texbake.hip - baking a mesh's materials into textures: the per-face-chart atlas rasterised (which face owns a texel,
// and where on that face the texel's centre lies), the baked float maps encoded to 8-bit levels, and the bilinear lookup at
// the atlas position of (face, barycentrics).  DESIGN.md 6p; include/nefii_amd.h states the atlas and the arithmetic; the
// host layer is nefii_amd/texture.py, the fp64 restatement tests/texbake_ref.py.
//
// The atlas (mirrored by texture.py and texbake_ref.py): a T x T image of n x n square cells of c texels, the margin beyond
// n c unused.  Cell q = face / 2 sits at column q % n, row q / n, origin (x0, y0) = (c (q % n), c (q / n)); texel (i, j) has
// its centre at (i + 1/2, j + 1/2), j counts rows from the top.  With p the pad and s = c - 3 p the leg:
//   even face, corners 0 1 2 at (x0 + p, y0 + p), (x0 + p + s, y0 + p), (x0 + p, y0 + p + s);
//   odd face,  corners 0 1 2 at (x0 + c - p, y0 + c - p), (x0 + c - p - s, y0 + c - p), (x0 + c - p, y0 + c - p - s);
//   a texel of the cell with (i - x0) + (j - y0) + 1 < c is the even face's, every other one the odd face's.
//
// All kernels stream: one thread per texel or sample, consecutive threads write consecutive elements, no atomics, no
// shared memory, nothing that depends on the launch geometry - the same bits from run to run.  All arithmetic that decides
// a level or a weight is fp64 (the library is built without fp contraction); every GPU store is a vector store.
//
// Ambient occlusion and bent normals: nefii_bake_ao_rays gives every texel its K cosine-weighted hemisphere
// rays (the frame is to_world of mc_sampling.h), the tracer traces them against the SDF, nefii_bake_ao_accumulate reduces the
// hits.  The host layer is texture.bake_occlusion, the restatement tests/texbake_ao_ref.py.
//
// The diffuse lightmap under a map light: nefii_bake_irradiance_rays mixes those cosine rays with rays drawn from
// the map's own distribution and gives every ray its balance-heuristic weight, nefii_bake_irradiance_accumulate sums the
// unoccluded ones.  The host layer is texture.bake_irradiance, the restatement tests/texbake_irradiance_ref.py.
#include <hip/hip_runtime.h>
#include "../../include/nefii_amd.h"

#include "hip_check.h"
#include "mc_sampling.h"
#include "envlight_table.h"

namespace {

constexpr int BLOCK = 256;
constexpr int MAX_SIZE = 8192;                       // T: T^2 = 2^26 texels stay far inside int32
constexpr int64_t MAX_COUNT = 0x7fffffffll;

__global__ void bake_clear_kernel(int *__restrict__ flags) {
    flags[0] = 0;
    flags[1] = 0;
}

__global__ __launch_bounds__(BLOCK) void bake_raster_kernel(
    const float *__restrict__ verts, int n_verts, const int *__restrict__ faces, int n_faces, int T, int n, int c, int p,
    int first, int count, int *__restrict__ owner, unsigned char *__restrict__ covered, float *__restrict__ bary,
    float *__restrict__ pos, int *__restrict__ flags) {
    const int k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= count) return;
    const int t = first + k;
    const int j = t / T, i = t - j * T;
    const int cx = i / c, cy = j / c;
    int f = -1, k1 = 0, k2 = 0;
    const int s = c - 3 * p;
    if (cx < n && cy < n) {                          // not in the margin
        const int q = cy * n + cx;
        const int li = i - cx * c, lj = j - cy * c;
        const bool even = li + lj + 1 < c;
        const int64_t ff = 2 * (int64_t)q + (even ? 0 : 1);
        if (ff < n_faces) {                          // also: the cell is one of the ceil(F / 2) used ones
            f = (int)ff;
            // twice the texel centre's offset from corner 0 along the two legs: the barycentrics are k / (2 s)
            k1 = even ? 2 * (li - p) + 1 : 2 * (c - p - li) - 1;
            k2 = even ? 2 * (lj - p) + 1 : 2 * (c - p - lj) - 1;
        }
    }
    float b1 = 0.0f, b2 = 0.0f, px = 0.0f, py = 0.0f, pz = 0.0f;
    unsigned char cov = 0;
    if (f >= 0) {
        const int k0 = 2 * s - k1 - k2;
        const double d1 = (double)k1 / (double)(2 * s), d2 = (double)k2 / (double)(2 * s), d0 = (double)k0 / (double)(2 * s);
        b1 = (float)d1, b2 = (float)d2;
        cov = (k0 >= 0 && k1 >= 0 && k2 >= 0) ? 1 : 0;
        const int i0 = faces[3 * (int64_t)f], i1 = faces[3 * (int64_t)f + 1], i2 = faces[3 * (int64_t)f + 2];
        if ((unsigned)i0 >= (unsigned)n_verts || (unsigned)i1 >= (unsigned)n_verts || (unsigned)i2 >= (unsigned)n_verts) {
            flags[0] = 1;                            // negative indices wrap above V; the vertices are never read
        } else {
            const float *a = verts + 3 * (int64_t)i0, *b = verts + 3 * (int64_t)i1, *cc = verts + 3 * (int64_t)i2;
            const double x = (d0 * (double)a[0] + d1 * (double)b[0]) + d2 * (double)cc[0];
            const double y = (d0 * (double)a[1] + d1 * (double)b[1]) + d2 * (double)cc[1];
            const double z = (d0 * (double)a[2] + d1 * (double)b[2]) + d2 * (double)cc[2];
            px = (float)x, py = (float)y, pz = (float)z;
            if (!(fabs(x) < INFINITY) || !(fabs(y) < INFINITY) || !(fabs(z) < INFINITY)) flags[1] = 1;
        }
    }
    owner[k] = f;
    covered[k] = cov;
    reinterpret_cast<float2 *>(bary)[k] = make_float2(b1, b2);
    pos[3 * (int64_t)k] = px;
    pos[3 * (int64_t)k + 1] = py;
    pos[3 * (int64_t)k + 2] = pz;
}

// floor(255 x + 0.5) for x in [0, 1] (NaN counts as 0)
__device__ inline unsigned char level_of(double x) {
    x = fmin(fmax(x, 0.0), 1.0);                     // fmax(NaN, 0) = 0
    return (unsigned char)(int)floor(255.0 * x + 0.5);
}

__global__ __launch_bounds__(BLOCK) void bake_encode_kernel(
    const float *__restrict__ albedo, const float *__restrict__ roughness, const float *__restrict__ normal,
    const int *__restrict__ owner, int64_t n, uchar4 *__restrict__ rgba_albedo, uchar4 *__restrict__ rgba_normal,
    unsigned char *__restrict__ grey_roughness) {
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n) return;
    uchar4 a = make_uchar4(0, 0, 0, 0), nn = make_uchar4(0, 0, 0, 0);
    unsigned char r = 0;
    if (owner[k] >= 0) {
        unsigned char la[3], ln[3];
        for (int ch = 0; ch < 3; ++ch) {
            const double v = fmax((double)albedo[3 * k + ch], 0.0);          // the render panel's tone map
            la[ch] = level_of(pow(v, 1.0 / 2.2));
            ln[ch] = level_of(0.5 * (double)normal[3 * k + ch] + 0.5);
        }
        a = make_uchar4(la[0], la[1], la[2], 255);
        nn = make_uchar4(ln[0], ln[1], ln[2], 255);
        r = level_of((double)roughness[k]);
    }
    rgba_albedo[k] = a;
    rgba_normal[k] = nn;
    grey_roughness[k] = r;
}

template <int C>
__global__ __launch_bounds__(BLOCK) void texture_sample_kernel(const float *__restrict__ tex, int T,
                                                               const int *__restrict__ face,
                                                               const double *__restrict__ bary, int n, int c, int p,
                                                               int64_t count, float *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= count) return;
    const int f = face[k];
    double acc[C];
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0.0;
    if (f >= 0 && f / 2 < n * n) {                   // a face without a cell gives zeros
        const int q = f / 2;
        const double x0 = (double)(c * (q % n)), y0 = (double)(c * (q / n));
        const double s = (double)(c - 3 * p);
        const double b0 = bary[3 * k], b1 = bary[3 * k + 1], b2 = bary[3 * k + 2];
        double ax, ay, dir;                          // corner 0 and the direction of the legs
        if ((f & 1) == 0) ax = x0 + (double)p, ay = y0 + (double)p, dir = 1.0;
        else ax = x0 + (double)(c - p), ay = y0 + (double)(c - p), dir = -1.0;
        const double x = (b0 * ax + b1 * (ax + dir * s)) + b2 * ax;
        const double y = (b0 * ay + b1 * ay) + b2 * (ay + dir * s);
        const double u = x - 0.5, v = y - 0.5;
        const double fu = floor(u), fv = floor(v);
        const double wx = u - fu, wy = v - fv;
        // clamped to the image while still doubles: barycentrics far outside [0, 1] (or not finite) never index past it
        const double hi = (double)(T - 1);
        const int i0 = (int)fmin(fmax(fu, 0.0), hi), i1 = (int)fmin(fmax(fu + 1.0, 0.0), hi);
        const int j0 = (int)fmin(fmax(fv, 0.0), hi), j1 = (int)fmin(fmax(fv + 1.0, 0.0), hi);
        const double w00 = (1.0 - wx) * (1.0 - wy), w10 = wx * (1.0 - wy), w01 = (1.0 - wx) * wy, w11 = wx * wy;
        const float *t00 = tex + ((int64_t)j0 * T + i0) * C, *t10 = tex + ((int64_t)j0 * T + i1) * C;
        const float *t01 = tex + ((int64_t)j1 * T + i0) * C, *t11 = tex + ((int64_t)j1 * T + i1) * C;
        for (int ch = 0; ch < C; ++ch)
            acc[ch] = ((w00 * (double)t00[ch] + w10 * (double)t10[ch]) + w01 * (double)t01[ch]) + w11 * (double)t11[ch];
    }
    for (int ch = 0; ch < C; ++ch) out[k * C + ch] = (float)acc[ch];
}

// ---- ambient occlusion and bent normals: per-texel hemisphere rays and their reduction -----------------------
constexpr int MAX_AO_RAYS = 1024;

__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// One thread per texel, a loop over the K samples: row s of dirs (and uniforms) is written by consecutive threads at
// consecutive elements.  A direction depends on (texel index, s, K, seed) and the texel's normal alone.
__global__ __launch_bounds__(BLOCK) void bake_ao_rays_kernel(
    const float *__restrict__ pos, const float *__restrict__ normal, const float *__restrict__ sdf,
    const float *__restrict__ gnorm, const int64_t *__restrict__ texel, int64_t m, int K, uint32_t seed, float bias,
    float *__restrict__ origins, float *__restrict__ dirs, float2 *__restrict__ uniforms) {
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= m) return;
    const F3 x = f3(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]);
    const F3 n = f3(normal[3 * k], normal[3 * k + 1], normal[3 * k + 2]);
    // a first-order lift onto the level set plus the offset along the normal
    const float t = bias - sdf[k] / gnorm[k];
    origins[3 * k] = x.x + t * n.x;
    origins[3 * k + 1] = x.y + t * n.y;
    origins[3 * k + 2] = x.z + t * n.z;
    const uint32_t h0 = lowbias32((uint32_t)texel[k] ^ lowbias32(seed));
    const uint32_t h1 = lowbias32(h0 + 0x9e3779b9u);
    const float r0 = (float)(h0 >> 8) * 0x1p-24f, r1 = (float)(h1 >> 8) * 0x1p-24f;      // exact
    // to_world's frame degenerates at n = (-1, 0, 0) (its tangent cross((1, 0, 0), n) vanishes): below -0.9 the frame of -n
    // is used with the local z mirrored, l.x t' + l.y s' + (-l.z)(-n) - as well conditioned as the n.x > 0.9 branch
    const bool flip = n.x < -0.9f;
    const F3 axis = flip ? f3(-n.x, -n.y, -n.z) : n;
    for (int s = 0; s < K; ++s) {
        float u0 = r0 + ((float)s + 0.5f) / (float)K;                   // a rotated stratified sequence
        if (u0 >= 1.f) u0 -= 1.f;
        u0 = fminf(u0, 1.f - 0x1p-24f);
        float u1 = r1 + (float)__brev((uint32_t)s) * 0x1p-32f;          // the rotated van der Corput sequence
        if (u1 >= 1.f) u1 -= 1.f;
        const float phi = 2.f * PI_F * u1;
        const float r = sqrtf(u0), lz = sqrtf(1.f - u0);                // cosine-weighted, well conditioned at the pole
        F3 w = to_world(f3(r * cosf(phi), r * sinf(phi), flip ? -lz : lz), axis);
        // to_world's tangents are short by TINY / |t| (up to 2.3e-6): back to unit length
        const float inv = 1.f / sqrtf(dot3(w, w));
        w = f3(w.x * inv, w.y * inv, w.z * inv);
        const int64_t e = (int64_t)s * m + k;
        dirs[3 * e] = w.x;
        dirs[3 * e + 1] = w.y;
        dirs[3 * e + 2] = w.z;
        if (uniforms) uniforms[e] = make_float2(u0, u1);
    }
}

// One thread per texel, a loop over s in order: row s of every input is read by consecutive threads.
__global__ __launch_bounds__(BLOCK) void bake_ao_accumulate_kernel(
    const unsigned char *__restrict__ hit, const float *__restrict__ hit_pts, const float *__restrict__ origins,
    const float *__restrict__ dirs, const float *__restrict__ normal, int64_t m, int K, float distance,
    float *__restrict__ ao, float *__restrict__ bent) {
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= m) return;
    const float ox = origins[3 * k], oy = origins[3 * k + 1], oz = origins[3 * k + 2];
    const float far2 = distance * distance;
    int occluded = 0;
    double bx = 0.0, by = 0.0, bz = 0.0;
    for (int s = 0; s < K; ++s) {
        const int64_t e = (int64_t)s * m + k;
        const float dx = hit_pts[3 * e] - ox, dy = hit_pts[3 * e + 1] - oy, dz = hit_pts[3 * e + 2] - oz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const float wx = dirs[3 * e], wy = dirs[3 * e + 1], wz = dirs[3 * e + 2];
        if (hit[e] != 0 && (distance <= 0.f || d2 <= far2)) {           // a miss's point is never looked at
            ++occluded;
        } else {
            bx += (double)wx;
            by += (double)wy;
            bz += (double)wz;
        }
    }
    ao[k] = (float)(K - occluded) / (float)K;
    const double len = sqrt((bx * bx + by * by) + bz * bz);
    float ex = normal[3 * k], ey = normal[3 * k + 1], ez = normal[3 * k + 2];
    if (occluded < K && len > 0.0) ex = (float)(bx / len), ey = (float)(by / len), ez = (float)(bz / len);
    bent[3 * k] = ex;
    bent[3 * k + 1] = ey;
    bent[3 * k + 2] = ez;
}

// ---- the diffuse lightmap under a map light: the rays of both techniques with their balance-heuristic weights,
// and the reduction of the traced hits.  The table is read with the renderer's own code (envlight_table.h).
//
// The two halves of bake_ao_rays_kernel's loop body, operation for operation (that kernel keeps its own text, and with it its
// instructions): sample s of K of a texel's sequence - stratified in the first dimension, van der Corput in the second, both
// rotated by the texel's own offsets (r0, r1) ...
__device__ __forceinline__ void rotated_sample(float r0, float r1, int s, int K, float &u0, float &u1) {
    u0 = r0 + ((float)s + 0.5f) / (float)K;                             // a rotated stratified sequence
    if (u0 >= 1.f) u0 -= 1.f;
    u0 = fminf(u0, 1.f - 0x1p-24f);
    u1 = r1 + (float)__brev((uint32_t)s) * 0x1p-32f;                    // the rotated van der Corput sequence
    if (u1 >= 1.f) u1 -= 1.f;
}

// ... and the cosine-weighted direction of (u0, u1) about `axis` (the normal, or its negative with the local z mirrored: flip)
__device__ __forceinline__ F3 cosine_direction(float u0, float u1, const F3 &axis, bool flip) {
    const float phi = 2.f * PI_F * u1;
    const float r = sqrtf(u0), lz = sqrtf(1.f - u0);                    // cosine-weighted, well conditioned at the pole
    F3 w = to_world(f3(r * cosf(phi), r * sinf(phi), flip ? -lz : lz), axis);
    // to_world's tangents are short by TINY / |t| (up to 2.3e-6): back to unit length
    const float inv = 1.f / sqrtf(dot3(w, w));
    return f3(w.x * inv, w.y * inv, w.z * inv);
}

// One thread per texel, a loop over the K = K_cos + K_map samples, row s of dirs, weight (and uniforms) written by consecutive
// threads at consecutive elements.  Rows s < K_cos are bake_ao_rays_kernel's for K := K_cos (the same operations in the same
// order: the same bits); rows s >= K_cos invert the map's CDFs as envlight_mis_kernel does, on a second rotated sequence whose
// offsets are hashes chained off the first two.  weight = L c / (K_cos c / pi + K_map p_map), c = max(n . w, 0): with it the
// irradiance is the plain sum of the unoccluded rows (the multi-sample balance heuristic), and exactly 0 where c = 0.
__global__ __launch_bounds__(BLOCK) void bake_irradiance_rays_kernel(
    const float *__restrict__ pos, const float *__restrict__ normal, const float *__restrict__ sdf,
    const float *__restrict__ gnorm, const int64_t *__restrict__ texel, int64_t m, int K_cos, int K_map, uint32_t seed,
    float bias, const float *__restrict__ map, Table tb, int H, int W, int coord, const float *__restrict__ rot,
    int rot_identity, float *__restrict__ origins, float *__restrict__ dirs, float *__restrict__ weight,
    float2 *__restrict__ uniforms) {
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= m) return;
    Rot R{{}, true};
    if (rot && !rot_identity) {
#pragma unroll
        for (int q = 0; q < 9; ++q) R.m[q] = rot[q];
        R.identity = false;
    }
    const F3 x = f3(pos[3 * k], pos[3 * k + 1], pos[3 * k + 2]);
    const F3 n = f3(normal[3 * k], normal[3 * k + 1], normal[3 * k + 2]);
    const float t = bias - sdf[k] / gnorm[k];
    origins[3 * k] = x.x + t * n.x;
    origins[3 * k + 1] = x.y + t * n.y;
    origins[3 * k + 2] = x.z + t * n.z;
    const uint32_t h0 = lowbias32((uint32_t)texel[k] ^ lowbias32(seed));
    const uint32_t h1 = lowbias32(h0 + 0x9e3779b9u);
    const uint32_t h2 = lowbias32(h1 + 0x9e3779b9u);
    const uint32_t h3 = lowbias32(h2 + 0x9e3779b9u);
    const float r0 = (float)(h0 >> 8) * 0x1p-24f, r1 = (float)(h1 >> 8) * 0x1p-24f;      // exact
    const float r2 = (float)(h2 >> 8) * 0x1p-24f, r3 = (float)(h3 >> 8) * 0x1p-24f;
    const bool flip = n.x < -0.9f;
    const F3 axis = flip ? f3(-n.x, -n.y, -n.z) : n;
    const float k_cos = (float)K_cos, k_map = (float)K_map;
    for (int s = 0; s < K_cos + K_map; ++s) {
        float u0, u1, p_map;
        F3 w;
        int ti, tj;
        if (s < K_cos) {
            rotated_sample(r0, r1, s, K_cos, u0, u1);
            w = cosine_direction(u0, u1, axis, flip);
            const Texel tx = texel_of(to_light(R, w), H, W, coord);
            ti = tx.i, tj = tx.j;
            p_map = solid_angle_pdf(texel_prob(tb, W, ti, tj), H, W, tx.sin_phi);
        } else {      // row by the marginal (u0), column by that row's conditional (u1), continuous inside the texel
            rotated_sample(r2, r3, s - K_cos, K_map, u0, u1);
            float dv, du;
            ti = sample_cdf(tb.M, H, u0, dv);
            tj = sample_cdf(tb.C + (int64_t)ti * W, W, u1, du);
            const float v2 = ((float)ti + dv) / (float)H, u2 = ((float)tj + du) / (float)W;
            w = to_world_rot(R, direction_of(u2, v2, coord));
            p_map = solid_angle_pdf(texel_prob(tb, W, ti, tj), H, W, sinpif(v2));
        }
        const float c = fmaxf(dot3(n, w), 0.f);
        const float den = k_cos * (c / PI_F) + k_map * p_map;
        const float g = c > 0.f && den > 0.f ? c / den : 0.f;           // (a map row at a pole of the map has p_map = 0)
        float L[3];
        copy_texel(map, W, ti, tj, L);
        const int64_t e = (int64_t)s * m + k;
        dirs[3 * e] = w.x;
        dirs[3 * e + 1] = w.y;
        dirs[3 * e + 2] = w.z;
        weight[3 * e] = g > 0.f ? L[0] * g : 0.f;
        weight[3 * e + 1] = g > 0.f ? L[1] * g : 0.f;
        weight[3 * e + 2] = g > 0.f ? L[2] * g : 0.f;
        if (uniforms) uniforms[e] = make_float2(u0, u1);
    }
}

// One thread per texel, a loop over s in order.  A row whose three weights are zero is never looked up in hit.  The noise is
// the standard error of the luminance estimate: per technique, n_t times the sample variance of its n_t contributions.
__global__ __launch_bounds__(BLOCK) void bake_irradiance_accumulate_kernel(
    const unsigned char *__restrict__ hit, const float *__restrict__ weight, int64_t m, int K_cos, int K_map,
    float *__restrict__ irradiance, float *__restrict__ noise) {
    const int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (k >= m) return;
    double ex = 0.0, ey = 0.0, ez = 0.0, var = 0.0;
    int s = 0;
    for (int tech = 0; tech < 2; ++tech) {
        const int n = tech == 0 ? K_cos : K_map;
        double S = 0.0, Q = 0.0;
        for (const int end = s + n; s < end; ++s) {
            const int64_t e = (int64_t)s * m + k;
            const float wx = weight[3 * e], wy = weight[3 * e + 1], wz = weight[3 * e + 2];
            if (wx == 0.f && wy == 0.f && wz == 0.f) continue;
            if (hit[e] != 0) continue;
            ex += (double)wx;
            ey += (double)wy;
            ez += (double)wz;
            const double y = (((double)wx + (double)wy) + (double)wz) / 3.0;
            S += y;
            Q += y * y;
        }
        if (n >= 2) var += (Q - S * S / (double)n) * ((double)n / (double)(n - 1));
    }
    irradiance[3 * k] = (float)ex;
    irradiance[3 * k + 1] = (float)ey;
    irradiance[3 * k + 2] = (float)ez;
    noise[k] = (float)sqrt(fmax(var, 0.0));
}

bool atlas_ok(int T, int n, int c, int p) {
    if (T < 7 || T > MAX_SIZE || n < 1 || c < 1 || p < 2) return false;
    if ((int64_t)n * c > T || c - 3 * p < 1) return false;
    return true;
}

}  // namespace

extern "C" int nefii_bake_raster(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, int T, int n,
                                 int c, int p, int64_t first, int64_t count, int32_t *owner, uint8_t *covered, float *bary,
                                 float *pos, int32_t *flags, void *stream) {
    if (!verts || !faces || !owner || !covered || !bary || !pos || !flags) return NEFII_E_ARG;
    if (n_verts < 0 || n_verts > MAX_COUNT || n_faces < 0 || 3 * n_faces > MAX_COUNT) return NEFII_E_SHAPE;
    if ((uintptr_t)bary & 7) return NEFII_E_ARG;                             // written as pairs of floats
    if (!atlas_ok(T, n, c, p)) return NEFII_E_SHAPE;
    if (n_faces > 2 * (int64_t)n * n) return NEFII_E_SHAPE;                  // the atlas holds two faces per cell
    if (first < 0 || count < 0 || first + count > (int64_t)T * T) return NEFII_E_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bake_clear_kernel, dim3(1), dim3(1), 0, s, flags);
    HIP_CHECK_LAUNCH();
    if (count == 0) return 0;
    hipLaunchKernelGGL(bake_raster_kernel, dim3((unsigned)((count + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, verts,
                       (int)n_verts, faces, (int)n_faces, T, n, c, p, (int)first, (int)count, owner, covered, bary, pos, flags);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_bake_encode(const float *albedo, const float *roughness, const float *normal, const int32_t *owner,
                                 int64_t n, uint8_t *rgba_albedo, uint8_t *rgba_normal, uint8_t *grey_roughness,
                                 void *stream) {
    if (!albedo || !roughness || !normal || !owner || !rgba_albedo || !rgba_normal || !grey_roughness) return NEFII_E_ARG;
    if (n < 0 || n > (int64_t)MAX_SIZE * MAX_SIZE) return NEFII_E_SHAPE;
    if (((uintptr_t)rgba_albedo | (uintptr_t)rgba_normal) & 3) return NEFII_E_ARG;      // written as 32-bit words
    if (n == 0) return 0;
    hipLaunchKernelGGL(bake_encode_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                       albedo, roughness, normal, owner, n, reinterpret_cast<uchar4 *>(rgba_albedo),
                       reinterpret_cast<uchar4 *>(rgba_normal), grey_roughness);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_texture_sample(const float *tex, int T, int C, const int32_t *face, const double *bary, int n, int c,
                                    int p, int64_t count, float *out, void *stream) {
    if (!tex || !face || !bary || !out) return NEFII_E_ARG;
    if (C < 1 || C > 4 || !atlas_ok(T, n, c, p)) return NEFII_E_SHAPE;
    if (count < 0 || count > MAX_COUNT) return NEFII_E_SHAPE;
    if (count == 0) return 0;
    const dim3 grid((unsigned)((count + BLOCK - 1) / BLOCK)), block(BLOCK);
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1: hipLaunchKernelGGL(texture_sample_kernel<1>, grid, block, 0, s, tex, T, face, bary, n, c, p, count, out); break;
        case 2: hipLaunchKernelGGL(texture_sample_kernel<2>, grid, block, 0, s, tex, T, face, bary, n, c, p, count, out); break;
        case 3: hipLaunchKernelGGL(texture_sample_kernel<3>, grid, block, 0, s, tex, T, face, bary, n, c, p, count, out); break;
        default: hipLaunchKernelGGL(texture_sample_kernel<4>, grid, block, 0, s, tex, T, face, bary, n, c, p, count, out); break;
    }
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_bake_ao_rays(const float *pos, const float *normal, const float *sdf, const float *gnorm,
                                  const int64_t *texel, int64_t m, int K, uint32_t seed, float bias, float *origins, float *dirs,
                                  float *uniforms, void *stream) {
    if (!pos || !normal || !sdf || !gnorm || !texel || !origins || !dirs) return NEFII_E_ARG;     // uniforms may be NULL
    if ((uintptr_t)uniforms & 7) return NEFII_E_ARG;                         // written as pairs of floats
    if (K < 1 || K > MAX_AO_RAYS || m < 0 || m > MAX_COUNT) return NEFII_E_SHAPE;
    if (m == 0) return 0;
    hipLaunchKernelGGL(bake_ao_rays_kernel, dim3((unsigned)((m + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, pos,
                       normal, sdf, gnorm, texel, m, K, seed, bias, origins, dirs, reinterpret_cast<float2 *>(uniforms));
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_bake_ao_accumulate(const uint8_t *hit, const float *hit_pts, const float *origins, const float *dirs,
                                        const float *normal, int64_t m, int K, float distance, float *ao, float *bent,
                                        void *stream) {
    if (!hit || !hit_pts || !origins || !dirs || !normal || !ao || !bent) return NEFII_E_ARG;
    if (K < 1 || K > MAX_AO_RAYS || m < 0 || m > MAX_COUNT) return NEFII_E_SHAPE;
    if (m == 0) return 0;
    hipLaunchKernelGGL(bake_ao_accumulate_kernel, dim3((unsigned)((m + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream,
                       hit, hit_pts, origins, dirs, normal, m, K, distance, ao, bent);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_bake_irradiance_rays(const float *pos, const float *normal, const float *sdf, const float *gnorm,
                                          const int64_t *texel, int64_t m, int K_cos, int K_map, uint32_t seed, float bias,
                                          const float *map, const void *table, int height, int width, int coord, const float *rot,
                                          int rot_identity, float *origins, float *dirs, float *weight, float *uniforms,
                                          void *stream) {
    if (!pos || !normal || !sdf || !gnorm || !texel || !map || !table || !origins || !dirs || !weight) return NEFII_E_ARG;
    if ((uintptr_t)uniforms & 7) return NEFII_E_ARG;                         // written as pairs of floats; may be NULL, as rot
    if (coord != 0 && coord != 1) return NEFII_E_ARG;
    if (K_cos < 0 || K_map < 0 || K_cos > MAX_AO_RAYS || K_map > MAX_AO_RAYS) return NEFII_E_SHAPE;
    if (K_cos + K_map < 1 || K_cos + K_map > MAX_AO_RAYS || m < 0 || m > MAX_COUNT) return NEFII_E_SHAPE;
    if (bad_shape(height, width)) return NEFII_E_SHAPE;
    if (m == 0) return 0;
    hipLaunchKernelGGL(bake_irradiance_rays_kernel, dim3((unsigned)((m + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0,
                       (hipStream_t)stream, pos, normal, sdf, gnorm, texel, m, K_cos, K_map, seed, bias, map,
                       table_of(table, height), height, width, coord, rot, rot_identity, origins, dirs, weight,
                       reinterpret_cast<float2 *>(uniforms));
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" int nefii_bake_irradiance_accumulate(const uint8_t *hit, const float *weight, int64_t m, int K_cos, int K_map,
                                                float *irradiance, float *noise, void *stream) {
    if (!hit || !weight || !irradiance || !noise) return NEFII_E_ARG;
    if (K_cos < 0 || K_map < 0 || K_cos > MAX_AO_RAYS || K_map > MAX_AO_RAYS) return NEFII_E_SHAPE;
    if (K_cos + K_map < 1 || K_cos + K_map > MAX_AO_RAYS || m < 0 || m > MAX_COUNT) return NEFII_E_SHAPE;
    if (m == 0) return 0;
    hipLaunchKernelGGL(bake_irradiance_accumulate_kernel, dim3((unsigned)((m + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0,
                       (hipStream_t)stream, hit, weight, m, K_cos, K_map, irradiance, noise);
    HIP_CHECK_LAUNCH();
    return 0;
}
