// envlight_table.h - reading a map light's sampling table on the device: the texel under a direction, a
// texel's probability and solid-angle density from the stored fp32 CDFs, their continuous inversion, the direction of map
// coordinates, and the rotation in and out of the light's frame.  Shared by nefii_envlight.hip (the renderer's samplers and
// lookups) and nefii_texbake.hip (the irradiance bake), so that both read the table with the same code.
//
// Table (nefii_envlight_table_bytes): M [H] float | C [H][W] float | row sums [H] double, each part 256-byte aligned.
#pragma once
#include <hip/hip_runtime.h>
#include "mc_sampling.h"

namespace {

constexpr float DV_MAX = 1.f - 5.9604645e-8f;      // 1 - 2^-24: a continuous offset stays inside its texel

bool bad_shape(int H, int W) { return H < 1 || W < 1 || (int64_t)H * W >= ((int64_t)1 << 31); }

struct Table {
    const float *M, *C;
};
int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }
int64_t c_offset(int H) { return align256((int64_t)H * 4); }                         // C after M
Table table_of(const void *table, int H) {
    const char *b = (const char *)table;
    return {(const float *)b, (const float *)(b + c_offset(H))};
}

// ---- lookups --------------------------------------------------------------------------------------------------------
// clamp(floor(x), 0, n - 1); NaN -> 0
__device__ __forceinline__ int cell(float x, int n) {
    const float f = fmaxf(floorf(x), 0.f);
    return f < (float)n ? min((int)f, n - 1) : n - 1;
}

struct Texel {
    int i, j;
    float sin_phi;     // of the direction itself
};

// the texel under direction d (normalised first, norm clamped at 1e-8).  phi = atan2(rho, up) is acos(up) of the unit
// vector, evaluated without acos's loss near the poles; sin phi = rho / |(rho, up)|.
__device__ __forceinline__ Texel texel_of(F3 d, int H, int W, int coord) {
    const float inv = 1.f / fmaxf(sqrtf(dot3(d, d)), 1e-8f);
    d = f3(d.x * inv, d.y * inv, d.z * inv);
    const float up = coord == 0 ? d.y : d.z;
    const float side = coord == 0 ? d.z : d.y;        // the second horizontal axis
    const float rho = sqrtf(d.x * d.x + side * side);
    const float phi = atan2f(rho, up);
    const float theta = atan2f(side, d.x);
    float u;
    if (coord == 0) {
        u = (theta + 0.5f * PI_F) / (2.f * PI_F);
        u = u - floorf(u);
    } else {
        u = (PI_F - theta) / (2.f * PI_F);
    }
    const float r = sqrtf(rho * rho + up * up);
    Texel t;
    t.i = cell(phi / PI_F * (float)H, H);
    t.j = cell(u * (float)W, W);
    t.sin_phi = rho > 0.f ? rho / r : 0.f;
    return t;
}

// P(i, j) from the stored CDFs
__device__ __forceinline__ float texel_prob(const Table &tb, int W, int i, int j) {
    const float *c = tb.C + (int64_t)i * W;
    const float pm = tb.M[i] - (i > 0 ? tb.M[i - 1] : 0.f);
    const float pc = c[j] - (j > 0 ? c[j - 1] : 0.f);
    return pm * pc;
}

__device__ __forceinline__ float solid_angle_pdf(float P, int H, int W, float sin_phi) {
    return sin_phi > 0.f ? P * ((float)H * (float)W) / (2.f * PI_F * PI_F * sin_phi) : 0.f;
}

// first k in [0, n) with cdf[k] > x (n - 1 if none), and the continuous offset inside it
__device__ __forceinline__ int sample_cdf(const float *cdf, int n, float x, float &d) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    const float prev = lo > 0 ? cdf[lo - 1] : 0.f;
    const float w = cdf[lo] - prev;
    d = w > 0.f ? (x - prev) / w : 0.f;
    d = fminf(fmaxf(d, 0.f), DV_MAX);
    return lo;
}

__device__ __forceinline__ F3 direction_of(float u, float v, int coord) {
    const float sp = sinpif(v), cp = cospif(v);
    const float s2 = sinpif(2.f * u), c2 = cospif(2.f * u);
    if (coord == 0) return f3(s2 * sp, cp, -c2 * sp);        // theta = 2 pi u - pi/2: cos = sin 2pi u, sin = -cos 2pi u
    return f3(-c2 * sp, s2 * sp, cp);                         // theta = pi - 2 pi u:  cos = -cos 2pi u, sin = sin 2pi u
}

__device__ __forceinline__ void copy_texel(const float *__restrict__ map, int W, int i, int j, float *out) {
    const float *p = map + ((int64_t)i * W + j) * 3;
    out[0] = p[0], out[1] = p[1], out[2] = p[2];
}

// ---- the rotation: R is world-from-light, row-major; identity: the nine floats are exactly the identity's,
// and the products are skipped (1 x + 0 y + 0 z would turn -0 into +0 and move atan2f(side, x) across the seam)
struct Rot {
    float m[9];
    bool identity;
};

// The products run in fp64 and are rounded once: every component then carries its OWN relative rounding error, so
// sin(phi) = rho / r of a rotated direction near a pole is as good as the unrotated one's (a 3-term fp32 product would
// leave an absolute 1e-7 in rho), and the rotated direction adds half an ulp to direction_of's error.
__device__ __forceinline__ float dot3d(float a, float b, float c, const F3 &d) {
    return (float)((double)a * (double)d.x + (double)b * (double)d.y + (double)c * (double)d.z);
}

// R^T d: world -> light, on the way into texel_of
__device__ __forceinline__ F3 to_light(const Rot &R, F3 d) {
    if (R.identity) return d;
    return f3(dot3d(R.m[0], R.m[3], R.m[6], d), dot3d(R.m[1], R.m[4], R.m[7], d), dot3d(R.m[2], R.m[5], R.m[8], d));
}

// R d: light -> world, on the way out of direction_of
__device__ __forceinline__ F3 to_world_rot(const Rot &R, F3 d) {
    if (R.identity) return d;
    return f3(dot3d(R.m[0], R.m[1], R.m[2], d), dot3d(R.m[3], R.m[4], R.m[5], d), dot3d(R.m[6], R.m[7], R.m[8], d));
}

}  // namespace
