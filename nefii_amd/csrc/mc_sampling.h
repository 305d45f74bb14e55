// mc_sampling.h - the BRDF half of the Monte-Carlo shading's sampling: the cosine-weighted and GGX directions and
// their pdfs, shared by nefii_mis_sample (SG-mixture light, nefii_shading.hip) and nefii_envlight_mis_sample (lat-long map
// light, nefii_envlight.hip), so that rows 0 and 1 of both samplers are the same code and agree bitwise - and the BRDF of
// the shading sum, shared by nefii_mc_shade_forward / backward and nefii_envlight_bounce_sample in the same way.
//   samplers + pdfs   code/model/path_tracing_render.py:12-156
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr float TINY = 1e-6f;
constexpr float PI_F = 3.14159265358979323846f;

struct F3 {
    float x, y, z;
};
__device__ __forceinline__ F3 f3(float x, float y, float z) { return {x, y, z}; }
__device__ __forceinline__ float dot3(const F3 &a, const F3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ F3 cross3(const F3 &a, const F3 &b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// rotate local coordinates (z = axis n) to world space (rotate_to_normal, :12-33)
__device__ __forceinline__ F3 to_world(const F3 &l, const F3 &n) {
    const F3 up = n.x > 0.9f ? f3(0.f, 1.f, 0.f) : f3(1.f, 0.f, 0.f);
    F3 t = cross3(up, n);
    const float inv = 1.f / (sqrtf(dot3(t, t)) + TINY);
    t = f3(t.x * inv, t.y * inv, t.z * inv);
    const F3 s = cross3(t, n);
    return {(l.x * t.x + l.y * s.x) + l.z * n.x, (l.x * t.y + l.y * s.y) + l.z * n.y, (l.x * t.z + l.y * s.z) + l.z * n.z};
}
__device__ __forceinline__ F3 polar(float theta, float phi) {
    const float st = sinf(theta);
    return {st * cosf(phi), st * sinf(phi), cosf(theta)};
}
__device__ __forceinline__ float pdf_cos_fn(const F3 &wi, const F3 &n) { return fmaxf(dot3(wi, n), TINY) / PI_F; }
__device__ __forceinline__ float pdf_ggx_fn(const F3 &wi, const F3 &n, const F3 &v, float rough) {
    F3 h = f3(wi.x + v.x, wi.y + v.y, wi.z + v.z);
    const float nh = sqrtf(dot3(h, h));
    h = f3(h.x / nh, h.y / nh, h.z / nh);
    if (isnan(h.x)) h.x = n.x;          // wi = -v: half vector undefined -> normal (:110-111)
    if (isnan(h.y)) h.y = n.y;
    if (isnan(h.z)) h.z = n.z;
    const float c = fmaxf(dot3(h, n), TINY);
    const float r4 = (rough * rough) * (rough * rough);
    const float root = c * c + (1.f - c * c) / r4;
    const float pdf_h = c / (PI_F * r4 * root * root);
    const float hv = fmaxf(dot3(h, v), TINY);
    return pdf_h / (4.f * hv);
}

// ---- the GGX + Lambert BRDF of the Monte-Carlo shading sum (:1406-1476): nefii_mc_shade_forward / backward and the
// recomputed bounce under the map light evaluate these two functions, so the three agree bitwise
struct BrdfGeom {      // per (point, direction) constants
    float nh, P, d1, d2, den;
};
__device__ __forceinline__ BrdfGeom brdf_geom(const F3 &nn, const F3 &vv, const F3 &wi) {
    BrdfGeom g;
    F3 h = f3(wi.x + vv.x, wi.y + vv.y, wi.z + vv.z);
    const float inv = 1.f / (sqrtf(dot3(h, h)) + TINY);
    h = f3(h.x * inv, h.y * inv, h.z * inv);
    g.nh = fmaxf(dot3(nn, h), 0.f);
    const float vh = fmaxf(dot3(vv, h), 0.f);
    g.P = exp2f(-(5.55473f * vh + 6.8316f) * vh);
    g.d1 = fmaxf(dot3(vv, nn), 0.f);
    g.d2 = fmaxf(dot3(wi, nn), 0.f);
    g.den = 4.f * g.d1 * g.d2 + TINY;
    return g;
}

// GGX D * G for one direction as a function of roughness: T is float, or a type with float's arithmetic operators
// (nefii_shading.hip's Dual<1>, found at the point of instantiation)
template <class T>
__device__ __forceinline__ T ggx_dg(const T &rough, float nh, float d1, float d2) {
    const T a2 = rough * rough;
    const T a4 = a2 * a2;
    const T root = nh * nh + (1.f - nh * nh) / a4;
    const T D = 1.f / (PI_F * a4 * root * root);
    const T k = (rough + 1.f) * (rough + 1.f) / 8.f;
    const T g = (d1 / (d1 * (1.f - k) + k + TINY)) * (d2 / (d2 * (1.f - k) + k + TINY));
    return D * g;
}

}  // namespace

// The cosine-weighted (row 0) and GGX-reflected (row 1) direction of one point and their own pdfs, declared in the
// caller's scope as w0 / p0 and w1 / p1 (and the temporaries th0, th1, h1, vh).  nn, vv: unit normal and view (F3), r: the
// roughness, u: the point's 7 uniforms (cosine reads u[0..1], GGX u[2..3]).  A macro rather than a function: expanded in
// mis_sample_kernel it is the very text the kernel had before, so that kernel compiles to the same instructions (a
// function, even force-inlined, changed its register allocation).
#define MC_SAMPLE_BRDF(nn, vv, r, u)                                                                       \
    /* --- cosine-weighted (:128-156) */                                                                   \
    const float th0 = acosf(sqrtf(1.f - u[0]));                                                            \
    const F3 w0 = to_world(polar(th0, 2.f * PI_F * u[1]), nn);                                             \
    const float p0 = cosf(th0) / PI_F;                                                                     \
    /* --- GGX half-vector (:61-103) */                                                                    \
    const float th1 = atanf((r * r) * sqrtf(u[2] / (1.f - u[2])));                                         \
    const F3 h1 = to_world(polar(th1, 2.f * PI_F * u[3]), nn);                                             \
    const float vh = dot3(vv, h1);                                                                         \
    const F3 w1 = f3(2.f * vh * h1.x - vv.x, 2.f * vh * h1.y - vv.y, 2.f * vh * h1.z - vv.z);              \
    const float p1 = pdf_ggx_fn(w1, nn, vv, r)
