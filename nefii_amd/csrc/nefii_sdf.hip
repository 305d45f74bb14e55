// nefii_sdf.hip - what is built FROM the SDF net once, outside the tracer's rounds: the fragment streams its tile evaluators
// read (nefii_sdf_stream_bytes, nefii_pack_sdf_stream) and the SDF interval grid (nefii_sdf_bound_grid_*).
// The evaluators themselves - the rounds', the point lists' (nefii_sdf_eval*) and the value + gradient kernel - stay together
// in nefii_tracer.hip: they share the tile functions of mlp_tile.h, and the compiler specialises a tile function that has a
// single caller in its file, so a kernel moved away from its siblings - and every sibling left behind - compiles to other code.
#include "sdf_launch.h"
#include "hip_check.h"

using namespace nefii;

// ---- shapes and sizes of the fragment streams (host) ---------------------------------------------
namespace nefii {
// shapes the pipelined kernels take: every hidden layer W wide (512; 256 with the 16x16x32 layout only), inputs of 0 or
// W previous features plus 0 or 64 encoding columns, a W-deep last layer.  Returns the feature tiles per wave
// (W / 128), 0 when the shape does not fit.
// one encoded input - the point - and no feature vector ...
static bool point_input_only(const nefii_mlp *m) {
    return m->enc_freqs[0] >= 0 && m->enc_freqs[1] < 0 && m->enc_freqs[2] < 0 && m->feat_width == 0;
}
// ... and a first layer that reads the encoding alone: the nets the SDF evaluators take
bool sdf_net_ok(const nefii_mlp *m) { return point_input_only(m) && m->layer[0].k_x == 0; }

int shape16p(const nefii_mlp *m) {
    const int NH = m->n_layers - 1;
    if (NH < 1) return 0;
    const int W = m->layer[0].n_pad;
    if (W != 512 && !(W == 256 && m->reserved == 1)) return 0;
    for (int l = 0; l < NH; ++l) {
        const nefii_layer &L = m->layer[l];
        if (L.n_pad != W || (L.k_x != 0 && L.k_x != W) || (L.k_e != 0 && L.k_e != 64) || L.k_x + L.k_e == 0) return 0;
    }
    const nefii_layer &Ll = m->layer[NH];
    return Ll.k_x == W && Ll.k_e == 0 ? W / 128 : 0;
}
int fits16p(const nefii_mlp *m) { return m->w_stream ? shape16p(m) : 0; }

static int layer_units(const nefii_layer &L, int ft) { return ft == 2 ? q_units<2>(L) : (L.k_x + L.k_e) >> 4; }
int stream_steps(const nefii_mlp *m) {
    const int ft = shape16p(m);
    int G = 0;
    for (int l = 0; l < m->n_layers - 1; ++l) G += layer_units(m->layer[l], ft);
    return G;
}
// units of the second, K-padded copy the deep-prefetch 32-query instance reads (512-wide nets, 16x16x32 layout)
static int stream_steps8(const nefii_mlp *m) {
    if (shape16p(m) != 4 || m->reserved != 1) return 0;
    int G = 0;
    for (int l = 0; l < m->n_layers - 1; ++l) G += q_units8(m->layer[l]);
    return G;
}
// units of the single-pass copy (0: the net has none)
static int stream_steps_sp(const nefii_mlp *m) {
    if (!shape16p(m) || m->reserved != 1) return 0;
    int G = 0;
    for (int l = 0; l < m->n_layers - 1; ++l) G += s_units(m->layer[l]);
    return G;
}

// ---- fourth copy: the value + gradient kernel's stream (sdf_value_grad16q_kernel) ------------------------------------------
// Softplus nets of the pipelined shapes (512- or 256-wide) with transposed fragments on every layer.  Per wave: the
// forward units of the plain 16x16x32 stream, then the BACKWARD units - for l = NH-1 .. 1 the units of the transposed
// layer (contraction over layer l's W outputs, the wave's share of its W hidden inputs as output features), gathered
// from nefii_layer.w_bwd_f16x3 - so that one cursor runs forward, backward, and wraps to the next tile's forward.
// Returns the feature tiles per wave (4 / 2), 0 when the net does not take the kernel.
int vg_shape(const nefii_mlp *m) {
    const int ft = shape16p(m);
    if (!ft || m->reserved != 1 || m->act != NEFII_ACT_SOFTPLUS100) return 0;
    const int NH = m->n_layers - 1;
    if (NH < 2 || NH > 12 || m->layer[0].k_e != 64) return 0;
    if (!point_input_only(m)) return 0;
    for (int l = 0; l <= NH; ++l)
        if (!m->layer[l].w_f16x3 || !m->layer[l].w_bwd_f16x3 || !m->layer[l].bias) return 0;
    return ft;
}
int vg_units_bwd(const nefii_mlp *m) {
    const int ft = vg_shape(m);
    return ft ? (m->n_layers - 2) * vg_units_layer(m->layer[0].n_pad, ft) : 0;
}
// half8 offset of the copy in w_stream
size_t vg_stream_offset(const nefii_mlp *m) {
    return (size_t)8 * (stream_steps(m) + stream_steps8(m)) * 256 + (size_t)8 * stream_steps_sp(m) * shape16p(m) * 64;
}

// bytes of the first four copies (the fifth - the "16f" evaluator's - follows them)
size_t stream_bytes_1to4(const nefii_mlp *h_sdf) {
    size_t units_vg = 0;
    if (vg_shape(h_sdf)) units_vg = (size_t)stream_steps(h_sdf) + vg_units_bwd(h_sdf);
    return (size_t)8 * (stream_steps(h_sdf) + stream_steps8(h_sdf) + units_vg) * 256 * sizeof(half8) +
           (size_t)8 * stream_steps_sp(h_sdf) * shape16p(h_sdf) * 64 * sizeof(half8);
}
}  // namespace nefii

namespace {

__device__ __forceinline__ int layer_units_dev(const nefii_layer &L, int ft) {
    return ft == 2 ? q_units<2>(L) : (L.k_x + L.k_e) >> 4;
}

// layout 0 (32x32x16 fragments): dst[(wave*G + g)*256 + i] <- the 4 KiB fragment block of (k-step g of the layer
// sequence, column tiles 2 wave, 2 wave + 1), a straight copy.
// layout 1 (16x16x32 fragments, nefii_mlp.reserved == 1), 512-wide: unit g is a HALF step (32-deep k-step g/2 of the
// layer sequence, feature-tile pair g&1): dst[((wave*G + g)*4 + 2 f + part)*64 + lane][j] = W[n = 64 wave + 16 (2 (g&1)
// + f) + (lane&15)][k = 32 s32 + 8 (lane>>4) + j], gathered from the layer's 32x32x16 fragments (one source half8 per
// destination half8).  256-wide: unit g is a whole 32-deep k-step of the layer's K padded to a multiple of 128,
// n = 32 wave + 16 f + (lane&15); k-steps past the layer's own K hold zeros.
// Gw: units per wave of the destination copy (G, or more when other units follow in the same copy).
__global__ void pack_sdf_stream_kernel(nefii_mlp m, half8 *__restrict__ dst, int Gw, int ft, int padded) {
    const int g = blockIdx.x, wave = blockIdx.y, G = Gw;
    int l = 0, s = g;
    while (s >= (padded ? q_units8(m.layer[l]) : layer_units_dev(m.layer[l], ft)))
        s -= padded ? q_units8(m.layer[l]) : layer_units_dev(m.layer[l], ft), ++l;
    const half8 *w = reinterpret_cast<const half8 *>(m.layer[l].w_f16x3);
    if (m.reserved != 1) {
        const half8 *src = w + ((size_t)s * 16 + 2 * wave) * 2 * 64;
        dst[((size_t)wave * G + g) * 256 + threadIdx.x] = src[threadIdx.x];
        return;
    }
    const int frag = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = frag >> 1, part = frag & 1, kg = lane >> 4;
    if (ft == 2) {
        const int n = 32 * wave + 16 * f + (lane & 15);
        const int s16 = 2 * s + (kg >> 1), t = n >> 5, lane_src = (n & 31) + 32 * (kg & 1);
        half8 v;
        for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.f;
        if (s16 < ((m.layer[l].k_x + m.layer[l].k_e) >> 4)) v = w[(((size_t)s16 * 8 + t) * 2 + part) * 64 + lane_src];
        dst[((size_t)wave * G + g) * 256 + threadIdx.x] = v;
        return;
    }
    const int half = s & 1, s32 = s >> 1;
    const int n = 64 * wave + 16 * (2 * half + f) + (lane & 15);
    const int s16 = 2 * s32 + (kg >> 1), t = n >> 5, lane_src = (n & 31) + 32 * (kg & 1);
    half8 v;
    for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.f;          // k-steps past the layer's own K (padded copy): zeros
    if (s16 < ((m.layer[l].k_x + m.layer[l].k_e) >> 4)) v = w[(((size_t)s16 * 16 + t) * 2 + part) * 64 + lane_src];
    dst[((size_t)wave * G + g) * 256 + threadIdx.x] = v;
}

// third copy (nefii_mlp.reserved == 1 only): the single-pass evaluator's stream.  Unit g of a wave = one 32-deep k-step
// of the layer sequence with every layer's K padded to a multiple of 128, hi fragments of the wave's FT feature tiles:
// dst[((wave*G + g)*FT + f)*64 + lane][j] = hi(W[n = 16 FT wave + 16 f + (lane&15)][k = 32 s + 8 (lane>>4) + j]),
// zeros past the layer's own K.  blockDim.x = 64 FT.
__global__ void pack_sdf_stream_sp_kernel(nefii_mlp m, half8 *__restrict__ dst, int G, int ft) {
    const int g = blockIdx.x, wave = blockIdx.y;
    int l = 0, s = g;
    while (s >= s_units(m.layer[l])) s -= s_units(m.layer[l]), ++l;
    const half8 *w = reinterpret_cast<const half8 *>(m.layer[l].w_f16x3);
    const int f = threadIdx.x >> 6, lane = threadIdx.x & 63, kg = lane >> 4;
    const int n = 16 * ft * wave + 16 * f + (lane & 15);
    const int s16 = 2 * s + (kg >> 1), t = n >> 5, lane_src = (n & 31) + 32 * (kg & 1);
    const int NT = m.layer[l].n_pad >> 5;
    half8 v;
    for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.f;
    if (s16 < ((m.layer[l].k_x + m.layer[l].k_e) >> 4)) v = w[(((size_t)s16 * NT + t) * 2) * 64 + lane_src];
    dst[((size_t)wave * G + g) * ft * 64 + threadIdx.x] = v;
}

__global__ void pack_sdf_stream_bwd_kernel(nefii_mlp m, half8 *__restrict__ dst, int Gw, int g0, int ft) {
    const int g = blockIdx.x, wave = blockIdx.y;
    const int NH = m.n_layers - 1, U = vg_units_layer(m.layer[0].n_pad, ft);
    const int l = NH - 1 - g / U, s = g % U;
    const nefii_layer &L = m.layer[l];
    const half8 *wb = reinterpret_cast<const half8 *>(L.w_bwd_f16x3);
    const int KT = (L.k_x + L.k_e) >> 5;
    const int frag = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = frag >> 1, part = frag & 1, kg = lane >> 4;
    // kk: hidden input of layer l = output feature here
    const int half = s & 1, s32 = ft == 4 ? s >> 1 : s;
    const int kk = ft == 4 ? 64 * wave + 16 * (2 * half + f) + (lane & 15) : 32 * wave + 16 * f + (lane & 15);
    const int s16 = 2 * s32 + (kg >> 1), t = kk >> 5, lane_src = (kk & 31) + 32 * (kg & 1);
    dst[((size_t)wave * Gw + g0 + g) * 256 + threadIdx.x] = wb[(((size_t)s16 * KT + t) * 2 + part) * 64 + lane_src];
}

}  // namespace

// units per wave of the fifth copy (mlp_tile.h "16f": 8 per 128-deep chunk), 0 when the net does not take that evaluator
int stream_steps_f8(const nefii_mlp *m) {
    if (shape16p(m) != 4 || m->reserved != 1) return 0;
    int G = 0;
    for (int l = 0; l < m->n_layers - 1; ++l) G += 8 * f_chunks(m->layer[l]);
    return G;
}

extern "C" size_t nefii_sdf_stream_bytes(const nefii_mlp *h_sdf) {
    if (!h_sdf || h_sdf->n_layers < 2 || h_sdf->n_layers > NEFII_MAX_LAYERS || !shape16p(h_sdf)) return 0;
    return stream_bytes_1to4(h_sdf) + (size_t)8 * stream_steps_f8(h_sdf) * 4096;
}

extern "C" int nefii_sdf_fp8corr_supported(const nefii_mlp *h_sdf) {
    return h_sdf && h_sdf->w_stream && h_sdf->n_layers >= 2 && h_sdf->n_layers <= NEFII_MAX_LAYERS && stream_steps_f8(h_sdf) > 0;
}

// fifth copy.  Unit g of a wave: chunk c = (g - first unit of its layer) >> 3, j = & 7.  j < 4: the hi fragments of k-step 4 c + j
// (as the single-pass copy).  j >= 4: feature tile ft = j - 4, 16-byte element i of the lane: part = i >> 1 (0: w_l, 1: w_h),
// bytes 16 (i & 1) .. + 15 of the lane's 32: e4m3(W_part[n = 64 wave + 16 ft + (lane & 15)][k = 128 c + 32 (lane >> 4) + byte] x 2^E).
__global__ void pack_sdf_stream_f8_kernel(nefii_mlp m, half8 *__restrict__ dst, int G) {
    const int g = blockIdx.x, wave = blockIdx.y;
    int l = 0, u = g;
    while (u >= 8 * f_chunks(m.layer[l])) u -= 8 * f_chunks(m.layer[l]), ++l;
    const half8 *w = reinterpret_cast<const half8 *>(m.layer[l].w_f16x3);
    const int NT = m.layer[l].n_pad >> 5, K16 = (m.layer[l].k_x + m.layer[l].k_e) >> 4;
    const int c = u >> 3, j = u & 7;
    const int i = threadIdx.x >> 6, lane = threadIdx.x & 63, kg = lane >> 4;
    half8 v;
    for (int e = 0; e < 8; ++e) v[e] = (_Float16)0.f;
    if (j < 4) {
        const int s = 4 * c + j, n = 64 * wave + 16 * i + (lane & 15);
        const int s16 = 2 * s + (kg >> 1), t = n >> 5, lane_src = (n & 31) + 32 * (kg & 1);
        if (s16 < K16) v = w[(((size_t)s16 * NT + t) * 2) * 64 + lane_src];
    } else {
        const int ft = j - 4, part = i >> 1, n = 64 * wave + 16 * ft + (lane & 15), t = n >> 5;
        const int k0 = 128 * c + 32 * kg + 16 * (i & 1), s16 = k0 >> 4;
        const float sc = f8_scale(part == 0 ? F8_WL_E : F8_WH_E);
        int out[4] = {0, 0, 0, 0};
        if (s16 < K16) {
            const half8 a = w[(((size_t)s16 * NT + t) * 2 + (part == 0 ? 1 : 0)) * 64 + (n & 31)];            // k0 .. k0 + 7
            const half8 b = w[(((size_t)s16 * NT + t) * 2 + (part == 0 ? 1 : 0)) * 64 + (n & 31) + 32];       // k0 + 8 .. + 15
            out[0] = f8_pack4((float)a[0] * sc, (float)a[1] * sc, (float)a[2] * sc, (float)a[3] * sc);
            out[1] = f8_pack4((float)a[4] * sc, (float)a[5] * sc, (float)a[6] * sc, (float)a[7] * sc);
            out[2] = f8_pack4((float)b[0] * sc, (float)b[1] * sc, (float)b[2] * sc, (float)b[3] * sc);
            out[3] = f8_pack4((float)b[4] * sc, (float)b[5] * sc, (float)b[6] * sc, (float)b[7] * sc);
        }
        const i32x4 o4 = {out[0], out[1], out[2], out[3]};
        v = __builtin_bit_cast(half8, o4);
    }
    dst[((size_t)wave * G + g) * 256 + threadIdx.x] = v;
}

extern "C" int nefii_sdf_coarse_supported(const nefii_mlp *h_sdf) {
    return h_sdf && h_sdf->w_stream && h_sdf->n_layers >= 2 && h_sdf->n_layers <= NEFII_MAX_LAYERS &&
           stream_steps_sp(h_sdf) > 0;
}

extern "C" int nefii_pack_sdf_stream(const nefii_mlp *h_sdf, void *w_stream, void *stream) {
    if (!h_sdf || !w_stream) return NEFII_E_ARG;
    if (nefii_sdf_stream_bytes(h_sdf) == 0) return NEFII_E_UNSUPPORTED;
    for (int l = 0; l < h_sdf->n_layers - 1; ++l)
        if (!h_sdf->layer[l].w_f16x3) return NEFII_E_ARG;
    const int G = stream_steps(h_sdf);
    hipLaunchKernelGGL(pack_sdf_stream_kernel, dim3(G, 8), dim3(256), 0, (hipStream_t)stream, *h_sdf, (half8 *)w_stream, G,
                       shape16p(h_sdf), 0);
    HIP_CHECK_LAUNCH();
    const int G8 = stream_steps8(h_sdf);
    if (G8 > 0) {
        hipLaunchKernelGGL(pack_sdf_stream_kernel, dim3(G8, 8), dim3(256), 0, (hipStream_t)stream, *h_sdf,
                           (half8 *)w_stream + (size_t)8 * G * 256, G8, 4, 1);
        HIP_CHECK_LAUNCH();
    }
    const int Gs = stream_steps_sp(h_sdf);
    if (Gs > 0) {
        const int ft = shape16p(h_sdf);
        hipLaunchKernelGGL(pack_sdf_stream_sp_kernel, dim3(Gs, 8), dim3(64 * ft), 0, (hipStream_t)stream, *h_sdf,
                           (half8 *)w_stream + (size_t)8 * (G + G8) * 256, Gs, ft);
        HIP_CHECK_LAUNCH();
    }
    if (const int ft = vg_shape(h_sdf)) {
        const int Gb = vg_units_bwd(h_sdf), Gw = G + Gb;
        half8 *dst = (half8 *)w_stream + vg_stream_offset(h_sdf);
        hipLaunchKernelGGL(pack_sdf_stream_kernel, dim3(G, 8), dim3(256), 0, (hipStream_t)stream, *h_sdf, dst, Gw, ft, 0);
        HIP_CHECK_LAUNCH();
        hipLaunchKernelGGL(pack_sdf_stream_bwd_kernel, dim3(Gb, 8), dim3(256), 0, (hipStream_t)stream, *h_sdf, dst, Gw, G, ft);
        HIP_CHECK_LAUNCH();
    }
    if (const int Gf = stream_steps_f8(h_sdf)) {
        hipLaunchKernelGGL(pack_sdf_stream_f8_kernel, dim3(Gf, 8), dim3(256), 0, (hipStream_t)stream, *h_sdf,
                           reinterpret_cast<half8 *>((char *)w_stream + stream_bytes_1to4(h_sdf)), Gf);
        HIP_CHECK_LAUNCH();
    }
    return 0;
}

// ---- SDF interval grid (include/nefii_amd.h: nefii_sdf_bound_grid_build) ------------------------
namespace {
constexpr int GRID_SLAB = 8;       // vertex planes evaluated per launch of the point evaluator

// the vertices of planes i0 .. i0 + planes - 1 as a point list [planes (G+1)^2][3]: vertex (i, j, k) = -radius + (i, j, k) h
__global__ __launch_bounds__(256) void grid_points_kernel(int G, float radius, float h, int i0, int planes, float *__restrict__ x) {
    const int V = G + 1;
    const int64_t n = (int64_t)planes * V * V;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(q % V), j = (int)((q / V) % V), i = i0 + (int)(q / ((int64_t)V * V));
        x[q * 3] = fadd(-radius, fmul((float)i, h));
        x[q * 3 + 1] = fadd(-radius, fmul((float)j, h));
        x[q * 3 + 2] = fadd(-radius, fmul((float)k, h));
    }
}

// x -> the nearest fp16 on the far side of it: >= x (up) or <= x (down); finite |x| well inside the fp16 range
__device__ __forceinline__ unsigned short half_toward(float x, bool up) {
    const _Float16 hv = (_Float16)x;
    unsigned short bits = __builtin_bit_cast(unsigned short, hv);
    const bool wrong = up ? (float)hv < x : (float)hv > x;
    if (wrong) {
        const bool pos = !(bits & 0x8000u);
        if ((bits & 0x7FFFu) == 0)
            bits = up ? 0x0001u : 0x8001u;        // zero steps to the smallest subnormal
        else
            bits = (unsigned short)(pos == up ? bits + 1 : bits - 1);      // away from zero when the move and the sign agree
    }
    return bits;
}

// one thread per cell: min / max of its 8 corners, the largest slope over the grid edges of the 4^3 vertices around it
// (cell_l, where given: the cell's slope bound for grid_corner_bounds as fp16, rounded up)
__global__ __launch_bounds__(256) void grid_cells_kernel(int G, float h, float tau, float l_floor, float safety,
                                                         const float *__restrict__ g, unsigned *__restrict__ cells,
                                                         unsigned short *__restrict__ cell_l) {
    const int V = G + 1;
    const int64_t n = (int64_t)G * G * G;
    const float reach = (float)((double)h * 0.8660254037844386);       // h sqrt(3) / 2
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(c % G), j = (int)((c / G) % G), i = (int)(c / ((int64_t)G * G));
        auto at = [&](int a, int b, int d) { return g[((int64_t)a * V + b) * V + d]; };
        float lo = __builtin_inff(), hi = -__builtin_inff();
        // per axis: the largest and the least SIGNED slope over the block's edges along it
        float ux = -__builtin_inff(), uy = ux, uz = ux, dx = __builtin_inff(), dy = dx, dz = dx;
        auto edge = [&](float &u, float &d, float next, float here) {
            const float s = __fdiv_rn(fsub(next, here), h);
            u = fmaxf(u, s), d = fminf(d, s);
        };
        for (int a = i - 1; a <= i + 2; ++a)
            for (int b = j - 1; b <= j + 2; ++b)
                for (int d = k - 1; d <= k + 2; ++d) {
                    if (a < 0 || a > G || b < 0 || b > G || d < 0 || d > G) continue;
                    const float v = at(a, b, d);
                    if (a >= i && a <= i + 1 && b >= j && b <= j + 1 && d >= k && d <= k + 1) lo = fminf(lo, v), hi = fmaxf(hi, v);
                    // the edges that start here and stay inside the block
                    if (a < i + 2 && a < G) edge(ux, dx, at(a + 1, b, d), v);
                    if (b < j + 2 && b < G) edge(uy, dy, at(a, b + 1, d), v);
                    if (d < k + 2 && d < G) edge(uz, dz, at(a, b, d + 1), v);
                }
        const float sx = fmaxf(fabsf(ux), fabsf(dx)), sy = fmaxf(fabsf(uy), fabsf(dy)), sz = fmaxf(fabsf(uz), fabsf(dz));
        const float slope = fmaxf(fmaxf(sx, sy), sz);
        const float lcell = fmaxf(fmul(safety, slope), l_floor);
        const float slack = fadd(tau, fmul(lcell, reach));
        cells[c] = (unsigned)half_toward(fsub(lo, slack), false) | ((unsigned)half_toward(fadd(hi, slack), true) << 16);
        // the corner bounds lean on the slope itself, not on a slack with a corner spread beside it.  The differences along the
        // three axes measure the gradient's COMPONENTS, and its norm is up to sqrt(3) times the largest of them; and a
        // difference is the MEAN slope over its edge - how far the slope inside may lie above it is measured by how much
        // the means of the block's edges along that axis differ (largest - least): a feature little wider than a cell
        // shows there, and only there
        if (cell_l) {
            const float mx = fadd(sx, fsub(ux, dx)), my = fadd(sy, fsub(uy, dy)), mz = fadd(sz, fsub(uz, dz));
            const float norm = sqrtf(fadd(fadd(fmul(mx, mx), fmul(my, my)), fmul(mz, mz)));
            cell_l[c] = half_toward(fmaxf(fmul(safety, norm), l_floor), true);
        }
    }
}

// the vertex values as fp16, rounded to nearest (grid_corner_bounds adds what that can have moved them by)
__global__ __launch_bounds__(256) void grid_vertex_half_kernel(int64_t n, const float *__restrict__ g, unsigned short *__restrict__ out) {
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x)
        out[q] = __builtin_bit_cast(unsigned short, (_Float16)g[q]);
}

// one thread per block of NEFII_BOUND_GRID_BLOCK^3 cells: the least lo of its cells (fp16 bits ordered as the values are,
// -0 below +0; a NaN counts as -inf: no bound).  The last block of an axis is short where G is no multiple of the block.
__global__ __launch_bounds__(256) void grid_blocks_kernel(int G, int gb, const unsigned *__restrict__ cells,
                                                          unsigned short *__restrict__ blocks) {
    constexpr int B = NEFII_BOUND_GRID_BLOCK;
    const int64_t n = (int64_t)gb * gb * gb;
    auto key = [](unsigned bits) { return (bits & 0x8000u) ? (~bits & 0xFFFFu) : (bits | 0x8000u); };
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (int64_t)gridDim.x * blockDim.x) {
        const int k0 = (int)(q % gb) * B, j0 = (int)((q / gb) % gb) * B, i0 = (int)(q / ((int64_t)gb * gb)) * B;
        unsigned best = 0xFFFFu;
        for (int i = i0; i < i0 + B && i < G; ++i)
            for (int j = j0; j < j0 + B && j < G; ++j)
                for (int k = k0; k < k0 + B && k < G; ++k) {
                    unsigned bits = cells[((int64_t)i * G + j) * G + k] & 0xFFFFu;
                    if ((bits & 0x7FFFu) > 0x7C00u) bits = 0xFC00u;
                    const unsigned kk = key(bits);
                    best = kk < best ? kk : best;
                }
        blocks[q] = (unsigned short)((best & 0x8000u) ? (best & 0x7FFFu) : (~best & 0xFFFFu));
    }
}
}  // namespace

extern "C" int nefii_sdf_bound_grid_block_count(int G) {
    if (G < 2 || G > NEFII_BOUND_GRID_MAX) return 0;
    return (G + NEFII_BOUND_GRID_BLOCK - 1) / NEFII_BOUND_GRID_BLOCK;
}

extern "C" int nefii_sdf_bound_grid_blocks(const void *cells, int G, void *out_blocks, void *stream) {
    if (!cells || !out_blocks) return NEFII_E_ARG;
    const int gb = nefii_sdf_bound_grid_block_count(G);
    if (gb == 0) return NEFII_E_SHAPE;
    const int64_t n = (int64_t)gb * gb * gb;
    hipLaunchKernelGGL(grid_blocks_kernel, dim3((int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096)), dim3(256), 0,
                       (hipStream_t)stream, G, gb, (const unsigned *)cells, (unsigned short *)out_blocks);
    HIP_CHECK_LAUNCH();
    return 0;
}

extern "C" size_t nefii_sdf_bound_grid_workspace_bytes(int G) {
    if (G < 2 || G > NEFII_BOUND_GRID_MAX) return 0;
    const size_t V = (size_t)G + 1;
    return align256(sizeof(float) * V * V * V) + align256(sizeof(float) * 3 * GRID_SLAB * V * V);
}

extern "C" int nefii_sdf_bound_grid_build(const nefii_mlp *h_sdf, int G, float radius, float tau, float L_floor, float safety,
                                          void *out_cells, void *workspace, void *stream) {
    return nefii_sdf_bound_grid_build_vertices(h_sdf, G, radius, tau, L_floor, safety, out_cells, nullptr, nullptr, workspace, stream);
}

extern "C" int nefii_sdf_bound_grid_build_vertices(const nefii_mlp *h_sdf, int G, float radius, float tau, float L_floor,
                                                   float safety, void *out_cells, void *out_vertex_g, void *out_cell_l,
                                                   void *workspace, void *stream) {
    if (!h_sdf || !out_cells || !workspace || h_sdf->n_layers < 1 || h_sdf->n_layers > NEFII_MAX_LAYERS) return NEFII_E_ARG;
    if (!out_vertex_g != !out_cell_l) return NEFII_E_ARG;
    if (!(radius > 0.f && radius < 1e6f) || !(tau >= 0.f && tau < 1e6f) || !(L_floor > 0.f && L_floor < 1e6f) ||
        !(safety > 0.f && safety < 1e6f))
        return NEFII_E_ARG;
    if (G < 2 || G > NEFII_BOUND_GRID_MAX) return NEFII_E_SHAPE;
    if (!nefii_sdf_coarse_supported(h_sdf) || !sdf_net_ok(h_sdf)) return NEFII_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const int V = G + 1;
    const float h = (float)(2.0 * (double)radius / (double)G);
    float *g = (float *)workspace;
    float *x = (float *)((char *)workspace + align256(sizeof(float) * (size_t)V * V * V));
    for (int i0 = 0; i0 < V; i0 += GRID_SLAB) {
        const int planes = V - i0 < GRID_SLAB ? V - i0 : GRID_SLAB;
        const int64_t n = (int64_t)planes * V * V;
        hipLaunchKernelGGL(grid_points_kernel, dim3((int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024)), dim3(256), 0, st, G,
                           radius, h, i0, planes, x);
        HIP_CHECK_LAUNCH();
        const int rc = nefii_sdf_eval_coarse(h_sdf, x, n, g + (size_t)i0 * V * V, stream);
        if (rc) return rc;
    }
    const int64_t n_cells = (int64_t)G * G * G;
    hipLaunchKernelGGL(grid_cells_kernel, dim3((int)((n_cells + 255) / 256 < 4096 ? (n_cells + 255) / 256 : 4096)), dim3(256), 0,
                       st, G, h, tau, L_floor, safety, (const float *)g, (unsigned *)out_cells, (unsigned short *)out_cell_l);
    HIP_CHECK_LAUNCH();
    if (out_vertex_g) {
        const int64_t n_vert = (int64_t)V * V * V;
        hipLaunchKernelGGL(grid_vertex_half_kernel, dim3((int)((n_vert + 255) / 256 < 4096 ? (n_vert + 255) / 256 : 4096)), dim3(256),
                           0, st, n_vert, (const float *)g, (unsigned short *)out_vertex_g);
        HIP_CHECK_LAUNCH();
    }
    return 0;
}
