// sdf_launch.h - the little that nefii_tracer.hip (the SDF net's evaluators, along rays and at points) and nefii_sdf.hip (its
// fragment streams and the interval grid) share
#pragma once
#include "mlp_tile.h"

namespace nefii {

// defined in nefii_sdf.hip.  shape16p: feature tiles per wave (4 / 2) of a net the pipelined kernels take, else 0; fits16p: the
// same for a net that also has its fragment stream; sdf_net_ok: the nets the SDF evaluators take; stream_bytes_1to4: bytes of
// the first four copies of nefii_mlp.w_stream (the fifth - the "16f" evaluator's - follows them)
int shape16p(const nefii_mlp *m);
int fits16p(const nefii_mlp *m);
bool sdf_net_ok(const nefii_mlp *m);
size_t stream_bytes_1to4(const nefii_mlp *h_sdf);
// ... and the fourth copy, the value + gradient kernel's (sdf_value_grad16q_kernel): vg_shape - feature tiles per wave, 0 when the
// net does not take the kernel; stream_steps / vg_units_bwd - its forward / backward units per wave; vg_stream_offset - where
// it starts in w_stream, in half8
int vg_shape(const nefii_mlp *m);
int stream_steps(const nefii_mlp *m);
int vg_units_bwd(const nefii_mlp *m);
size_t vg_stream_offset(const nefii_mlp *m);

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// separate, correctly rounded operations: the arithmetic order of the reference, never contracted
__device__ __forceinline__ float fmul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float fadd(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float fsub(float a, float b) { return __fsub_rn(a, b); }

// backward units of one layer: 16-deep half steps (512-wide), whole 32-deep steps (256-wide)
__host__ __device__ __forceinline__ int vg_units_layer(int n_pad, int ft) { return ft == 4 ? n_pad >> 4 : n_pad >> 5; }

}  // namespace nefii
