/*
 * nefii_amd.h - C ABI of the MI355X (gfx950) hot-path library  libnefii_hip.so
 *
 * The reference (FuxiComputerVision/Nefii) has no FFI/plugin boundary: its hot path is eager
 * PyTorch.  This header is the boundary a maintainer would bind instead
 * (ctypes stub in INTEGRATION.md).  Each entry point names the reference code it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter is called h_* (host);
 *   - all tensors are contiguous float32 unless stated; masks are uint8 (0/1);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - nothing allocates, frees or synchronises: the caller owns every buffer including the
 *     workspaces, whose sizes come from the *_workspace_bytes() helpers (hipGraph-capturable);
 *   - return value: 0 = ok, negative = NEFII_E_* (bad argument), positive = hipError_t.
 */
#ifndef NEFII_AMD_H
#define NEFII_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NEFII_ABI_VERSION 19
#define NEFII_MAX_LAYERS 12
#define NEFII_TILE_ROWS 32          /* points per workgroup tile */
#define NEFII_MAX_WIDTH 512         /* widest hidden layer / feature vector */
#define NEFII_MAX_ENC 96            /* widest encoded-input block (padded) */
#define NEFII_MAX_LOBES 512         /* most light lobes (lgtSGs rows) any entry point accepts */

enum { NEFII_ACT_RELU = 0, NEFII_ACT_ELU = 1, NEFII_ACT_SOFTPLUS100 = 2 };
enum { NEFII_HEAD_NONE = 0, NEFII_HEAD_TANH01 = 1, NEFII_HEAD_POW2 = 2, NEFII_HEAD_SIGMOID = 3,
       NEFII_HEAD_RELU = 4, NEFII_HEAD_ABS = 5, NEFII_HEAD_RELU_INIT = 6 };
enum { NEFII_E_ARG = -1, NEFII_E_SHAPE = -2, NEFII_E_UNSUPPORTED = -3 };

/* One linear layer of a fused MLP.  Inputs of a layer are the concatenation
 *   [ hidden/feature block (k_x wide, lives in the LDS "X" buffer) | encoded-input block (k_e wide, LDS "E" buffer) ]
 * which covers the reference's three concat patterns:
 *   ImplicitNetwork skip layer   cat[x, PE(p)]/sqrt(2)         implicit_differentiable_renderer.py:97-98
 *   RenderingNetwork layer 0     cat[PE(p), PE(v), n, feat]    implicit_differentiable_renderer.py:205
 *   EnvmapMaterialNetwork lyr 0  cat[PE(p), feat]              sg_envmap_material.py:362-365
 * All widths are padded to multiples of 32 (pad weights are zero).  w_fwd / w_bwd are in the MFMA
 * fragment order produced by nefii_pack_linear(). */
typedef struct nefii_layer {
    int32_t k_x, k_e;        /* padded input widths (multiples of 32; either may be 0) */
    int32_t n_out;           /* true output width */
    int32_t n_pad;           /* padded output width (multiple of 32, <= 512) */
    const float *w_fwd;      /* packed [ (k_x+k_e)/8 ][ n_pad/32 ][64][4] */
    const float *w_bwd;      /* packed transpose for input gradients, or NULL */
    const float *bias;       /* [n_pad] */
    const void *w_f16x3;     /* optional: fp16 hi/lo split of w_fwd * 64 in 32x32x16 fragment order
                                [ (k_x+k_e)/16 ][ n_pad/32 ][ hi | lo ][64 lanes][8 halves]  (nefii_pack_linear_f16x3) */
    const void *w_bwd_f16x3; /* optional: the transposed fragments of the same split for input-gradient GEMMs
                                [ n_pad/16 ][ (k_x+k_e)/32 ][ hi | lo ][64 lanes][8 halves]  (nefii_pack_linear_f16x3_bwd) */
} nefii_layer;

typedef struct nefii_mlp {
    int32_t n_layers;
    int32_t act;             /* NEFII_ACT_* applied after every layer but the last */
    int32_t head;            /* NEFII_HEAD_* applied to the last layer's output */
    int32_t enc_freqs[3];    /* positional-encoding octaves of raw inputs a,b,c; -1 = input absent
                                (embedder.py:38-50: x, sin(2^k x), cos(2^k x), k < L) */
    int32_t feat_width;      /* per-point feature vector loaded into X before layer 0 (0 = none) */
    int32_t reserved;        /* layout of w_stream / matrix instruction of the pipelined evaluator: 0 = 32x32x16 fragments,
                                1 = 16x16x32 fragments (8 % faster per tile on MI355X; what nefii_amd.ops packs) */
    const void *w_stream;    /* optional (SDF nets, split precision): the hidden layers' w_f16x3 fragments re-packed as one
                                stream per wave for the pipelined tile evaluator (nefii_pack_sdf_stream), or NULL */
    nefii_layer layer[NEFII_MAX_LAYERS];
} nefii_mlp;

int nefii_abi_version(void);

/* Padded width of a hidden/output block of v columns: multiples of 32 up to 32, multiples of 64 beyond (every
 * 16-deep k-step count of the split-precision kernels is then a multiple of 4).  Encoded-input blocks pad to 32. */
int nefii_padded_width(int v);

/* Re-order one layer's effective weight W [n_out][k_in] (PyTorch nn.Linear layout, after weight-norm)
 * into MFMA fragment order, multiplying by `scale` (1/sqrt(2) for skip layers).
 * Input columns [x_src0, x_src0+x_len) feed the X block, [e_src0, e_src0+e_len) the E block
 * (X block and n_out padded with zeros to nefii_padded_width, E block to a multiple of 32).  Writes w_fwd ( (kx+ke)*n_pad floats ),
 * optionally w_bwd ( n_pad*(kx+ke) floats ) and bias_pad ( n_pad floats, from bias or zeros ). */
int nefii_pack_linear(const float *W, const float *bias, int n_out, int k_in,
                      int x_src0, int x_len, int e_src0, int e_len, float scale,
                      float *w_fwd, float *w_bwd, float *bias_pad, void *stream);

/* fp16 hi/lo split of the same weights for the 3-MFMA split-precision path (x*w ~ xh*wh + xh*wl + xl*wh, fp32
 * accumulate; the dropped xl*wl term is ~2^-22 relative).  Weights are pre-multiplied by 64 (exact) so that
 * the lo halves of typical |w| ~ 0.05 stay normal fp16 numbers; the kernel scales accumulators by 1/64. */
int nefii_pack_linear_f16x3(const float *W, int n_out, int k_in, int x_src0, int x_len, int e_src0, int e_len,
                            float scale, void *w_f16x3, void *stream);

/* The packings above (nefii_pack_linear, and - for the layers whose w_f16x3 / w_bwd_f16x3 pointers are set -
 * nefii_pack_linear_f16x3 / _f16x3_bwd) for EVERY layer of h_mlp in ONE launch: the radiance / material weights train
 * (idr_train.py:771-775 steps both optimizers every iteration), so they are re-packed every step.  h_layers: host array
 * [n_layers] of the sources; the destinations are the device pointers in h_mlp->layer[l] (bias always; w_fwd / w_bwd
 * unless skip_f32, which the fp16-MFMA kernels never read).  (ABI v7) */
typedef struct nefii_pack_source {
    const float *W;          /* [n_out][k_in], PyTorch nn.Linear layout, after weight-norm */
    const float *bias;       /* [n_out] or NULL */
    int32_t n_out, k_in, x_src0, x_len, e_src0, e_len;     /* as nefii_pack_linear */
    float scale;
    int32_t skip_f32;        /* 1: leave w_fwd / w_bwd alone */
} nefii_pack_source;
int nefii_pack_mlp(const nefii_mlp *h_mlp, const nefii_pack_source *h_layers, void *stream);

/* Fused MLP forward over n points (replaces ImplicitNetwork.forward :85-108, RenderingNetwork.forward
 * :196-241 and EnvmapMaterialNetwork's diffuse_albedo_layers sg_envmap_material.py:369).
 *   in_a/in_b/in_c : raw [n,3] inputs to be positional-encoded (NULL when enc_freqs[i] < 0)
 *   feat           : [n, feat_width] or NULL
 *   out            : [n, out_stride] receives the last layer's n_out columns (head applied)
 *   hidden_out     : optional [n, hid_stride]: activation entering the last layer (use_last_as_f feature)
 *   stash          : optional training stash [n_layers][n][stash_stride]: slot l < L-1 holds the
 *                    post-activation output of layer l (= input of layer l+1), slot L-1 the last layer's
 *                    pre-head output; consumed by nefii_mlp_backward and the weight-gradient GEMMs.
 *                    stash_stride >= widest n_pad. */
int nefii_mlp_forward(const nefii_mlp *h_mlp, const float *in_a, const float *in_b, const float *in_c,
                      const float *feat, int64_t n, float *out, int out_stride,
                      float *hidden_out, int hid_stride, float *stash, int stash_stride, void *stream);

/* Backward of nefii_mlp_forward wrt the hidden activations (the MLP inputs are not differentiated: geometry
 * is frozen in Step-2).  d_out [n, out_stride] is dL/d(head output).  Writes dz [n_layers][n][dz_stride]:
 * the gradient wrt every layer's pre-activation; parameter gradients follow with nefii_mlp_wgrad per layer. */
int nefii_mlp_backward(const nefii_mlp *h_mlp, const float *d_out, int out_stride, const float *stash,
                       int stash_stride, int64_t n, float *dz, int dz_stride, void *stream);

/* Parameter gradients of one layer from the buffers of nefii_mlp_forward (stash) / nefii_mlp_backward (dz):
 * dW [n_out][k_in] = scale * dz[:, :n_out]^T x[:, :k_in] (PyTorch nn.Linear layout), db [n_out] = column sums of dz
 * (db may be NULL).  x = nefii_encode_inputs output for layer 0, stash slot l-1 for layer l.  Overwrites dW / db. */
int nefii_mlp_wgrad(const float *dz, int dz_stride, const float *x, int x_stride, int64_t n, int n_out, int k_in,
                    float scale, float *dW, float *db, void *stream);

/* fp16-MFMA variants of the three entry points above for the radiance and material MLPs (the north star's "fused MLP
 * forward/backward with MFMA fp16 tiles"; every layer must carry w_f16x3 / w_bwd_f16x3); stash, dz, dW and db stay
 * fp32; not for the SDF network.
 *   forward: single_pass = 0 - split precision (fp16 hi/lo operand pairs, 3 MFMAs per k-step, fp32-class accuracy: the
 *     default, its outputs are held to the north-star tolerance); 1 - operands rounded to fp16 once (measured 1.3e-3
 *     relative L2 on rendered RGB on config 3 - above the 1e-3 bar, kept for measurement only);
 *   backward / wgrad: one fp16 pass, fp32 accumulation.  Gradients sit far below fp16's normal range, so the GEMMs
 *     carry dz x *scale, a power of two that nefii_mlp_grad_scale derives on the device from max |d_out|; `scale` is a
 *     device pointer to one float.  Parameter gradients come out within ~1e-3 (2e-2 through weight-norm's projection). */
int nefii_mlp_forward_f16(const nefii_mlp *h_mlp, const float *in_a, const float *in_b, const float *in_c,
                          const float *feat, int64_t n, float *out, int out_stride,
                          float *hidden_out, int hid_stride, float *stash, int stash_stride, int single_pass,
                          void *stream);
/* Both scale functions: up to 65 536 entries one launch; beyond that three on `stream` (clear, a many-block maximum that
 * accumulates in scale[0] itself, the final value).  scale stays ONE float that holds the scale once the stream gets there; no
 * workspace, nothing kept between calls, capturable into a graph. */
int nefii_mlp_grad_scale(const float *d_out, int64_t count, float *scale, void *stream);
/* The same scale with the head's derivative counted, for heads whose derivative is unbounded (NEFII_HEAD_POW2: 2 |pre|): derived
 * from max(|d_out|, |d_out head'(pre)| / 8) over the n x n_out entries, pre = the head's pre-activations [n][pre_stride] (slot
 * n_layers-1 of the fp32 stash, or z_last).  The head may amplify the seed gradient by up to 8 before the scale gives way, so a
 * net whose head derivative stays below 8 gets exactly nefii_mlp_grad_scale's value; beyond that scale[0] * dz of the last
 * layer stays below 2048 as for the other heads.  (Added without a struct change: NEFII_ABI_VERSION stays.) */
int nefii_mlp_grad_scale_head(const float *d_out, int out_stride, const float *pre, int pre_stride, int64_t n, int n_out,
                              int head, float *scale, void *stream);
int nefii_mlp_backward_f16(const nefii_mlp *h_mlp, const float *d_out, int out_stride, const float *stash,
                           int stash_stride, int64_t n, float *dz, int dz_stride, const float *scale, void *stream);
int nefii_mlp_wgrad_f16(const float *dz, int dz_stride, const float *x, int x_stride, int64_t n, int n_out, int k_in,
                        float scale, const float *gscale, float *dW, float *db, void *stream);

/* ABI 10 - the same three calls with the training state in HALVES, for nets nefii_mlp_h16_supported() accepts (streamed
 * forward and backward kernels: 512-wide hidden layers, no skip layer, a head of <= 8 outputs - the reference's material,
 * radiance and indirect-radiance networks, sg_envmap_material.py:131-176, implicit_differentiable_renderer.py:126-193).
 * What autograd keeps between RenderingNetwork.forward and its backward in the reference (fp32 activations per layer) is
 * here: stash16 = [n_layers - 1][n][stash_stride] halves holding 16 * h_l (the forward's own fp16 operand image),
 * z_last = [n][8] floats (pre-activations of the head), dz16 = [n_layers][n][dz_stride] halves holding scale[0] * dz_l.
 * nefii_mlp_wgrad_f16h consumes one layer's dz16 with x = its input: fp32 rows (x_half = 0: nefii_encode_inputs' matrix,
 * layer 0) or the stash16 slice of the layer below (x_half = 1).  Weight gradients are bit-identical to the fp32-stash
 * calls (the GEMM rounded its operands to these very halves); the backward's act'(h) is taken from the fp16 h.
 * x0_16 (optional) = [n][nefii_mlp_x0_width()] halves: 16 * layer 0's input as the kernel lays it out - its padded feature
 * columns, then the encodings of a, b, c, zero-padded - so that layer 0's weight gradient needs no nefii_encode_inputs
 * matrix: nefii_mlp_wgrad_f16h(dz16 of layer 0, x0_16, x_half = 1, k_in = that width) yields dW in THAT column order
 * (columns [0, x_len) = the Linear's feature columns, [k_x, k_x + e_len) = its encoding columns).
 * Strides count elements of the array's own type. */
int nefii_mlp_h16_supported(const nefii_mlp *h_mlp);
int nefii_mlp_x0_width(const nefii_mlp *h_mlp);
int nefii_mlp_forward_f16h(const nefii_mlp *h_mlp, const float *in_a, const float *in_b, const float *in_c,
                           const float *feat, int64_t n, float *out, int out_stride, float *hidden_out, int hid_stride,
                           void *stash16, int stash_stride, float *z_last, void *x0_16, void *stream);
int nefii_mlp_backward_f16h(const nefii_mlp *h_mlp, const float *d_out, int out_stride, const void *stash16,
                            int stash_stride, const float *z_last, int64_t n, void *dz16, int dz_stride,
                            const float *scale, void *stream);
int nefii_mlp_wgrad_f16h(const void *dz16, int dz_stride, const void *x, int x_stride, int x_half, int64_t n, int n_out,
                         int k_in, float scale, const float *gscale, float *dW, float *db, void *stream);

/* ABI 12 - nefii_mlp_wgrad_f16h for EVERY layer of a net in (at most) one zero-fill and one launch per kernel form: what
 * autograd does layer by layer behind RenderingNetwork.forward / diffuse_albedo_layers (one mm + one sum per nn.Linear).
 * Items are independent; results equal the per-layer calls (the same kernels' bodies on a flat grid). */
#define NEFII_MAX_WGRAD_ITEMS 12
typedef struct nefii_wgrad_item {
    const void *dz16;        /* [n][dz_stride] halves: scale[0] * dz of this layer (nefii_mlp_backward_f16h) */
    const void *x;           /* the layer's input rows: halves holding 16 h (x_half = 1) or floats (x_half = 0) */
    float *dW, *db;          /* [n_out][k_in]; [n_out] or NULL */
    int32_t dz_stride, x_stride, x_half, n_out, k_in;
    float scale;
} nefii_wgrad_item;
int nefii_mlp_wgrad_f16h_batch(const nefii_wgrad_item *h_items, int n_items, int64_t n, const float *gscale, void *stream);

/* The reference's layer-0 concatenation [PE(a) | PE(b) | PE(c) | feat] as a dense [n, width] matrix. */
int nefii_encode_inputs(const nefii_mlp *h_mlp, const float *in_a, const float *in_b, const float *in_c,
                        const float *feat, int64_t n, float *out, int width, void *stream);

/* SDF value, optional last-hidden feature, and d sdf / d x in one pass
 * (replaces implicit_network(points) + ImplicitNetwork.gradient, implicit_differentiable_renderer.py:110-123,
 * 533-540; the reference runs three SDF passes on the same points).  `ws`: nefii_sdf_value_grad_workspace_bytes(h_mlp, n)
 * bytes - n*(n_layers-1)*512 floats for the generic 32-row kernels; one slot per hidden layer and workgroup (at most
 * 256 workgroups; 128 KiB for 512-wide nets on 64-row tiles, 96 KiB for 256-wide nets on 96-row tiles) for softplus nets
 * of the streamed shapes (nefii_sdf_stream_bytes) with AT LEAST TWO hidden layers, one encoder whose columns pad to 64
 * (3 + 6 L columns with L = 5 ... 10) and no feature block, a fragment stream in the 16x16x32 layout (w_stream, reserved == 1)
 * and transposed fragments on every layer: they run forward AND backward on the stream (the tracer's split-precision
 * evaluator followed by the same k-loop over the transposed layers; the last layer may have any number of columns up to
 * 512).  A net with ONE hidden layer, or with fewer than 33 encoding columns, takes the generic kernels here even when
 * nefii_sdf_eval and the tracer run it on the stream. */
int nefii_sdf_value_grad(const nefii_mlp *h_mlp, const float *x, int64_t n, float *sdf_out, int out_stride,
                         float *feat_out, int feat_stride, float *grad_out, float *ws, void *stream);
size_t nefii_sdf_value_grad_workspace_bytes(const nefii_mlp *h_mlp, int64_t n);

/* RayTracing.forward (ray_tracing.py:29-101) for rays with per-ray origins: bounding-sphere intersection
 * (rend_util.py:200-221), both-ends sphere tracing with back-off (:104-193), 100-sample bracket search +
 * bisection for rays that did not converge (:195-280) and, when `training`, the min-SDF search for rays
 * that miss (:309-337).  Bisection stops per ray (documented difference, <=1e-6 in t).
 *
 * Directions must be UNIT vectors: the sphere intersection (b^2 - (|o|^2 - r^2), no division by |d|^2), the clamp of both
 * depths to 0.01 and every Lipschitz argument of the staged searches take depths as distances.  Nothing checks it.
 *
 * What a trace call accepts (anything else is refused before anything is enqueued - NEFII_E_SHAPE for a range, NEFII_E_ARG
 * for a switch):
 *   object_bounding_sphere, sdf_threshold, line_search_step   any value (the reference's: 1.0, 5e-5, 0.5)
 *   n_steps                >= 2^bisect_levels (8 with the default 3 levels); the coarse pass and the staged searches run for
 *                          16 <= n_steps <= 128 only (7-bit sample ids) and are silently off outside that range
 *   sphere_tracing_iters   0 .. 250 (0: the fronts stay on the bounding sphere, every ray with a positive end goes to the
 *                          bracket search)
 *   line_step_iters        0 .. 15 (the back-off factor is (1 - line_search_step) / 2^k)
 *   n_rootfind_steps       0 .. 250 (0: a bracketed ray takes the middle of its bracket)
 *   bisect_levels          0 .. 5;  precision 0 .. 2 (1 and 2 with w_f16x3 on every layer);  coarse_tau 0 .. 1;
 *   minsdf_lipschitz 0 .. 1e6;  tier_kappa, tier_gate >= 0;  trace_tier, unread_misses, split_fp8 0 or 1
 *   training != 0 needs minsdf_steps;  the workspace at least nefii_trace_workspace_bytes();  1 <= n_rays < 2^29
 *   (nefii_trace_rays* with n_rays == 0 is a no-op) */
typedef struct nefii_tracer_params {
    float object_bounding_sphere, sdf_threshold, line_search_step;
    int32_t line_step_iters, sphere_tracing_iters, n_steps, n_rootfind_steps;
    int32_t training;
    int32_t bisect_levels;   /* bisection steps resolved per round by evaluating the next levels of the bisection tree
                                speculatively (2^levels - 1 queries per ray per round, bit-identical result):
                                1..5, 0 = default 3.  5 suits small latency-bound batches, 3 large ones. */
    int32_t precision;       /* SDF evaluation inside the tracer: 0 = f32-input MFMA (exact fp32),
                                1 = 3x fp16 split MFMA, 32-query tiles; 2 = the same arithmetic on 64-query tiles
                                (8 waves, weight fragments shared by two row tiles); 1 and 2 need w_f16x3 */
    float coarse_tau;        /* > 0 (precision 2, pipelined shapes, 16x16x32 stream layout): the n_steps samples of the
                                bracket search (:203-219) and of the min-SDF search (:316-331) are first evaluated in ONE
                                fp16 pass (a third of the matrix work); coarse_tau bounds |coarse - split| of a sample.
                                Only samples whose coarse value cannot decide - within coarse_tau of zero where the
                                first sign change is looked for, within 2 coarse_tau of the minimum where the argmin
                                is - are re-evaluated in split precision, so every decision (and the outputs) is the
                                split evaluator's PROVIDED the bound holds for every sample taken: it is the CALLER'S
                                claim about this net, measured (nefii_sdf_eval_coarse against nefii_sdf_eval, with a
                                safety factor), not proven - a sample whose true difference exceeded it could decide
                                differently.  0 = off. */
    int32_t coarse_cap;      /* most samples of one ray re-evaluated individually; a ray with more takes all n_steps
                                in split precision instead.  <= 0: 64.  At most 100. */
    int32_t minsdf_group;    /* > 0: minsdf_steps holds one row of n_steps uniform draws per minsdf_group consecutive rays
                                (several batches - each with the draw the reference makes per call, ray_tracing.py:316 -
                                traced as ONE call); 0: one row for all rays */
    int32_t small_round;     /* rounds of at most this many split-precision queries run on 32-query tiles (more CUs, shorter
                                round; 1.5x the chip time per query); 0: 8192.  Traces that overlap other work pass a
                                smaller value. */
    int32_t trace_tier;      /* ABI 12 - tiered sphere tracing (needs coarse_tau > 0; ignored without it).  1: a sphere-tracing
                                evaluation (ray_tracing.py:128-134,164-168,182-183) whose front is still far from the surface
                                - the step that led to the query exceeds tier_gate * coarse_tau; the first evaluation on the
                                bounding sphere always - runs on the single-pass evaluator, and its value v16 is TAKEN AS THE
                                VALUE when |v16| > max(tier_kappa * coarse_tau, coarse_tau + 2 sdf_threshold): both decisions
                                the recurrence makes with it (v <= sdf_threshold :140-148, v < 0 :170-171,186-187) are then
                                the split evaluator's, but the front advances by v16 instead of v.  Inside that band the
                                query is repeated in split precision first.  UNLIKE the coarse pass of the two dense searches
                                this changes values, not only schedules: fronts differ by up to coarse_tau per step on the
                                way and end where the exact value is <= sdf_threshold as before (depths within ~sdf_threshold
                                / cos of the split-precision trace; measured: DESIGN.md, "tiered sphere tracing").  0: off. */
    float tier_kappa;        /* <= 0: 2 */
    float tier_gate;         /* <= 0: 4 */
    float minsdf_lipschitz;  /* ABI 13 - staged min-SDF search (needs coarse_tau > 0, 16 <= n_steps <= 128; ignored otherwise).
                                > 0: the caller's bound L on |sdf(p) - sdf(q)| / |p - q| along a ray inside the bounding sphere
                                (rays have unit directions).  The search (ray_tracing.py:309-337: argmin over n_steps depths)
                                then evaluates ceil(n_steps / 4) of the depths - evenly spread over their SORTED order, both
                                ends included - in the single-pass evaluator first; a depth s between evaluated neighbours
                                a < s < b whose lower bound  max(v_a - L (t_s - t_a), v_b - L (t_b - t_s)) - coarse_tau  exceeds
                                (lowest value seen) + coarse_tau cannot be the argmin and is NEVER evaluated; the others go to
                                the single-pass evaluator one by one, and the refinement in split precision proceeds as
                                before over the depths that were evaluated.  The argmin (first index of the exact minimum) is
                                the full search's PROVIDED L holds: like coarse_tau a measured claim about this net (largest
                                |grad sdf| seen on a sample of the ball, with a safety factor), not a proof.  Audited online:
                                every depth of the second stage - plus, per search, ONE of the skipped depths picked by a
                                hash and evaluated after all - is checked against the lower bound it was given,
                                counters[r][NEFII_CNT_LIP_AUDIT].  The BRACKET search (:195-257) is staged the same way for eval-mode traces and
                                for rays outside the object mask: a quarter row of its n_steps samples spread over the row
                                first; a sample whose lower bound proves it positive - and, unless the ray lies inside the
                                mask and surely has a negative sample in front of which only signs matter, above the lowest
                                value seen + coarse_tau - is never evaluated; the first negative sample, the bracket and the
                                argmin fallback are the full row's.  0: off (all n_steps depths / samples are evaluated). */
    int32_t unread_misses;   /* ABI 14 - 1: the caller reads nothing of the rays that end WITHOUT a hit (out_points / out_dists of
                                such rays are then unspecified, out_hit is exact).  Honoured for eval-mode traces (training == 0):
                                the bracket search's argmin fallback (:221-231: a ray without a negative sample takes the depth
                                of its lowest sample) is not computed - no refinement of the samples near the minimum, and the
                                staged search skips every sample its bound proves positive.  Hit masks, hit points and hit
                                depths are those of unread_misses == 0 bit for bit.  What the Monte-Carlo renderer's secondary
                                rays need (path_tracing_render.py: visibility and the radiance at secondary HITS). */
    int32_t split_fp8;       /* ABI 15 - 1: the split-precision evaluations of the trace (every query the coarse pass and the tier do
                                not take) run on the "16f" evaluator: the main product x_h w_h on fp16 MFMAs as before, the two
                                correction products x_h w_l and x_l w_h on the block-scaled fp8 MFMA
                                (v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 operands, constant scales).  A THIRD arithmetic: max |sdf
                                error| against fp64 ~1e-5 (1.6e-6 near the surface) where the fp16 split gives 5e-7 - values, not
                                only schedules, change at that level (depths of converged rays within ~1e-5; DESIGN.md section
                                4g).  Needs precision 2 and a 512-wide net with the fifth stream copy
                                (nefii_sdf_fp8corr_supported); ignored otherwise.  0: off (default). */
} nefii_tracer_params;
#define NEFII_TRACE_COUNTERS 14  /* int32 counters per round: the columns below (see nefii_trace_rays) */
/* Columns of counters[round][NEFII_TRACE_COUNTERS].  "adds": a count, summed over rays (and addable over chunks and traces);
 * "max": the bits of a float >= 0, the largest value seen (such bit patterns order like the floats; combine with max).
 * A column marked (W) counts entries of one of the round's work lists: while any of them is non-zero in the last round that
 * ran, a ray still waits for an evaluation and the trace is not finished. */
#define NEFII_CNT_SINGLES 0          /* adds (W): sphere-tracing queries in split precision */
#define NEFII_CNT_DENSE_ROWS 1       /* adds (W): rays with all n_steps samples of a dense search in split precision */
#define NEFII_CNT_BISECT_RAYS 2      /* adds (W): rays in bisection (2^levels - 1 speculative queries each) */
#define NEFII_CNT_BISECT_USED 3      /* adds: bisection evaluations actually consumed */
#define NEFII_CNT_REFINED 4          /* adds (W): coarse-pass samples re-evaluated one by one in split precision */
#define NEFII_CNT_COARSE_WINDOWS 5   /* adds (W): QUARTER rows (ceil(n_steps / 4) samples of one ray) in the single-pass (coarse) evaluator (ABI 11; whole rows before) */
#define NEFII_CNT_SEARCHES 6         /* adds: rays entering a dense search (the reference evaluates n_steps samples for each) */
#define NEFII_CNT_BISECT_EVALS 7     /* adds: (2^levels - 1) * BISECT_RAYS, the speculative bisection evaluations executed */
#define NEFII_CNT_TAU_AUDIT 8        /* max: |coarse - split| among the samples this round re-evaluated in split precision - the online
                                        audit of coarse_tau (every refined sample is evaluated both ways anyway); a value above
                                        coarse_tau means the caller's bound does not hold for this net */
#define NEFII_CNT_COARSE_SINGLES 9   /* adds (W): (ABI 12, trace_tier) sphere-tracing queries in the single-pass evaluator */
#define NEFII_CNT_REPEATS 10         /* adds: queries of SINGLES that repeat a COARSE_SINGLES one in split precision (they take part in TAU_AUDIT) */
#define NEFII_CNT_COARSE_SAMPLES 11  /* adds (W): (ABI 13, minsdf_lipschitz) samples of staged searches evaluated one by one in the single-pass
                                        evaluator (the first stage's samples are a quarter row of COARSE_WINDOWS) */
#define NEFII_CNT_LIP_AUDIT 12       /* max: the amount by which such a sample's value fell below the lower bound that minsdf_lipschitz
                                        gave it; above 0 the bound does not hold for this net */
#define NEFII_CNT_PROBES 13          /* adds: (ABI 15) samples the staged searches had SKIPPED and evaluated after all as probes of that audit: one
                                        per search picked by a hash of (ray, position), plus up to 6 whose bound cleared the limit by
                                        less than 2 coarse_tau (they are among COARSE_SAMPLES) */

/* The pipelined evaluator behind nefii_trace_rays (precision 2) and nefii_sdf_eval reads the hidden layers' fragments as
 * ONE stream per wave, 4 KiB per 16-deep unit of the layer sequence: [8 waves][units][4 fragments][64 lanes][8 halves];
 * the fragments are 32x32x16 ones (hi/lo of the wave's two column tiles) or, with nefii_mlp.reserved == 1, 16x16x32 ones
 * (hi/lo of two of the wave's four 16-feature tiles, alternating between the halves of a 32-deep k-step).
 * With reserved == 1 a third copy follows for the single-pass (coarse) evaluator: hi fragments only, one 32-deep k-step
 * of the wave's feature tiles per unit, K zero-padded to multiples of 128.
 * When every layer also carries transposed fragments (w_bwd_f16x3) and the last layer has one column, a fourth copy
 * follows for nefii_sdf_value_grad: per wave the forward units again, then for l = n_layers-2 .. 1 the 16-deep units of
 * the transposed layer (the wave's 64 hidden inputs as output features) - one cursor runs forward and backward.
 * nefii_sdf_stream_bytes: size of that buffer, 0 if the net's shape does not qualify (at least one hidden layer; every
 * hidden layer W wide, W = 512, or 256 with reserved == 1; every layer's k_x in {0,W} and k_e in {0,64}, so a skip layer may sit
 * anywhere among the hidden layers; a W-deep last layer WITHOUT encoding columns, so a skip into the output layer does not
 * qualify) - such nets run on the generic kernel and leave w_stream NULL.
 * nefii_pack_sdf_stream: device-side copy from the layers' w_f16x3 (call after nefii_pack_linear_f16x3). */
size_t nefii_sdf_stream_bytes(const nefii_mlp *h_sdf);
int nefii_pack_sdf_stream(const nefii_mlp *h_sdf, void *w_stream, void *stream);

/* The same idea for the radiance / material MLPs (RenderingNetwork.forward, implicit_differentiable_renderer.py:196-241;
 * EnvmapMaterialNetwork's MLPs, sg_envmap_material.py:357-425) on the split-precision forward nefii_mlp_forward_f16: nets
 * with at least one hidden layer whose hidden layers are all 512 wide (layer 0: 0 ... 512 feature columns, padded as
 * nefii_padded_width pads them, + 0 ... 96 padded encoding columns, NEFII_MAX_ENC - any of the three encoders or none; no
 * skip layer; last layer: at most 8 outputs, 9 and more run on the generic kernels) keep their hidden layers' hi/lo
 * fragments as one stream per wave, [8 waves][units][4 fragments][64
 * lanes][8 halves], a unit = 16-deep half step of a layer whose K is rounded up to a multiple of 64 with zero weights.
 * With w_stream set the forward runs 48- / 64-row tiles on the tracer's pipelined evaluator structure.
 * nefii_mlp_stream_bytes: size of the buffer, 0 when the shape does not qualify; nefii_pack_mlp_stream: device-side
 * gather from the layers' w_f16x3 - call after every nefii_pack_linear_f16x3 (the weights train). */
size_t nefii_mlp_stream_bytes(const nefii_mlp *h_mlp);
int nefii_pack_mlp_stream(const nefii_mlp *h_mlp, void *w_stream, void *stream);

/* Transposed counterpart for the split-precision input-gradient GEMMs (nefii_sdf_value_grad picks its split-precision
 * kernel when every layer carries both w_f16x3 and w_bwd_f16x3). */
int nefii_pack_linear_f16x3_bwd(const float *W, int n_out, int k_in, int x_src0, int x_len, int e_src0, int e_len,
                                float scale, void *w_bwd_f16x3, void *stream);

/* sdf_out[i] = implicit_network(x[i])[:, 0] (implicit_differentiable_renderer.py:85-108) with the tracer's
 * split-precision tile evaluator (the arithmetic of precision 2): the bulk SDF query the reference issues from
 * ray_tracing.py:128-131,211-216,322-327 and pixel_pair_generator.py:52, as a stand-alone call.  x [n][3], needs
 * w_f16x3 in every layer (and uses w_stream when set); bias arrays hold n_pad floats, 16-byte aligned. */
int nefii_sdf_eval(const nefii_mlp *h_sdf, const float *x, int64_t n, float *sdf_out, void *stream);
/* The same points through the tracer's single-pass (coarse) evaluator; NEFII_E_UNSUPPORTED when the net has no
 * single-pass stream (nefii_sdf_coarse_supported).  max |nefii_sdf_eval_coarse - nefii_sdf_eval| over points of the
 * bounding sphere, with a safety factor, is what a caller passes as nefii_tracer_params.coarse_tau. */
int nefii_sdf_eval_coarse(const nefii_mlp *h_sdf, const float *x, int64_t n, float *sdf_out, void *stream);
int nefii_sdf_coarse_supported(const nefii_mlp *h_sdf);
/* ABI 15 - the same points through the "16f" evaluator (nefii_tracer_params.split_fp8: correction products on block-scaled fp8);
 * NEFII_E_UNSUPPORTED unless nefii_sdf_fp8corr_supported (512-wide hidden layers, reserved == 1, w_stream packed by this
 * library version: the fifth copy of nefii_pack_sdf_stream - per wave and 128-deep chunk of each layer's 128-padded K eight 4-KiB
 * units: four 32-deep k-steps of hi fragments, then per 16-feature tile [e4m3(w_l 2^10) 32 B | e4m3(w_h 2^-1) 32 B] per lane). */
int nefii_sdf_eval_fp8corr(const nefii_mlp *h_sdf, const float *x, int64_t n, float *sdf_out, void *stream);
int nefii_sdf_fp8corr_supported(const nefii_mlp *h_sdf);

size_t nefii_trace_workspace_bytes(int64_t n_rays, const nefii_tracer_params *h_params);
int nefii_trace_max_rounds(const nefii_tracer_params *h_params);
/* lin_steps: the n_steps values of torch.linspace(0,1,n_steps); minsdf_steps: the n_steps uniforms of
 * minimal_sdf_points (only read when training).  counters (optional, int32 [max_rounds][NEFII_TRACE_COUNTERS])
 * receives per round the columns NEFII_CNT_* above.  With n_steps = nefii_tracer_params.n_steps:
 * algorithmic evaluations (what the reference's recurrences need) = SINGLES + COARSE_SINGLES - REPEATS + n_steps*SEARCHES +
 * BISECT_USED; executed in split precision = SINGLES + n_steps*DENSE_ROWS + BISECT_EVALS + REFINED; executed in the coarse
 * evaluator = ceil(n_steps / 4)*COARSE_WINDOWS + COARSE_SINGLES + COARSE_SAMPLES. */
int nefii_trace_rays(const nefii_mlp *h_sdf, const nefii_tracer_params *h_params,
                     const float *origins, const float *dirs, const uint8_t *object_mask, int64_t n_rays,
                     const float *lin_steps, const float *minsdf_steps,
                     float *out_points, uint8_t *out_hit, float *out_dists,
                     void *workspace, size_t workspace_bytes, int32_t *counters, void *stream);

/* SDF interval grid under frozen geometry: what nefii_trace_rays_rounds / _groups read through a nefii_trace_grid.
 * The cube [-radius, radius]^3 is cut into G^3 cells of edge h = 2 radius / G.
 * nefii_sdf_bound_grid_build evaluates the single-pass SDF (nefii_sdf_eval_coarse's evaluator) at the (G+1)^3 vertices
 * -radius + (i, j, k) h and writes per cell (i, j, k), at out_cells[(i G + j) G + k], one 32-bit word: fp16 lo in the low half,
 * fp16 hi in the high half,
 *   lo = min_c g_c - tau - L_cell h sqrt(3)/2 (rounded down),   hi = max_c g_c + tau + L_cell h sqrt(3)/2 (rounded up),
 *   L_cell = max(L_floor, safety x the largest |g_a - g_b| / h over the grid edges (a, b) of the 3x3x3 block of cells around it)
 * (c: the cell's 8 corners; tau: the caller's bound on |single-pass - exact|).  lo <= sdf <= hi then holds over the cell as far
 * as L_cell bounds the slope inside it - a measured bound, audited by the tracer wherever it evaluates a sample
 * (NEFII_CNT_LIP_AUDIT).  workspace: nefii_sdf_bound_grid_workspace_bytes(G) bytes of device memory.  Everything is
 * enqueued on `stream`.  Refused before anything is enqueued: a NULL pointer, radius / tau / L_floor / safety not finite or
 * radius, L_floor, safety <= 0 or tau < 0 (NEFII_E_ARG); G outside 2 .. NEFII_BOUND_GRID_MAX (NEFII_E_SHAPE); a net without
 * the single-pass stream (NEFII_E_UNSUPPORTED).
 * nefii_sdf_bound_grid_build_vertices is nefii_sdf_bound_grid_build - the same evaluator, slabs, workspace and out_cells, bit for
 * bit - and additionally writes the values behind the grid (both or neither; NULL, NULL: exactly that call)
 *   out_vertex_g [(G+1)^3] fp16: g at vertex (i, j, k), at [(i (G+1) + j) (G+1) + k], rounded to nearest (so the stored value is
 *                within e = 2^-11 |stored| + 2^-25 of g);
 *   out_cell_l   [G^3] fp16: the slope bound L_c of cell (i, j, k), at [(i G + j) G + k], rounded up:
 *                L_c = max(L_floor, safety x sqrt(mx^2 + my^2 + mz^2)), m_a = s_a + (u_a - d_a), with u_a / d_a the largest / least
 *                signed (g_b - g_a) / h over the edges along axis a of the same block and s_a = max(|u_a|, |d_a|) - the differences
 *                along the axes measure the gradient's components, whose norm is up to sqrt(3) times the largest, and each is
 *                a mean over its edge, which the slope inside may exceed by as much as neighbouring means differ; L_c >= L_cell.
 * A point p of cell c is then bounded from c's 8 corners x_k, with d_k = |p - x_k| + 1e-6:
 *   lo(p) = max_k (g_k - e_k - L_c d_k) - tau,   hi(p) = min_k (g_k + e_k + L_c d_k) + tau
 * - the same measured quantities and the same slope claim over the cell as the cell's interval, without the spread over the
 * corners and with the actual reach instead of the largest one.
 * nefii_sdf_bound_grid_blocks: the block level over a grid - out_blocks fp16 [Gb][Gb][Gb], Gb = nefii_sdf_bound_grid_block_count(G)
 * = ceil(G / NEFII_BOUND_GRID_BLOCK), the least `lo` of the cells of each block of NEFII_BOUND_GRID_BLOCK^3 cells (a minimum of
 * fp16 values: exact, nothing to round; the last block of an axis is short where G is no multiple).  0 for G outside
 * 2 .. NEFII_BOUND_GRID_MAX (count) / NEFII_E_SHAPE (build). */
#define NEFII_BOUND_GRID_MAX 640
#define NEFII_BOUND_GRID_BLOCK 4
#define NEFII_CERTIFY_MARGIN 1e-4f
#define NEFII_CERTIFY_COUNTS 4        /* [0] rays certified as crossed, [1] their block look-ups; [2] rays ended as free, [3] their look-ups */
size_t nefii_sdf_bound_grid_workspace_bytes(int G);
int nefii_sdf_bound_grid_build(const nefii_mlp *h_sdf, int G, float radius, float tau, float L_floor, float safety,
                               void *out_cells, void *workspace, void *stream);
int nefii_sdf_bound_grid_build_vertices(const nefii_mlp *h_sdf, int G, float radius, float tau, float L_floor, float safety,
                                        void *out_cells, void *out_vertex_g, void *out_cell_l, void *workspace, void *stream);
int nefii_sdf_bound_grid_block_count(int G);
int nefii_sdf_bound_grid_blocks(const void *cells, int G, void *out_blocks, void *stream);

/* ABI 19 - the grid a trace reads (radius = object_bounding_sphere), in one descriptor.  A NULL descriptor, or cells == NULL, is a trace without a grid.  In
 * every mode the trace gives the same points, hit mask and depths - of every ray whose outputs are read - wherever the
 * intervals hold; a net without the staged searches (minsdf_lipschitz > 0 and the single-pass stream) traces as if no grid
 * had been given. */
typedef struct nefii_trace_grid {
    /* int32 [G,G,G] of nefii_sdf_bound_grid_build.  The staged bracket searches of an EVAL-MODE trace read their first stage from
     * it - one look-up per sample - instead of evaluating a quarter row.  Samples the intervals do not decide count under
     * NEFII_CNT_COARSE_SAMPLES, probes under NEFII_CNT_PROBES. */
    const void *cells;
    /* fp16 [(G+1)^3] and [G^3] of nefii_sdf_bound_grid_build_vertices, both or neither (one without the other, or both without
     * cells: NEFII_E_ARG).  A bracket search then bounds the samples its cell intervals leave undecided from their corners - max
     * of the lower ends, min of the upper ends - and decides again: the survivors are a subset of the cell intervals' (probes
     * apart), and the audit holds every evaluated sample against the combined interval. */
    const void *vertex_g, *cell_l;
    /* fp16 [Gb,Gb,Gb] of nefii_sdf_bound_grid_blocks over the same cells; read, and needed, when certify != 0 */
    const void *blocks;
    /* device int32 [NEFII_CERTIFY_COUNTS], ADDED to (the caller zeroes it); may be NULL */
    int32_t *certify_counts;
    /* cells per axis; with cells, outside 1 .. NEFII_BOUND_GRID_MAX: NEFII_E_SHAPE */
    int32_t G;
    /* 0: only eval-mode traces read the grid.  1: a TRAINING-MODE trace reads it as well - the bracket searches of its rays INSIDE
     * the object mask start from the grid (cell intervals, corner bounds, probes and audit as in eval mode, with the argmin
     * limit max(0, U + tau) unless the front decides, since training mode reads the argmin of a ray without a negative
     * sample) in place of the quarter-row windows; rays outside the mask keep their evaluated first stage, the min-SDF
     * searches theirs.  Anything else: NEFII_E_ARG. */
    int32_t training;
    /* bits; rays the grid decides are ended before they are traced ("certificates").  Outside 0 .. 3, or set
     * without cells and blocks: NEFII_E_ARG.  With off = coarse_tau + NEFII_CERTIFY_MARGIN:
     *   bit 0, training-mode traces, the CROSSING certificate: bounds a_k <= t_s, b_k >= t_e on the two fronts, a_0 = t0, b_0 = t1.
     *     Per step a walk over every block j the chord [a_k, b_k] crosses, which the chord is in from depth in_j to out_j;
     *     s_j = lo_j - off must exceed sdf_threshold in every one of them, then a_k+1 = min_j (max(a_k, in_j) + s_j),
     *     b_k+1 = max_j (min(b_k, out_j) - s_j).  A ray with a_k >= b_k for some k <= sphere_tracing_iters goes to its min-SDF
     *     search in round 0 with no sphere-tracing query; every sample that search evaluates is held against its cell's interval
     *     into NEFII_CNT_LIP_AUDIT.
     *   bit 1, eval-mode traces with unread_misses, the FREE-STRETCH certificate: at every sphere-tracing iteration, before its
     *     queries go out, a ray whose stretch [t_s, t_max] (to where it leaves the bounding sphere) lies in cells with
     *     lo - off > sdf_threshold throughout - walked by blocks, a block that is not free by its cells - ends as a miss: hit 0,
     *     finite point and depth.  One such ray in 16 (a hash) first sends one depth of the stretch to the single-pass evaluator
     *     (NEFII_CNT_PROBES) and holds the value against its cell into NEFII_CNT_LIP_AUDIT.
     * Both rest on the grid's intervals and on the network being above sdf_threshold wherever a step that overshoots the other
     * front can land outside the bounding sphere (a crossing step is evaluated before the fronts are compared).  Eval-mode
     * traces whose misses are read are not changed. */
    int32_t certify;
    int32_t reserved;
} nefii_trace_grid;

/* nefii_trace_rays restricted to rounds [round_begin, round_end) (round_end <= 0: up to nefii_trace_max_rounds), with a grid.  Rounds
 * after the last one that emitted a query are empty launches; a caller that synchronises anyway can run a prefix,
 * read the work-list columns of counters[round_end-1] - the seven marked (W) at NEFII_CNT_*: SINGLES, DENSE_ROWS, BISECT_RAYS,
 * REFINED, COARSE_WINDOWS, COARSE_SINGLES, COARSE_SAMPLES - and continue with round_begin = round_end only if any of them is non-zero
 * (ray state and counters persist in `workspace` between the calls; outputs are complete once none is pending). */
int nefii_trace_rays_rounds(const nefii_mlp *h_sdf, const nefii_tracer_params *h_params,
                            const float *origins, const float *dirs, const uint8_t *object_mask, int64_t n_rays,
                            const float *lin_steps, const float *minsdf_steps,
                            float *out_points, uint8_t *out_hit, float *out_dists,
                            void *workspace, size_t workspace_bytes, int32_t *counters,
                            int round_begin, int round_end, const nefii_trace_grid *grid, void *stream);
/* The same for n_groups contiguous chunks of the ray batch (rays [group_begin[g], group_begin[g+1]) ), each with its own
 * workspace and hipStream_t, enqueued round-major so that all chunks advance together.  Rays are independent: results
 * are those of one nefii_trace_rays_rounds call over the whole batch.  What it buys: the latency-bound rounds of a small
 * batch (fewer 64-query tiles than CUs - one tile time per round, however few the queries) of different chunks overlap
 * on the chip.  counters: [n_groups][max_rounds][NEFII_TRACE_COUNTERS].  The caller orders the streams against its own (events). */
int nefii_trace_rays_groups(const nefii_mlp *h_sdf, const nefii_tracer_params *h_params,
                            const float *origins, const float *dirs, const uint8_t *object_mask,
                            int n_groups, const int64_t *group_begin,
                            const float *lin_steps, const float *minsdf_steps,
                            float *out_points, uint8_t *out_hit, float *out_dists,
                            void *const *workspaces, const size_t *workspace_bytes, int32_t *counters,
                            int round_begin, int round_end, const nefii_trace_grid *grid, void *const *streams);

/* Measurement hooks (bench.py): when enabled, nefii_trace_rays brackets every SDF-evaluation launch with HIP
 * events on the launch stream; nefii_trace_profile_read returns the summed launch durations (ms), the number
 * of launches and the span of the last trace call, and clears the record.  Off by default. */
int nefii_trace_profile_enable(int on);
int nefii_trace_profile_read(double *h_eval_ms, int *h_n_eval, double *h_span_ms);
/* per-launch durations (ms) in launch order into h_ms[cap]; returns the count (does not clear the record) */
int nefii_trace_profile_launches(float *h_ms, int cap);

/* rend_util.get_camera_params + lift (rend_util.py:90-142): uv [B,S,2], pose [B,4,4], intrinsics [B,4,4]
 * -> unit ray dirs [B,S,3] and per-ray origins [B,S,3] (camera centre broadcast). */
int nefii_camera_rays(const float *uv, const float *pose, const float *intrinsics, int batch, int64_t samples,
                      float *out_dirs, float *out_origins, void *stream);

/* Every entry point that takes a light lgtSGs [n_lobes,7] needs 1 <= n_lobes <= NEFII_MAX_LOBES (512) and returns
 * NEFII_E_SHAPE otherwise. */

/* render_with_sg (sg_render.py:164-295) for one base material (K=1) with global roughness [1] and
 * specular [3]: outputs rgb / specular / diffuse [n,3].  1 <= n_lobes <= 512. */
int nefii_sg_render_forward(const float *lgtSGs, int n_lobes, const float *specular, const float *roughness,
                            const float *albedo, const float *normal, const float *view, int64_t n,
                            float *rgb, float *spec_rgb, float *diff_rgb, void *stream);
/* Gradients of sum(d_rgb*rgb + d_spec*spec_rgb + d_diff*diff_rgb) wrt albedo [n,3], roughness [1], specular [3]
 * and lgtSGs [n_lobes,7] (the last three accumulated atomically into zero-initialised buffers).  1 <= n_lobes <= 512. */
int nefii_sg_render_backward(const float *lgtSGs, int n_lobes, const float *specular, const float *roughness,
                             const float *albedo, const float *normal, const float *view, int64_t n,
                             const float *d_rgb, const float *d_spec, const float *d_diff,
                             float *g_albedo, float *g_roughness, float *g_specular, float *g_lgtSGs, void *stream);

/* IDRNetwork.get_background_rgb (implicit_differentiable_renderer.py:646-663): sum of light SGs along dirs.
 * 1 <= n_lobes <= 512. */
int nefii_env_radiance_forward(const float *lgtSGs, int n_lobes, const float *dirs, int64_t n, float eps,
                               float *rgb, void *stream);
int nefii_env_radiance_backward(const float *lgtSGs, int n_lobes, const float *dirs, int64_t n, float eps,
                                const float *d_rgb, float *g_lgtSGs, void *stream);

/* ABI 16 - fitting light SGs to an environment map (envmaps/fit_envmap_with_sg.py), fused and deterministic:
 * rgb(d) = sum_m |mu_m| exp(|lambda_m| (d . v_m / (|v_m| + eps) - 1)), loss = mean over n*3 of (rgb - target)^2, for
 * dirs / target [n,3] and 1 <= n_lobes <= 512.  workspace: nefii_envfit_workspace_bytes(n, n_lobes) bytes of device memory
 * (one slab of n_lobes*7 + 1 partial sums per 256 directions; 0 for a bad shape).  No atomics: results are bitwise
 * identical from run to run.
 * loss_grad: loss [1], g_lgtSGs [n_lobes,7] (overwritten; abs has gradient 0 at 0, as in torch) and, when rgb is not
 * NULL, the fitted map rgb [n,3].
 * adam: `iters` iterations of the fit with torch.optim.Adam's update applied in place to lgtSGs / exp_avg / exp_avg_sq
 * (updates step0 + 1 ... step0 + iters), enqueued without a host synchronisation; losses [iters], losses[i] the loss
 * BEFORE update step0 + i + 1.  lr / betas / adam_eps are doubles, as torch holds them (the kernels see them rounded
 * to fp32 in the places torch's foreach kernels do). */
int64_t nefii_envfit_workspace_bytes(int64_t n, int n_lobes);
int nefii_envfit_loss_grad(const float *lgtSGs, int n_lobes, const float *dirs, const float *target, int64_t n, float eps,
                           void *workspace, float *loss, float *g_lgtSGs, float *rgb, void *stream);
int nefii_envfit_adam(float *lgtSGs, float *exp_avg, float *exp_avg_sq, int n_lobes, const float *dirs,
                      const float *target, int64_t n, float eps, double lr, double beta1, double beta2,
                      double adam_eps, int64_t step0, int iters, void *workspace, float *losses, void *stream);

/* ABI 17 - marching cubes over a dense fp32 volume vol[nx][ny][nz] (C order, z fastest), as utils/plots.py meshes the SDF
 * (skimage marching_cubes_lewiner), with welded vertices and a fixed output order.  Inside: v < level.  Each crossing grid
 * edge gets one vertex, owned by the edge's lower grid point and numbered by (owner's linear index, axis x < y < z), at
 * origin + (p0 + t (p1 - p0)) * spacing per axis, t = (level - v0) / (v1 - v0), index space before the affine map.
 * Triangles [F,3] int32 come by cell linear index, then in the order of the table (nefii_amd/csrc/mc_tables.h; ambiguous
 * faces are cut alike from both cells, so meshes have no cracks), wound so that face normals point towards increasing
 * values (outward for an SDF).  No atomics decide any order: two runs are bitwise equal.
 * Shapes: nx, ny, nz >= 2 and nx*ny*nz < 2^31 (NEFII_E_SHAPE otherwise); level, origin and spacing finite (NEFII_E_ARG).
 * workspace: nefii_mcubes_workspace_bytes(nx, ny, nz) bytes of device memory (0 for a bad shape) - one int32 vertex base
 * per grid point, then one int2 count pair and one int64 offset pair per tile of 2048 grid points, each part aligned to
 * 256 bytes.  It carries the count call's results to the emit call.
 * count: enqueues pass 1 and the scan; counts [2] int64 (device) <- (n_verts, n_tris).
 * emit: with the SAME vol, shape, level and workspace, after count, enqueues passes 2 and 3: verts [n_verts,3] float32,
 * faces [n_tris,3] int32.  max_verts / max_tris are the rows the caller's buffers hold: nothing is written beyond them.
 * Face indices are int32, so n_verts must be below 2^31.  No host synchronisation in either call. */
int64_t nefii_mcubes_workspace_bytes(int nx, int ny, int nz);
int nefii_mcubes_count(const float *vol, int nx, int ny, int nz, float level, void *workspace, int64_t *counts,
                       void *stream);
int nefii_mcubes_emit(const float *vol, int nx, int ny, int nz, float level, float origin_x, float origin_y,
                      float origin_z, float spacing_x, float spacing_y, float spacing_z, void *workspace, float *verts,
                      int64_t max_verts, int *faces, int64_t max_tris, void *stream);

/* Sparse mesh export from the SDF interval grid (DESIGN.md 6f "Sparse export"; added without a struct change: NEFII_ABI_VERSION
 * stays).  The fine grid of nx x ny x nz points (2 .. 4096 per axis) is cut into bricks of B cells per edge, 2 <= B <= 8:
 *   cell bricks  [cbx][cby][cbz], cb = ceil((n - 1) / B): brick I holds the cells anchored at grid points I B .. I B + B - 1,
 *                clipped to the grid; fewer than 2^31 of them;
 *   point bricks [pbx][pby][pbz], pb = (n - 1) / B + 1: brick I owns the grid points I B .. I B + B - 1, clipped; each grid
 *                point has one owner (pb = cb + 1 where the grid's last plane starts a brick of its own).
 * Linear indices of grid points are int64: the grid may hold more than 2^31 points.
 *
 * nefii_mcubes_classify_bricks: out_active [cbx][cby][cbz] uint8, 1 where the brick may hold a crossing of `level`.  cells,
 * G, radius: the words of nefii_sdf_bound_grid_build.  frame [12] doubles ON THE HOST: the world position of grid point
 * (0, 0, 0), then the world steps of one index along x, y and z; grid point (i, j, k) lies at ((p0 + i sx) + j sy) + k sz.
 * Rule: the brick's 8 corner points (clipped to the grid) in fp64, each rounded once to fp32; their axis-aligned box, widened
 * outwards by one fp32 ulp of its largest |coordinate|; the interval cells the box overlaps are those of
 * (int)((x + radius) * (float)(G / (2 radius))) at its two ends per axis; lo_b = the least lo, hi_b = the greatest hi among
 * them, compared in fp32: inactive only if lo_b > level or hi_b < level.  (The ulp covers the corners' rounding; a caller whose
 * grid points are rounded otherwise than this frame - fp32 linspace values lie up to half an ulp of the grid's LARGEST coordinate
 * off it - can have a point that far outside the box: far inside the intervals' slack, and to be audited against its own cell.)  A box that leaves [-radius, radius]^3 anywhere and
 * any non-finite word make the brick active.  A thread serves a brick while no brick can overlap more than 64 cells, a wave
 * beyond that; the bytes are the same.
 *
 * nefii_mcubes_sparse_count / _emit: marching cubes over the listed cell bricks with the conventions of ABI 17 - inside v <
 * level, one vertex per crossing edge owned by its lower grid point, t = (level - v0) / (v1 - v0), the same fp32 position
 * expression, table and winding.  vals [n_slots][B^3] float32: the values of the evaluated point bricks, point (lx, ly, lz) of
 * a brick at (lx B + ly) B + lz; slot_map [pbx][pby][pbz] int32: a point brick's slot, or -1.  The caller evaluates every point
 * brick an active cell brick touches (the active set dilated by +1 brick along each axis).  active_list [n_active] int32:
 * linear indices of cell bricks, each at most once; one workgroup per entry gathers the brick's (B+1)^3 corners into LDS.
 * count: counts [n_active][2] int32 <- (crossing edges among the brick's cells, triangles).
 * emit, with offsets [n_active][2] int64 = the exclusive prefix sums of counts: per crossing edge vert_keys <- owner's linear
 * index * 3 + axis and vert_pos [.,3]; per triangle face_cell <- the cell's linear index and face_keys [.,3] <- its vertices'
 * keys, a cell's triangles in table order.  An edge on a face that two listed bricks share is written by both, bit-equal.
 * Sorting vert_keys (dropping repeats), sorting faces stably by face_cell and looking the keys up gives the dense mesh's
 * verts and faces in its order.  Nothing is written beyond max_verts / max_tris rows.  No atomics; no host synchronisation. */
int nefii_mcubes_classify_bricks(const void *cells, int G, float radius, int nx, int ny, int nz, const double *frame,
                                 float level, int B, uint8_t *out_active, void *stream);
int nefii_mcubes_sparse_count(const float *vals, const int *slot_map, int n_slots, int nx, int ny, int nz, int B,
                              const int *active_list, int n_active, float level, int *counts, void *stream);
int nefii_mcubes_sparse_emit(const float *vals, const int *slot_map, int n_slots, int nx, int ny, int nz, int B,
                             const int *active_list, int n_active, float level, float origin_x, float origin_y,
                             float origin_z, float spacing_x, float spacing_y, float spacing_z, const int64_t *offsets,
                             int64_t *vert_keys, float *vert_pos, int64_t max_verts, int64_t *face_cell, int64_t *face_keys,
                             int64_t max_tris, void *stream);

/* The three importance-sampled directions per surface point and their 3x3 pdf table for multiple importance
 * sampling (cos_sampling :128, brdf_sampling :61, mix_sg_sampling :168 and the pdf_fn_* of
 * path_tracing_render.py; table as :1312-1325).  uniforms [n,7] = (cos r1 r2 | ggx r1 r2 | mix r0 r1 r2) in the
 * reference's draw order; roughness [n].  Outputs: wi [3,n,3], own_pdf [3,n] (clamped at 1e-6),
 * pdf_table [3,n,3] (row = direction, column = pdf of strategy j for that direction).  1 <= n_lobes <= 512. */
int nefii_mis_sample(const float *lgtSGs, int n_lobes, const float *roughness, const float *normal, const float *view,
                     const float *uniforms, int64_t n, float *wi, float *own_pdf, float *pdf_table, void *stream);

/* ABI 18 - a lat-long HDR environment map as the Monte-Carlo renderer's light (constant_2d_light_sampling and
 * pdf_fn_constant_2d_light, code/model/path_tracing_render.py:291-380; the envmap renderer :1496 on).  DESIGN.md 6g.
 * map [H,W,3] float32; texel (i,j) covers v in [i/H,(i+1)/H), u in [j/W,(j+1)/W), phi = pi v; coord 0 (mitsuba, y up):
 * d = (cos t sin phi, cos phi, sin t sin phi), t = 2 pi u - pi/2; coord 1 (blender, z up): d = (cos t sin phi,
 * sin t sin phi, cos phi), t = pi - 2 pi u.  Radiance is the nearest texel.  Distribution f(i,j) = max(mean rgb, 0) *
 * sin(pi (i + 0.5) / H), summed in fp64, stored as fp32 CDFs ending in exactly 1.0f (uniform for a zero row / an all-zero
 * map); pdf(d) = P(i,j) H W / (2 pi^2 sin phi), P from the stored CDF differences, 0 where sin phi = 0.
 * table: nefii_envlight_table_bytes(H, W) bytes of device memory (0 for a bad shape); nefii_envlight_build fills it from
 * the map (two launches, no atomics: two builds are bitwise equal).  Shapes: H, W >= 1 and H*W < 2^31 (NEFII_E_SHAPE).
 * mis_sample: nefii_mis_sample's outputs and conventions with the SG-mixture technique replaced by the map - rows 0 and 1
 * are that function's, bitwise; row 2 samples the map by continuous inversion (uniforms column 4: row, 5: column; 6 is
 * unused); column 2 of pdf_table is the map's pdf.  light [3,n,3]: the map's radiance along each of the 3 directions (row
 * 2: the texel it was drawn from), ready for nefii_mc_shade_forward.  radiance: rgb [n,3] along dirs [n,3]; pdf: [n]. */
int64_t nefii_envlight_table_bytes(int height, int width);
int nefii_envlight_build(const float *map, int height, int width, void *table, void *stream);
int nefii_envlight_mis_sample(const float *map, const void *table, int height, int width, int coord,
                              const float *roughness, const float *normal, const float *view, const float *uniforms,
                              int64_t n, float *wi, float *own_pdf, float *pdf_table, float *light, void *stream);
int nefii_envlight_radiance(const float *map, int height, int width, int coord, const float *dirs, int64_t n,
                            float *rgb, void *stream);
int nefii_envlight_pdf(const void *table, int height, int width, int coord, const float *dirs, int64_t n, float *pdf,
                       void *stream);

/* One recomputed bounce under the map light (added without a struct change: NEFII_ABI_VERSION stays).  For
 * each of m secondary hits - specular [3] global, roughness [m], albedo / normal / view [m,3], uniforms [m,3] =
 * (u0, u1, u2) - ONE direction wo [m,3] by one-sample MIS with the balance heuristic over the three techniques of
 * nefii_envlight_mis_sample: k = min((int)(3 u0), 2) picks cosine (k = 0, (u1, u2)), GGX (k = 1, (u1, u2)) or the map
 * (k = 2, u1: row, u2: column); wo is the direction row k of that function returns for the same normal, view and
 * roughness.  mix = (pdf_cos + pdf_ggx + pdf_map) / 3 along wo (pdf_map: the texel that was drawn for k = 2, the texel
 * under wo otherwise); mix >= 1e-6 / (3 pi).  weight [m,3] = max(fs cos L / mix, 0) + max(albedo / pi cos L / mix, 0): the
 * hit's outgoing radiance estimate along view for unit visibility, with nefii_mc_shade_forward's BRDF (GGX D, Schlick
 * 2^(-(5.55473 vh + 6.8316) vh), Smith-Schlick G, its clamps), cos = max(wo.n, 0) and L the map's texel along wo (the
 * texel drawn for k = 2).  mix_pdf [m] <- mix, or NULL.  No atomics: two calls are bitwise equal.  Argument checks as
 * nefii_envlight_mis_sample (m <= 0 returns 0 before anything is read). */
int nefii_envlight_bounce_sample(const float *map, const void *table, int height, int width, int coord,
                                 const float *specular, const float *roughness, const float *albedo,
                                 const float *normal, const float *view, const float *uniforms, int64_t m, float *wo,
                                 float *weight, float *mix_pdf, void *stream);

/* The map light under a rotation (no struct change: NEFII_ABI_VERSION stays).  rot [A,3,3] fp32 on the
 * device: R, world-from-light, row-major (rotate_light_sgs' convention).  L_R(d) = L(R^T d), a sampled direction is
 * R direction_of(u, v), p_R(d) = p(R^T d): the table of the unrotated map serves every R.  rot_identity [A] int32 on the
 * device, set by the host from the nine floats: nonzero where rotation a is exactly the identity; the kernels then skip
 * the products (1 x + 0 y + 0 z turns -0 into +0) and reproduce the unrotated entry points bit for bit.  A >= 1
 * (NEFII_E_ARG); mis_sample_rot also needs A <= 65535 (NEFII_E_SHAPE).  Other checks as the unrotated entry points.
 * mis_sample_rot: one launch for all A rotations; wi [A,3,n,3], own_pdf [A,3,n], pdf_table [A,3,n,3], light [A,3,n,3];
 * slice a is what a call with rotation a alone returns; rows 0-1 of wi and own_pdf and columns 0-1 of their pdf_table do
 * not depend on a.  bounce_sample_rot / radiance_rot / pdf_rot: rot_index [m] (or [n]) int32 on the device picks each
 * item's rotation, NULL means rotation 0 for all; an index outside [0, A) is the caller's error and is not checked here. */
int nefii_envlight_mis_sample_rot(const float *map, const void *table, int height, int width, int coord,
                                  const float *rot, const int *rot_identity, int A, const float *roughness,
                                  const float *normal, const float *view, const float *uniforms, int64_t n, float *wi,
                                  float *own_pdf, float *pdf_table, float *light, void *stream);
int nefii_envlight_bounce_sample_rot(const float *map, const void *table, int height, int width, int coord,
                                     const float *rot, const int *rot_identity, int A, const int *rot_index,
                                     const float *specular, const float *roughness, const float *albedo,
                                     const float *normal, const float *view, const float *uniforms, int64_t m,
                                     float *wo, float *weight, float *mix_pdf, void *stream);
int nefii_envlight_radiance_rot(const float *map, int height, int width, int coord, const float *rot,
                                const int *rot_identity, int A, const int *rot_index, const float *dirs, int64_t n,
                                float *rgb, void *stream);
int nefii_envlight_pdf_rot(const void *table, int height, int width, int coord, const float *rot,
                           const int *rot_identity, int A, const int *rot_index, const float *dirs, int64_t n,
                           float *pdf, void *stream);

/* One level of the feature-guided a-trous wavelet filter that denoises a Monte-Carlo frame (Dammertz et al.
 * 2010); the weights are written out in nefii_amd/csrc/nefii_denoise.hip, section 1.  The frame is height x width, row-major;
 * every array holds float4 elements, 16-byte aligned: guides0 [H*W] = (normal.xyz, valid), guides1 [H*W] = (world
 * position.xyz, 0), in / out [n_signals][H*W] = (r, g, b, carried through).  A valid pixel p (guides0.w > 0.5) becomes the
 * normalised sum of its 5 x 5 taps q = p + step (i, j) that are inside the image, valid and finite, weighted by a B3 spline, a
 * normal term (sigma_n), a tangent-plane term (sigma_x) and, per signal, a relative-luminance term (sigma_c_level).  A tap is
 * not finite where r, g or b of any signal is NaN or inf; the fourth lane is neither looked at nor altered.  Equal
 * luminances and a centre that is not finite give the luminance term 1.  A pixel whose weights sum to 0 and an invalid pixel
 * keep their input, the latter bitwise.  The caller runs the levels l = 0 .. L-1 with step 2^l and sigma_c_level = sigma_c
 * 2^-l between two buffers; the guides are never filtered.  One launch, no workspace, no atomics: bitwise reproducible.
 * Refused without touching the device: a NULL pointer, in == out, step < 1, a negative or NaN sigma, an infinite sigma_n
 * (NEFII_E_ARG; sigma_c_level = inf is legal and switches the colour term off), n_signals outside 1 .. 2 (NEFII_E_ARG),
 * height or width outside 1 .. 16384 (NEFII_E_SHAPE). */
int nefii_denoise_atrous(const void *guides0, const void *guides1, const void *in, void *out, int n_signals, int height,
                         int width, int step, float sigma_n, float sigma_x, float sigma_c_level, void *stream);

/* Per-pixel variance from the rays, and the a-trous level it guides (added without a struct change:
 * NEFII_ABI_VERSION stays).  NEFII_ALBEDO_FLOOR is the denoiser's floor under the albedo it demodulates with, an fp32 number;
 * nefii_amd/denoise.py and tests/denoise_var_ref.py mirror it.
 * nefii_pixel_moments: diffuse, albedo, specular [n_pixels * rays, 3] fp32 and hit [n_pixels * rays] bytes, row p rays + r is
 * ray r of pixel p; signals [2][n_pixels] float4, 16-byte aligned - the `in` layout of the filter.  For a pixel whose rays all
 * hit, with a = max(mean_r albedo_r, NEFII_ALBEDO_FLOOR) per channel: signals[0][p] = (mean_r diffuse_r / a, v), signals[1][p] =
 * (mean_r specular_r, v), v = sum_r (e_r - ebar)^2 / (rays (rays - 1)) the variance of the mean of the Rec. 709 luminance e_r
 * of diffuse_r / a and of specular_r.  fp64 sums in two passes, one rounding to fp32, no contraction; equal samples give v = 0
 * exactly; a NaN or inf sample leaves the lanes it enters non-finite; a pixel with a ray that missed is four zeros in both
 * signals.  16 lanes per pixel, a summation order fixed by `rays` alone, no atomics: the same bits from run to run.  Refused
 * before anything is enqueued: a NULL pointer, misaligned signals (NEFII_E_ARG); rays outside 2 .. 4096, n_pixels < 1
 * (NEFII_E_SHAPE).
 * nefii_denoise_atrous_variance: nefii_denoise_atrous on in / out = (r, g, b, v), v read as max(v, 0), with the four
 * differences of nefii_amd/csrc/nefii_denoise.hip, section 2: a tap is not finite where any of the FOUR lanes of any signal is
 * NaN or inf; the luminance term is scaled by sigma_l times the square root of v's 3 x 3 average around p, and is 1 for equal
 * luminances, for a centre that is not finite or has no valid finite pixel in that average, and for sigma_l = inf; out.v is
 * the variance the weights leave.  A pixel whose weights sum to 0 keeps all four lanes of its input, and so does, bitwise, an
 * invalid p.  sigma_l is not scaled by the level.  Refusals as nefii_denoise_atrous. */
#define NEFII_ALBEDO_FLOOR 1e-3f
int nefii_pixel_moments(const float *diffuse, const float *albedo, const float *specular, const unsigned char *hit,
                        int64_t n_pixels, int rays, float *signals, void *stream);
int nefii_denoise_atrous_variance(const void *guides0, const void *guides1, const void *in, void *out, int n_signals,
                                  int height, int width, int step, float sigma_n, float sigma_x, float sigma_l, void *stream);

/* Adaptive sampling of Monte-Carlo frames (added without a struct change: NEFII_ABI_VERSION stays).  A frame
 * is rendered in rounds of `rays` rays per pixel; a pilot round over all pixels estimates each pixel's noise, the rest of a
 * ray budget goes to the pixels that need it, the rounds are merged.  Every sum is fp64 and nothing is contracted; no float
 * atomics; nothing depends on the launch geometry: the same bits from run to run and for any split into calls.  Every entry
 * point refuses, before anything is enqueued, a NULL pointer (merge's pixel aside), a pointer that is not aligned to its
 * element (out of the moments: 8 bytes) (NEFII_E_ARG) and n_pixels outside 1 .. 2^31 - 1 (NEFII_E_SHAPE).
 * nefii_ray_luminance_moments: rgb [n_pixels * rays, 3], row p rays + r is ray r of pixel p; out [n_pixels][2] = (ebar, M2),
 *   ebar = Y(mean_r rgb_r) with the Rec. 709 luminance Y, M2 = sum_r (Y(rgb_r) - ebar)^2.  Two passes in fp64, one rounding to
 *   fp32; rays = 1 and equal samples give M2 = 0 exactly; a NaN or inf sample leaves both lanes non-finite.  16 lanes per
 *   pixel, a summation order fixed by `rays` alone.  rays outside 1 .. 4096: NEFII_E_SHAPE.
 * nefii_adaptive_merge: rows [m][columns + 2] are one round's outputs of m pixels: `columns` means over the round's `rays`
 *   rays, then that round's (ebar, M2).  Row i belongs to pixel pixel[i], each pixel listed at most once; pixel = NULL means
 *   i, and then m == n_pixels.  sum [n_pixels][columns] and stat [n_pixels][3] = (n, mean, M2) are fp64 and start at zero:
 *     sum[p][c] += rays * rows[i][c]                                   (the product is exact)
 *     delta = ebar - mean;  n' = n + rays;  mean' = mean + (delta * rays) / n';
 *     M2' = (M2 + M2_b) + (delta * delta) * ((n * rays) / n')
 *   in exactly this order of operations; with n = 0 the result is (rays, ebar, M2_b) exactly.  An index outside
 *   [0, n_pixels) writes nothing.  columns outside 1 .. 64, rays outside 1 .. 4096, m outside 1 .. n_pixels: NEFII_E_SHAPE.
 * nefii_adaptive_score: stat of a height x width frame -> score [height * width] fp32, s = sqrt(M2 / (n - 1)) / (|mean| + eps)
 *   in fp64, rounded once; n < 2 or a rounded s that is not finite gives 0.  dilate = 1: the maximum of s over the 3 x 3 pixels
 *   around p that lie in the image; 0: s itself.  eps not in (0, inf), dilate not 0 or 1: NEFII_E_ARG; height or width outside
 *   1 .. 16384: NEFII_E_SHAPE.
 * nefii_adaptive_count: adds T(lambda) = sum_p k_p to *total, which the caller zeroes, k_p = min(max_rounds, max(1,
 *   ceil(fl32(lambda * score_p)))), evaluated as x > 1 ? (x >= max_rounds ? max_rounds : ceil(x)) : 1 so that a NaN product
 *   gives 1.  64-bit integer partial sums, one integer atomic per workgroup.  fp32 multiplication is monotone, so T is: the
 *   allocation of a budget of N rounds is the largest finite lambda >= 0 with T(lambda) <= N, found by bisection on the bit
 *   pattern of lambda (nefii_amd/ops/image.py: adaptive_allocate).  nefii_adaptive_targets: k [n_pixels] int32, the same k_p.
 *   Both: lambda negative, NaN or inf: NEFII_E_ARG; max_rounds outside 1 .. 65536: NEFII_E_SHAPE.
 * nefii_adaptive_finalise: out [n_pixels][columns] = fl32(sum / n), but for a column c with bit c of mask_columns set 1 where
 *   sum == n (the column was 1 for every ray of every round) else 0; rays [n_pixels] int32 = n; variance [n_pixels] = M2 /
 *   (n (n - 1)), the variance of the mean luminance, 0 for n < 2.  A pixel that was never merged (n = 0) gets NaN colours.
 *   columns outside 1 .. 64: NEFII_E_SHAPE; a bit of mask_columns at or above `columns`: NEFII_E_ARG. */
int nefii_ray_luminance_moments(const float *rgb, int64_t n_pixels, int rays, float *out, void *stream);
int nefii_adaptive_merge(const float *rows, const int32_t *pixel, int64_t m, int64_t n_pixels, int columns, int rays,
                         double *sum, double *stat, void *stream);
int nefii_adaptive_score(const double *stat, int height, int width, double eps, int dilate, float *score, void *stream);
int nefii_adaptive_count(const float *score, int64_t n_pixels, float lambda, int max_rounds, uint64_t *total, void *stream);
int nefii_adaptive_targets(const float *score, int64_t n_pixels, float lambda, int max_rounds, int32_t *k, void *stream);
int nefii_adaptive_finalise(const double *sum, const double *stat, int64_t n_pixels, int columns, uint64_t mask_columns,
                            float *out, int32_t *rays, float *variance, void *stream);

/* Exact signed distance from n_points query points to a triangle mesh through a bounding-volume hierarchy (DESIGN.md 6k;
 * added without a struct change: NEFII_ABI_VERSION stays).  Replaces the queries x faces products of
 * datasets/sdf_dataset.py:MeshSDF.__call__ (reference code/datasets/sdf_dataset.py:18-77: mesh-to-sdf's
 * sample_sdf_near_surface).  Everything is fp64 and in ONE frame (MeshSDF's skewed frame): tris [n_tris][9] = (a | b | c), the
 * faces in tree order; the tree is the implicit complete binary tree in heap order over n_leaves_pow2 = N leaves (children
 * of node i: 2 i + 1, 2 i + 2; leaves: nodes N - 1 .. 2 N - 2), leaf j holding the faces [j leaf_size, min((j + 1) leaf_size,
 * n_tris)); node_box [2 N - 1][6] = (lo.xyz, hi.xyz), 16-byte aligned, every face inside its leaf's box, every box containing
 * its children's, empty nodes lo = +inf, hi = -inf (nefii_amd/mesh_bvh.py builds all of it).  points [n_points][3].
 * out [n_points] = the distance to the nearest face (MeshSDF's point-triangle formulas, to rounding), negated when want_sign
 * != 0 and the ray q + t z, t > 0, crosses an odd number of faces (MeshSDF's parity terms, term for term: a closed mesh is
 * asked for, as there).  One thread per query, one launch, no workspace, no atomics: a query's result is the same bits
 * wherever it sits in the batch, from run to run and for any order of the faces.
 * Refused before anything is enqueued: a NULL pointer or a node_box that is not 16-byte aligned (NEFII_E_ARG); n_tris outside
 * 1 .. 2^26 - 1, leaf_size outside 1 .. 8, n_leaves_pow2 not a power of two in 1 .. 2^26 or with n_leaves_pow2 leaf_size <
 * n_tris, n_points < 0 or >= 2^31 (NEFII_E_SHAPE).  n_points == 0 returns 0 without a launch. */
int nefii_mesh_sdf_query(const double *node_box, int64_t n_leaves_pow2, const double *tris /* [F,9] sorted */,
                         int64_t n_tris, int leaf_size, const double *points, int64_t n_points, int want_sign, double *out,
                         void *stream);

/* Generalized winding number of n_points query points about the same mesh, through the same tree (added
 * without a struct change: NEFII_ABI_VERSION stays).  out_w [n_points] = the sum of the faces' signed solid angles seen from
 * the query, over 4 pi: 1 inside a closed mesh whose normals (b - a) x (c - a) point outwards, 0 outside, 2 where two closed
 * parts overlap, and it varies smoothly across a hole - the sign  w > 0.5  needs no closed mesh, which the parity count of
 * nefii_mesh_sdf_query does.  node_box, n_leaves_pow2, tris, leaf_size, points: as there.  node_moment [2 N - 1][8] =
 * (p.xyz, r, n.xyz, area) per node, 16-byte aligned (nefii_amd/mesh_bvh.py:build_moments): n = the sum of the node's faces'
 * area vectors 0.5 (b - a) x (c - a), area = the sum of their areas (0: an empty node, skipped), p = the area-weighted mean
 * of their centroids, r = a radius about p that holds every vertex of the node.
 * One thread per query, one depth-first traversal, the left child first: a leaf adds the exact solid angle of each of its
 * faces, 2 atan2(A . (B x C), |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|) with A = a - q, ... (Van Oosterom & Strackee; finite
 * for every finite input, a query on a vertex or in a face's plane included); an inner node with beta > 0 and |d|^2 >
 * (beta r)^2, d = p - q, adds the dipole term n . d / |d|^3 and is not descended; every other inner node is descended.
 * beta == 0 never approximates: the exact sum over all faces.  The traversal reads the moments and the faces; node_box is
 * checked and otherwise unused.  One launch, no workspace, no atomics, all fp64, no fused products: the order of the additions
 * is fixed per query, so its result is the same bits wherever it sits in the batch and from run to run.  It is a floating-
 * point sum in tree order, so - unlike nefii_mesh_sdf_query's results - it is NOT invariant under a permutation of the faces.
 * Refused before anything is enqueued: a NULL pointer, a node_box or node_moment that is not 16-byte aligned, beta NaN,
 * negative or in (0, 1) - the expansion means nothing inside the bounding sphere - (NEFII_E_ARG); the shapes
 * nefii_mesh_sdf_query refuses (NEFII_E_SHAPE).  n_points == 0 returns 0 without a launch. */
int nefii_mesh_winding_query(const double *node_box, const double *node_moment, int64_t n_leaves_pow2, const double *tris,
                             int64_t n_tris, int leaf_size, const double *points, int64_t n_points, double beta,
                             double *out_w, void *stream);

/* Connected components of a triangle mesh (added without a struct change: NEFII_ABI_VERSION stays).  Replaces
 * trimesh's Trimesh.split in the reference's get_surface_high_res_mesh (code/utils/plots.py:186-189).  faces [n_faces][3]
 * int32, parent [n_verts] int32, flags [2] int32 = (changed, bad input), all on the device.  nefii_mesh_cc_init sets
 * parent[v] = v and clears both flags.  nefii_mesh_cc_round clears flags[0], then runs one hook pass (per face: the least
 * grandparent g of its three vertices is written, by atomicMin on int32, to the three parents' entries and the three
 * vertices' entries; flags[0] = 1 if an entry was lowered) and one jump pass (per vertex: parent[v] = its root).  parent[x] <=
 * x holds throughout and entries only decrease, so every chase ends; no compare-and-swap loop, no spin.  The caller repeats
 * rounds, reading flags after each, until flags[0] == 0: then parent[v] is the SMALLEST vertex index of the edge-connected
 * component of v (a vertex in no face: v itself) - the same bits for any schedule, any order of the faces and from run to
 * run.  4 ceil(log2(max(n_verts, 2))) + 8 rounds are more than any mesh measured needs (nefii_amd/ops/mesh.py: mesh_components).
 * Duplicated faces and faces with repeated indices are legal.  A face with an index outside [0, n_verts) is not followed: it
 * sets flags[1] (sticky until the next init) and is skipped.  No allocation, no synchronisation.
 * Refused before anything is enqueued: a NULL pointer (NEFII_E_ARG); n_verts or n_faces negative or >= 2^31 (NEFII_E_SHAPE).
 * n_verts == 0 returns 0 without a launch; a round with n_faces == 0 only clears flags[0]. */
int nefii_mesh_cc_init(int32_t *parent, int64_t n_verts, int32_t *flags, void *stream);
int nefii_mesh_cc_round(const int32_t *faces, int64_t n_faces, int32_t *parent, int64_t n_verts, int32_t *flags,
                        void *stream);

/* The representative vertex of every cluster of a vertex-clustering simplification: the regularised minimiser of the cluster's
 * quadric error (Lindstrom 2000; added without a struct change: NEFII_ABI_VERSION stays).  The reference has
 * no counterpart.  All arrays on the device: verts [n_verts][3] fp32; faces [n_faces][3] int32; cluster [n_verts] int32, in
 * [0, n_clusters) for every vertex a face uses (anything, -1 by convention, for the others); corners [3 n_faces] int32, the
 * corners t = 3 face + k sorted STABLY by cluster[faces[t]] (ties: ascending t); seg [n_clusters + 1] int64, cluster c owning
 * corners[seg[c] .. seg[c + 1]); centre [n_clusters][3] fp64, the centre of the cluster's cell; pos [n_clusters][3] fp32;
 * flags [2] int32 = (an index outside its range, a cluster outside its range or a corner list that does not match it).
 * h: the cell's edge, eps: the regularisation, clamp: the half-width of the box the result is kept in (cell units), all fp64
 * ON THE HOST.  Per cluster c, all in fp64 and in local coordinates p' = (p - centre_c) (1 / h): for every corner of its run,
 * with (a0, a1, a2) the corner's face, nn = (a1' - a0') x (a2' - a0'), n = nn / |nn|, w = |nn| / 2 (the area over h^2), d =
 * -n . a0':   A += w n n^T,  b += w d n,  s += the corner's vertex',  m += 1.   A face counts once per corner it has in the
 * cluster; a face with |nn| == 0 adds to s and m only.  x0 = s / m; trace(A) == 0: x = x0; else (A + eps trace(A) I)(x - x0) =
 * -(b + A x0) by a 3 x 3 Cholesky factorisation (a pivot that is not positive - eps == 0 on a rank-deficient A - keeps x =
 * x0).  x is clamped per component to [-clamp, clamp]; pos = fp32(centre + h x), rounded once.  An empty run gives the centre.
 * 8 lanes own a cluster: lane j sums the run's entries j, j + 8, ... in order, then a fixed xor tree (1, 2, 4) joins the
 * lanes.  No atomics: the bits depend on the inputs alone, from run to run and for any launch geometry.
 * flags are cleared first, then set by a pass over the faces and by the main pass: flags[0] for a face index outside
 * [0, n_verts) or a corner outside [0, 3 n_faces), flags[1] for a used vertex whose cluster is outside [0, n_clusters), a
 * corner whose vertex is not in the run's cluster, or seg entries that are no run of the list.  Such a corner is skipped and
 * never dereferenced; pos is then not to be used.  No allocation, no synchronisation: the caller reads flags.
 * Refused before anything is enqueued: a NULL pointer; h or clamp not in (0, inf), eps not in [0, inf) (NEFII_E_ARG);
 * n_verts, n_faces or n_clusters negative or >= 2^31, 3 n_faces >= 2^31 (NEFII_E_SHAPE).  n_clusters == 0 or n_faces == 0
 * returns 0 without a launch (flags are then left as they are). */
int nefii_mesh_cluster_quadrics(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces,
                                const int32_t *cluster, const int32_t *corners, const int64_t *seg, const double *centre,
                                int64_t n_clusters, double h, double eps, double clamp, float *pos, int32_t *flags,
                                void *stream);

/* Baking a mesh's materials into textures (added without a struct change: NEFII_ABI_VERSION stays).  The
 * reference has no counterpart.  THE ATLAS, stated here once and mirrored by nefii_amd/texture.py and tests/texbake_ref.py:
 * a T x T image (7 <= T <= 8192) of n x n square cells of c texels, n c <= T, the margin beyond n c unused; pad p >= 2 and
 * leg s = c - 3 p >= 1.  Face f lives in cell q = f / 2 at column q % n, row q / n, origin (x0, y0) = (c (q % n), c (q / n)) in
 * texel units; texel (i, j), linear index j T + i, has its centre at (i + 1/2, j + 1/2); j counts image rows from the top.
 *   even face: corners 0, 1, 2 at (x0 + p, y0 + p), (x0 + p + s, y0 + p), (x0 + p, y0 + p + s);
 *   odd face:  corners 0, 1, 2 at (x0 + c - p, y0 + c - p), (x0 + c - p - s, y0 + c - p), (x0 + c - p, y0 + c - p - s);
 *   a texel of cell q with (i - x0) + (j - y0) + 1 < c belongs to face 2 q, every other one to face 2 q + 1; to nobody (-1)
 *   when that face is >= n_faces or the texel lies in the margin i >= n c or j >= n c.
 * With p >= 2 every texel a bilinear lookup at a point inside or on a chart reads with non-zero weight belongs to the chart's
 * face.  All three entry points: one thread per texel or sample, no atomics, no allocation, no synchronisation, the same bits
 * from run to run and for any launch geometry; refused before anything is enqueued: a NULL pointer (NEFII_E_ARG), an atlas
 * outside the limits above (NEFII_E_SHAPE).
 *
 * nefii_bake_raster - the texels first .. first + count - 1 (so that the host can bake in chunks; row k of every output is
 * texel first + k): owner [count] int32; bary [count][2] fp32 (8-byte aligned) = (b1, b2), the barycentric weights of corners 1
 * and 2 of the owner's chart at the texel's OWN CENTRE, b0 = 1 - b1 - b2 - exact rationals k / (2 s), k1 = 2 (i - x0 - p) + 1
 * and k2 = 2 (j - y0 - p) + 1 on an even face, 2 (x0 + c - p - i) - 1 and 2 (y0 + c - p - j) - 1 on an odd one, k0 = 2 s - k1 -
 * k2; gutter texels extrapolate (negative weights), they are not clamped; covered [count] uint8 = k0, k1, k2 all >= 0; pos
 * [count][3] fp32 = (b0 v0 + b1 v1) + b2 v2 in fp64 with b = (double)k / (double)(2 s), rounded once.  Unowned texels: owner
 * -1, zeros elsewhere.  verts [n_verts][3] fp32, faces [n_faces][3] int32.  flags [2] int32 are cleared, then flags[0] is set
 * for an owned face with an index outside [0, n_verts) - it is never followed, pos stays 0 - and flags[1] for a position that
 * is not finite; the caller reads them.  Also refused: 3 n_faces >= 2^31, n_faces > 2 n^2, a range outside [0, T^2]. */
int nefii_bake_raster(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, int T, int n, int c, int p,
                      int64_t first, int64_t count, int32_t *owner, uint8_t *covered, float *bary, float *pos, int32_t *flags,
                      void *stream);
/* nefii_bake_encode - n texels of baked float maps to 8-bit levels, in fp64: level(x) = floor(255 min(max(x, 0), 1) + 0.5), NaN
 * as 0.  rgba_albedo [n][4] = level(max(albedo, 0)^(1 / 2.2)) (the tone map of the PLY's vertex colours), rgba_normal [n][4] =
 * level(0.5 normal + 0.5) (object space), grey_roughness [n] = level(roughness); alpha 255.  A texel with owner < 0: all of its
 * bytes 0.  albedo, normal [n][3], roughness [n] fp32; the two rgba outputs 4-byte aligned. */
int nefii_bake_encode(const float *albedo, const float *roughness, const float *normal, const int32_t *owner, int64_t n,
                      uint8_t *rgba_albedo, uint8_t *rgba_normal, uint8_t *grey_roughness, void *stream);
/* nefii_texture_sample - out [count][C] fp32 = the bilinear lookup of tex [T][T][C] fp32 (C in 1 .. 4) at the atlas position of
 * (face [count] int32, bary [count][3] fp64): with (ax, ay) corner 0 of the face's chart and d = +1 (even) or -1 (odd), x = (b0
 * ax + b1 (ax + d s)) + b2 ax, y = (b0 ay + b1 ay) + b2 (ay + d s); u = x - 1/2, v = y - 1/2; the texels floor(u), floor(u) + 1
 * x floor(v), floor(v) + 1, each index clamped to [0, T - 1], weights (1 - wx)(1 - wy), wx (1 - wy), (1 - wx) wy, wx wy with wx
 * = u - floor(u), summed in that order; all in fp64, rounded once.  A face < 0 or without a cell (face / 2 >= n^2): zeros. */
int nefii_texture_sample(const float *tex, int T, int C, const int32_t *face, const double *bary, int n, int c, int p,
                         int64_t count, float *out, void *stream);
/* Ambient occlusion and bent normals of the baked texels (two symbols, no struct change).  Both: one thread per
 * texel looping over the K samples, rows of m elements read and written by consecutive threads, no atomics, no shared memory,
 * the same bits from run to run and for any split of the texels into calls.  Refused before anything is enqueued: a NULL
 * pointer (NEFII_E_ARG; uniforms alone may be NULL), K outside 1 .. 1024, m < 0 or m >= 2^31 (NEFII_E_SHAPE).  m == 0 returns 0.
 *
 * nefii_bake_ao_rays - pos, normal (unit) [m][3], sdf, gnorm [m] fp32: the texels' points, the SDF there and the norm of its
 * gradient; texel [m] int64: the texel's global index g = j T + i.  origins [m][3] = fl(x + fl(t n)) with t = bias - sdf / gnorm:
 * a first-order lift onto the level set plus the offset bias along the normal.  dirs [K][m][3] (sample-major), uniforms
 * [K][m][2] (8-byte aligned, optional).  Sample s of texel g, all fp32 in this order, a function of (g, s, K, seed) alone:
 *   lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 in uint32;
 *   h0 = lowbias32(uint32(g) ^ lowbias32(seed)), h1 = lowbias32(h0 + 0x9e3779b9); r0 = (h0 >> 8) 2^-24, r1 = (h1 >> 8) 2^-24;
 *   u0 = r0 + fl((s + 0.5f) / K), less 1 if >= 1, then min(u0, 1 - 2^-24); u1 = r1 + brev(s) 2^-32, less 1 if >= 1;
 *   phi = 2 PI_F u1; l = (sqrt(u0) cos phi, sqrt(u0) sin phi, sqrt(1 - u0)) - the cosine-weighted density;
 *   w = to_world(l, n) of csrc/mc_sampling.h; where n.x < -0.9, at whose end (-1, 0, 0) that frame vanishes, w = to_world((l.x,
 *   l.y, -l.z), -n) instead: the same l.z n on a frame as well conditioned as the n.x > 0.9 one;
 *   dir = w / sqrt(w . w): to_world's tangents are short by 1e-6 / |t|, up to 2.3e-6.
 *
 * nefii_bake_ao_accumulate - hit [K][m] uint8, hit_pts [K][m][3], origins [m][3], dirs [K][m][3], normal [m][3].  Sample s
 * occludes when hit is set and (distance <= 0 or d2 <= distance distance), d2 = (dx dx + dy dy) + dz dz in fp32 with d = hit_pt -
 * origin; the point of a miss is never looked at.  ao [m] = float(K - occluded) / float(K).  bent [m][3] = the sum of the
 * unoccluded dirs in order of s, accumulated and normalised in fp64 and rounded once; normal where nothing is unoccluded. */
int nefii_bake_ao_rays(const float *pos, const float *normal, const float *sdf, const float *gnorm, const int64_t *texel,
                       int64_t m, int K, uint32_t seed, float bias, float *origins, float *dirs, float *uniforms, void *stream);
int nefii_bake_ao_accumulate(const uint8_t *hit, const float *hit_pts, const float *origins, const float *dirs,
                             const float *normal, int64_t m, int K, float distance, float *ao, float *bent, void *stream);
/* The diffuse lightmap of the baked texels under a map light (two symbols, no struct change): the direct
 * irradiance E(x) = integral of L(R^T w) V(x, w) max(n . w, 0) dw, L the map's nearest texel as nefii_envlight_radiance reads it,
 * V the visibility against the SDF, estimated with K = K_cos + K_map rays per texel under the multi-sample balance heuristic.
 * Both: the layout, the determinism and the limits of the two entry points above (1 <= K <= 1024, either share may be 0).
 * Refused before anything is enqueued: a NULL pointer other than uniforms and rot, uniforms not 8-byte aligned, coord other
 * than 0 or 1 (NEFII_E_ARG); a negative share, K outside 1 .. 1024, m < 0 or m >= 2^31, height or width < 1 or height width >=
 * 2^31 (NEFII_E_SHAPE).  m == 0 returns 0.
 *
 * nefii_bake_irradiance_rays - pos, normal, sdf, gnorm, texel, seed, bias, origins: as nefii_bake_ao_rays.  map [height][width][3]
 * fp32 and table: the light and its nefii_envlight_build table; coord 0 (y up) or 1 (z up); rot: 9 floats on the device, R
 * world-from-light row-major, or NULL; rot_identity != 0 (or rot NULL): the rotation is skipped, not multiplied.  dirs, weight
 * [K][m][3], uniforms [K][m][2] (optional), sample-major.  With h0, h1, r0, r1 of nefii_bake_ao_rays, h2 = lowbias32(h1 +
 * 0x9e3779b9), h3 = lowbias32(h2 + 0x9e3779b9), r2 = (h2 >> 8) 2^-24, r3 = (h3 >> 8) 2^-24, and seq(ra, rb, s, n) = (ra + fl((s +
 * 0.5f) / n) less 1 if >= 1 then min(., 1 - 2^-24), rb + brev(s) 2^-32 less 1 if >= 1):
 *   row s < K_cos: (u0, u1) = seq(r0, r1, s, K_cos) and dir as nefii_bake_ao_rays has them for K := K_cos - the same bits; (i, j,
 *   sin phi) = the texel under R^T dir and the sine of its polar angle as nefii_envlight_pdf_rot finds them;
 *   row s >= K_cos: (u0, u1) = seq(r2, r3, s - K_cos, K_map); i = the first row with M[i] > u0, j = the first column with C[i][j]
 *   > u1, each with its continuous offset (x - cdf[k - 1]) / (cdf[k] - cdf[k - 1]) clamped to [0, 1 - 2^-24], v = (i + dv) /
 *   height, u = (j + du) / width, dir = R direction(u, v), sin phi = sinpi(v): nefii_envlight_mis_sample_rot's row 2;
 *   p_map = P(i, j) height width / (2 PI_F^2 sin phi) with P = (M[i] - M[i - 1]) (C[i][j] - C[i][j - 1]) from the stored floats, 0
 *   where sin phi = 0; c = max(n . dir, 0); den = K_cos (c / PI_F) + K_map p_map; weight = map[i][j] (c / den), and exactly 0
 *   where c = 0 or den = 0.  All fp32 in this order.
 *
 * nefii_bake_irradiance_accumulate - hit [K][m] uint8, weight [K][m][3].  A row whose three weights are 0 contributes nothing and
 * its hit is never read (the host need not trace it); of the others those with hit == 0 count.  irradiance [m][3] = their sum in
 * order of s, in fp64, rounded once.  noise [m] = the estimated standard error of the luminance y = ((w0 + w1) + w2) / 3 (fp64):
 * per technique t (rows s < K_cos; the others) with n_t its row count and S_t, Q_t the sums of y and y y over its counted rows,
 * var = sum over the techniques with n_t >= 2 of (Q_t - S_t S_t / n_t) (n_t / (n_t - 1)); noise = sqrt(max(var, 0)) rounded once. */
int nefii_bake_irradiance_rays(const float *pos, const float *normal, const float *sdf, const float *gnorm, const int64_t *texel,
                               int64_t m, int K_cos, int K_map, uint32_t seed, float bias, const float *map, const void *table,
                               int height, int width, int coord, const float *rot, int rot_identity, float *origins, float *dirs,
                               float *weight, float *uniforms, void *stream);
int nefii_bake_irradiance_accumulate(const uint8_t *hit, const float *weight, int64_t m, int K_cos, int K_map, float *irradiance,
                                     float *noise, void *stream);

/* PSNR / SSIM / MS-SSIM statistics of image pairs, in fp64 (added without a struct change: NEFII_ABI_VERSION
 * stays).  Restates scripts/evaluate.py's _ssim_cs and calculate_ms_ssim (Wang et al. 2003 / 2004 as pytorch-msssim has
 * them).  x, y: fp32 [B][H][W][C] on the device; everything after the load is fp64.  window: 11 doubles ON THE HOST, the
 * normalised Gaussian exactly as the caller formed it (it is copied into the launch, never recomputed).  Per level image
 * h x w: mu1, mu2, e11, e22, e12 = the separable 'valid' filterings of x, y, x x, y y, x y; s11 = e11 - mu1^2, s22 = e22 -
 * mu2^2, s12 = e12 - mu1 mu2; cs = (2 s12 + c2) / (s11 + s22 + c2); ssim = (2 mu1 mu2 + c1) / (mu1^2 + mu2^2 + c1) cs.
 * stats [B][levels][C][2] = (mean ssim, mean cs) over the (h - 10) x (w - 10) valid positions; sq_err [B][C] = sum (x - y)^2
 * over all H W pixels of level 0.  Level l + 1 is the 2 x 2 average (divisor 4) of level l, kept in fp64 in the workspace: an
 * even side pairs the inputs (2 i, 2 i + 1); an odd side s gives s / 2 + 1 outputs over (2 i - 1, 2 i), what lies outside
 * read as 0.  The relu, the weighted product over the levels and the mean over the channels are the caller's.  levels = 1
 * (SSIM) or 5 (MS-SSIM; level 0 of it is SSIM's).  No atomics; the partial sums are combined in an order that depends on
 * the shape alone: two runs give the same bits, and an image's numbers do not depend on its place in the batch.
 * nefii_image_metrics_workspace_bytes: the workspace (8-byte aligned) that call needs, or the refusal code, negative.
 * Refused before anything is enqueued: a NULL pointer, levels other than 1 or 5 (NEFII_E_ARG); C outside 1 .. 4, B outside
 * 1 .. 65535, H or W below 11 or above 16384, levels = 5 with H or W <= 160 (NEFII_E_SHAPE). */
int64_t nefii_image_metrics_workspace_bytes(int B, int H, int W, int C, int levels);
int nefii_image_metrics(const float *x, const float *y, int B, int H, int W, int C, int levels, const double *window,
                        double c1, double c2, void *workspace, double *stats, double *sq_err, void *stream);

/* Per-point MC shading sum of pt_render_diff_shadow_indirect_mlp (diff_geo=False), path_tracing_render.py:1406-1476:
 * light [3,n,3] = sum of light SGs along wi (nefii_env_radiance_forward with eps 1e-6), visibility [3,n],
 * indirect [3,n,3] radiance at secondary hits; specular [3] global, roughness [n], albedo [n,3]. */
int nefii_mc_shade_forward(const float *specular, const float *roughness, const float *albedo, const float *normal,
                           const float *view, const float *wi, const float *own_pdf, const float *pdf_table,
                           const float *light, const float *visibility, const float *indirect, int64_t n,
                           float *rgb, float *spec_rgb, float *diff_rgb, void *stream);
/* Gradients wrt light [3,n,3], indirect [3,n,3], albedo [n,3], roughness [n] (overwritten) and, when non-NULL,
 * the global specular [3] (accumulated atomically into a zero-initialised buffer). */
int nefii_mc_shade_backward(const float *specular, const float *roughness, const float *albedo, const float *normal,
                            const float *view, const float *wi, const float *own_pdf, const float *pdf_table,
                            const float *light, const float *visibility, const float *indirect, int64_t n,
                            const float *d_rgb, const float *d_spec, const float *d_diff, float *g_light,
                            float *g_indirect, float *g_albedo, float *g_roughness, float *g_specular, void *stream);

/* IDRLoss.forward (code/model/loss.py:278-320) for the terms the shipped confs weight: masked L1/L2/SmoothL1 of idr_rgb
 * and sg_rgb against the ground truth over rays with network_object_mask & object_mask (:163-184), the mask BCE over
 * the others (:186-196), the normal-smoothness variance over 2r x 2r patches (:198-207) and the background colour term
 * over rays missing both masks; eikonal is zero under frozen geometry.  The SSIM and roughness-smoothness terms are
 * nefii_idr_patch_loss's, below; the view-diff term is not built.
 * losses[0..5] = loss, idr_rgb_loss, sg_rgb_loss, mask_loss, normalsmooth_loss, background_rgb_loss;
 * d_idr_rgb / d_sg_rgb [n,3] (either may be NULL) receive d loss / d input in the same launch.
 * Every per-ray array holds n rows.  NEFII_E_SHAPE, with nothing enqueued, when n < 1 or when the normal-smoothness term
 * is on (r_patch >= 1 and a non-zero normalsmooth_weight) and n is not a multiple of the patch size 4 r_patch^2: the
 * reference's view(-1, 4 r^2, 3) raises there, and no ray is ever left out of a term. */
typedef struct nefii_loss_params {
    float idr_rgb_weight, sg_rgb_weight, mask_weight, alpha, normalsmooth_weight, background_rgb_weight;
    int32_t loss_type;       /* 0 L1, 1 L2, 2 SmoothL1(beta 1) */
    int32_t env_loss_type;   /* 0 L1, 1 L2 */
    int32_t r_patch;         /* patches of (2 r)^2 consecutive rays for the normal-smoothness term; < 1: off */
    int32_t reserved;
} nefii_loss_params;
int nefii_idr_loss(const nefii_loss_params *h_params, const float *idr_rgb, const float *sg_rgb, const float *rgb_gt,
                   const uint8_t *network_object_mask, const uint8_t *object_mask, const float *sdf_output,
                   const float *normals, int64_t n, float *losses, float *d_idr_rgb, float *d_sg_rgb, void *stream);

/* The patch terms of IDRLoss, value and gradient together (added without a struct change: nefii_loss_params
 * and NEFII_ABI_VERSION stay): the SSIM term of idr_rgb and of sg_rgb against rgb_gt (code/model/loss.py:54-120, :237-253)
 * and the roughness-smoothness term (:266-276).  n = N P^2 rays, P = 2 r_patch: patch p owns rows p P^2 .. (p + 1) P^2 - 1,
 * pixel (y, x) of it is row p P^2 + y P + x.  m = network_object_mask & object_mask.
 * SSIM (either SSIM weight non-zero; both values are then reported): per patch and channel the statistics of
 * nefii_image_metrics in fp32 with c1 = 1e-4, c2 = 9e-4 at the valid positions [5, P - 5)^2, S = the mean over the channels of
 * ssim there and 1 elsewhere; e = m eroded by the 11 x 11 window clipped to the patch; M = sum of e over all patches; the
 * term is sum(e (1 - S)) / M, 0 when M = 0.  window: the normalised Gaussian exactly as the caller formed it.
 * Roughness (its weight non-zero): a_p = m over the whole patch; the term is the mean over the patches with a_p of
 * var(roughness) (4 - mean over the channels of var(normal_c)), unbiased variances, 0 when no patch is whole.
 * losses[0..3] = the weighted sum of the three terms, idr_ssim_loss, sg_ssim_loss, roughnesssmooth_loss.  d_idr_rgb,
 * d_sg_rgb [n,3] and d_roughness [n] (each may be NULL) receive d losses[0] / d input; the normals and rgb_gt carry none.
 * Two launches, no atomics (two runs give the same bits), no allocation and no host synchronisation: workspace is the
 * caller's, nefii_idr_patch_loss_workspace_bytes of it (or that call's refusal code, negative), 8-byte aligned.
 * Refused before anything is enqueued: a NULL pointer other than the three gradients (NEFII_E_ARG); r_patch outside 1 .. 16,
 * an SSIM weight non-zero with r_patch below 6 (no valid position, or the reference's own IndexError), n < P^2 or n not a
 * multiple of P^2 (NEFII_E_SHAPE). */
#define NEFII_PATCH_WINDOW 11
typedef struct nefii_patch_loss_params {
    float idr_ssim_weight, sg_ssim_weight, roughnesssmooth_weight;
    int32_t r_patch;
    float window[NEFII_PATCH_WINDOW];
    int32_t reserved;
} nefii_patch_loss_params;
int64_t nefii_idr_patch_loss_workspace_bytes(const nefii_patch_loss_params *h_params, int64_t n);
int nefii_idr_patch_loss(const nefii_patch_loss_params *h_params, const float *idr_rgb, const float *sg_rgb,
                         const float *rgb_gt, const uint8_t *network_object_mask, const uint8_t *object_mask,
                         const float *roughness, const float *normals, int64_t n, void *workspace, float *losses,
                         float *d_idr_rgb, float *d_sg_rgb, float *d_roughness, void *stream);

/* Assembly of the per-ray output buffers of IDRNetwork.forward (implicit_differentiable_renderer.py:441-501): the reference
 * allocates eight [n_rays, C] buffers of ones / zeros and writes the shaded hit rays into them by boolean mask, one pair of
 * launches per buffer.  Here: all buffers in two launches.  Block b: dst [rows, cols] is filled with `fill`, then row
 * where[i] takes row i of src (src_row_stride floats apart: cols, or 0 for one row broadcast to every hit), i < n_src.
 * Several i may name the same row (the graph step pads its hit list with a scratch row): any of them wins.
 * nefii_gather_rows is the adjoint: dst [n_src, cols] <- src[where[i]] (src [rows, cols]: the gradient of an assembled
 * buffer; a block with a NULL src or dst is skipped). */
#define NEFII_MAX_ROW_BLOCKS 12
typedef struct nefii_row_block {
    const float *src;
    float *dst;
    int32_t cols;
    int32_t src_row_stride;
    float fill;
    int32_t reserved;
} nefii_row_block;
int nefii_assemble_rows(const nefii_row_block *h_blocks, int n_blocks, const int64_t *where, int64_t n_src, int64_t rows,
                        void *stream);
int nefii_gather_rows(const nefii_row_block *h_blocks, int n_blocks, const int64_t *where, int64_t n_src, int64_t rows,
                      void *stream);

/* ABI 12 - the inputs of get_rbg_value for the compacted hit rays in one launch (implicit_differentiable_renderer.py:358-364:
 * points[mask], -ray_dirs[mask]; :537-545: gradient / (norm + 1e-6), view / (norm + 1e-6)): row i of the outputs is taken from
 * row where[i] of points / ray_dirs / grad [rows, 3] (the SDF gradient at the traced points) and, when feat_cols > 0, of
 * feat_src [rows, feat_cols] -> pts_out, view_out (= -dir, normalised), nrm_out [n, 3], feat_out [n, feat_cols]. */
int nefii_prepare_hits(const float *points, const float *ray_dirs, const float *grad, const float *feat_src, int feat_cols,
                       const int64_t *where, int64_t n, int64_t rows, float *pts_out, float *view_out, float *nrm_out,
                       float *feat_out, void *stream);

/* ABI 12 - EnvmapMaterialNetwork.forward's head for GLOBAL roughness / specular parameters (physg.conf;
 * sg_envmap_material.py:381-414) in one launch each way: rough_out [1] = (1 - 0.089) sigmoid(rough_param[0]) + 0.089,
 * spec_out [3] = 0.16 sigmoid(spec_param)^2 (n_spec = 1: white specular, the value repeated; 3: per channel); fake_rough /
 * fake_spec (the warm-up flags, idr_train.py:705-713) put 0.5 in place of the sigmoid.  Backward: d_rough [1], d_spec [3]
 * (either may be NULL) -> g_rough_param [1], g_spec_param [n_spec] (overwritten). */
int nefii_material_head_global(const float *rough_param, const float *spec_param, int n_spec, int fake_rough, int fake_spec,
                               float *rough_out, float *spec_out, void *stream);
int nefii_material_head_global_backward(const float *rough_param, const float *spec_param, int n_spec, int fake_rough,
                                        int fake_spec, const float *d_rough, const float *d_spec, float *g_rough_param,
                                        float *g_spec_param, void *stream);

/* MEASUREMENT, not part of the reference's path: what the matrix cores of THIS device sustain on dense fp16 MFMAs with
 * random operands and nothing else in the instruction stream (v_mfma_f32_16x16x32_f16, four accumulator chains per wave,
 * one wave per SIMD, every CU): runs `groups` groups of 8 MFMAs per wave on 256 workgroups, synchronises, and returns the
 * elapsed milliseconds and the FLOPs executed.  MI355X is power-limited under such a loop (2.0 PFLOP/s on zero operands,
 * ~1.5 on random ones: profiles/r04/slot_probe.txt), so bench.py quotes roofline.sustained_peak beside the 2.5 PFLOP/s
 * spec peak the roofline fraction is priced against. */
int nefii_mfma_sustained_probe(int groups, float *h_ms, double *h_flops, void *stream);
/* The same loop on `chains` = 4 or 8 independent accumulator chains (a group is then 2 x chains MFMAs).  With 4 chains the
 * loop takes 148 cycles per 8 MFMAs against 128 for a free-running pipe (each accumulator is wanted again after 64 cycles of
 * issue); 8 chains leave every dependency 128 cycles - bench.py quotes both, so that the sustained figure is not an artefact
 * of the probe's own issue rate.  (ABI 12) */
int nefii_mfma_sustained_probe_chains(int groups, int chains, float *h_ms, double *h_flops, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* NEFII_AMD_H */
