"""Tensor-level wrappers and autograd glue over the C ABI (include/nefii_amd.h).

PyTorch is plumbing here: it owns device memory, the stream and the autograd graph between the
HIP kernels; every hot op below runs in libnefii_hip.so.  There is no eager fallback - without the
library (or without a GPU tensor) these functions raise.

One module per kernel family.  Callers use `ops.X`: every module-level name of every module is re-exported here,
underscore names included, and process-wide state (stream pools, workspaces) lives once, in the module that uses it.
Tests and tools replace names on this package; that reaches a call made through `ops.X` only, so no module here calls
another module's public function that they patch (denoise_atrous, denoise_atrous_variance, pixel_moments, image_metrics,
mis_sample, ray_luminance_moments and the adaptive_* ops)."""
from .._lib import (ACT_ELU, ACT_RELU, ACT_SOFTPLUS100, HEAD_ABS, HEAD_NONE, HEAD_POW2, HEAD_RELU,  # noqa: F401
                    HEAD_RELU_INIT, HEAD_SIGMOID, HEAD_TANH01, Mlp, TracerParams)
from . import _call, envfit, envlight, image, loss, mesh, mlp, shading, tracer

for _m in (_call, mlp, tracer, shading, loss, envfit, envlight, image, mesh):
    globals().update((k, v) for k, v in vars(_m).items() if not k.startswith('__'))
