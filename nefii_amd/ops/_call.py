"""What the wrappers of every kernel family share: width rounding, tensor -> pointer, the stream, the checked launch
and the argument checks."""
import torch

from .. import _lib


def _round32(v):
    return (v + 31) // 32 * 32


def _pad_hidden(v):
    """nefii_padded_width: hidden/output widths are multiples of 64 once wider than one 32-column tile."""
    return _round32(v) if v <= 32 else (v + 63) // 64 * 64


def need_gpu(*tensors):
    """the one RuntimeError for an argument that is not a tensor on the GPU"""
    if not all(torch.is_tensor(t) and t.is_cuda for t in tensors):
        raise RuntimeError('nefii_amd ops need GPU tensors (the hot path has no CPU fallback)')


def check_tensor(name, t, dtype, shape):
    """ValueError unless t is a contiguous tensor of `dtype` and of `shape`, whose None entries stand for any size"""
    if not torch.is_tensor(t) or t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError('%s must be a tensor of shape [%s], got %s' % (name, ', '.join('*' if s is None else str(s) for s in shape),
                                                                        tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError('%s must be contiguous %s, got %s with strides %s' % (name, dtype, t.dtype, t.stride()))


def _ptr(t):
    if t is None:
        return None
    if not t.is_cuda:
        need_gpu(t)
    if not t.is_contiguous():
        raise RuntimeError('tensor must be contiguous')
    return t.data_ptr()


def _f32(t):
    if t is None:
        return None
    return t.detach().to(torch.float32).contiguous()


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream():
    """hipStream_t of torch's current stream on the current device (the raw getter is ~20x cheaper than building a
    torch.cuda.Stream object: ~1300 calls per 300 steps of config 1)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def call(name, *args, stream=None):
    """lib.<name>(*args, stream), the status checked under the same name; stream: torch's current one unless given"""
    _lib.check(getattr(_lib.lib(), name)(*args, _stream() if stream is None else stream), name)


def nbytes(name, *args):
    """lib.<name>(*args), a workspace size in bytes: a negative one is a status"""
    n = getattr(_lib.lib(), name)(*args)
    if n < 0:
        _lib.check(int(n), name)
    return n
