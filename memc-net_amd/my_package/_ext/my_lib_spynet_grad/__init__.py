"""ctypes binding of libmemc_hip_spynet_grad.so (include/memc_spynet_grad.h): the gradient of one SPyNet pyramid level's
8-channel input with respect to the coarse flow, by one float32 kernel without atomics.  This is the call a training step of
MEMC_Net_s's flow estimator makes at every pyramid level but the coarsest, where `SPyNet.fused_level_backward` is set.

The library is loaded on first use, not at import: users of ``my_package`` that never train a SPyNet level through it never
touch it.  It is required for such calls: one without it raises RuntimeError (there is no fallback for a missing library).

Arguments are float32 torch CUDA tensors of 4 dimensions and two ints.  Return value: the C function's int -- 0 enqueued,
1 a call the library declines (nothing touched: the caller takes torch's gradient), -1 a failed check.  Work is enqueued on
the current HIP stream of the tensors' device; nothing synchronises.
"""
import ctypes

import torch

from .._satellite import Satellite, Tensor4, describe

_SYMBOL = "SpyNetLevelLayer_gpu_backward"
_SAT = Satellite("libmemc_hip_spynet_grad.so", "memc_spynet_grad",
                 "the SPyNet level backward has no fallback for a missing library", {})
# the entry point takes its ints BEHIND the descriptors (Satellite's table spells leading dtype codes only)
_SAT.table.append((_SYMBOL, ctypes.c_int, [ctypes.c_void_p] + [ctypes.POINTER(Tensor4)] * 4 + [ctypes.c_int] * 2))
LIB_PATH, lib, version = _SAT.path, _SAT.lib, _SAT.version


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "spynet_level_bwd:tiled"; "" before the first."""
    return _SAT.last_kernel_path()


def SpyNetLevelLayer_gpu_backward(second, coarse, gradoutput, gradcoarse, align_upsample, align_sample):
    """gradcoarse = d(sum(gradoutput * level_input)) / d(coarse): gradoutput[:, 6:8] and the warp's derivative with respect
    to the upsampled flow, through the adjoint of the x2 upsampling.  Every element of gradcoarse is assigned."""
    tensors = (second, coarse, gradoutput, gradcoarse)
    cargs = [ctypes.byref(describe(t, _SYMBOL, i)) for i, t in enumerate(tensors)]
    dev = second.device
    for i, t in enumerate(tensors):
        if t.device != dev:
            raise TypeError("%s: all tensors must live on the same device" % _SYMBOL)
        if t.dtype != torch.float32:
            raise TypeError("%s arg %d: expected torch.float32, got %s" % (_SYMBOL, i, t.dtype))
    with torch.cuda.device(dev):
        return int(getattr(_SAT.lib(), _SYMBOL)(torch.cuda.current_stream(dev).cuda_stream, *cargs,
                                                int(bool(align_upsample)), int(bool(align_sample))))


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "SpyNetLevelLayer_gpu_backward"]
