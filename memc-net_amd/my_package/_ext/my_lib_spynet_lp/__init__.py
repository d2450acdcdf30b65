"""ctypes binding of libmemc_hip_spynet_lp.so (include/memc_spynet_lp.h): the 8-channel input of one SPyNet pyramid level --
[first, second warped with the upsampled and doubled coarser flow, that flow] -- written by one kernel on float16 / bfloat16
frames, coarse flow and output.  This is the call the flow estimator of a MEMC_Net_s cast to bfloat16 / float16 makes at every
pyramid level, where `SPyNet.fused_level_half` asks for it.

The library is loaded on first use, not at import: users of ``my_package`` that never ask for this route never touch it.
It is required for such calls: one without it raises RuntimeError (there is no fallback for a missing library).

Arguments are torch CUDA tensors of 4 dimensions, all of ONE half dtype, and two ints.  Return value: the C function's int --
0 enqueued, 1 a call the library declines (nothing touched: the caller composes it), -1 a failed check.  Work is enqueued on
the current HIP stream of the tensors' device; nothing synchronises.
"""
import ctypes

import torch

from .._satellite import DTYPES, Satellite, Tensor4, describe

_SYMBOL = "SpyNetLevelLayer_gpu_forward_lp"
_SAT = Satellite("libmemc_hip_spynet_lp.so", "memc_spynet_lp",
                 "the half-precision SPyNet level has no fallback for a missing library", {})
# the dtype code leads, as in Satellite's table; the two ints stand BEHIND the descriptors, which that table does not spell
_SAT.table.append((_SYMBOL, ctypes.c_int,
                   [ctypes.c_void_p, ctypes.c_int] + [ctypes.POINTER(Tensor4)] * 4 + [ctypes.c_int] * 2))
LIB_PATH, lib, version = _SAT.path, _SAT.lib, _SAT.version


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "spynet_level_lp:quad" or
    "spynet_level_lp:direct"; "" before the first."""
    return _SAT.last_kernel_path()


def SpyNetLevelLayer_gpu_forward_lp(first, second, coarse, out, align_upsample, align_sample):
    """out[:, 0:3] = first (its bits); out[:, 6:8] = up = 2 * bilinear_x2(coarse), replicate-padded to first's size;
    out[:, 3:6] = second sampled bilinearly with zero padding at (x, y) + the unrounded up.  Computed in float32 on the
    exactly widened inputs, every stored element rounded once.  All four tensors are of ONE half dtype; anything else is a
    TypeError (float32 calls: my_lib_spynet)."""
    tensors = (first, second, coarse, out)
    cargs = [ctypes.byref(describe(t, _SYMBOL, i)) for i, t in enumerate(tensors)]
    dev, dtype = first.device, first.dtype
    if dtype not in (torch.float16, torch.bfloat16):
        raise TypeError("%s arg 0: expected torch.float16 or torch.bfloat16, got %s (float32 calls: my_lib_spynet)"
                        % (_SYMBOL, dtype))
    for i, t in enumerate(tensors):
        if t.device != dev:
            raise TypeError("%s: all tensors must live on the same device" % _SYMBOL)
        if t.dtype != dtype:
            raise TypeError("%s arg %d: expected %s, got %s" % (_SYMBOL, i, dtype, t.dtype))
    with torch.cuda.device(dev):
        return int(getattr(_SAT.lib(), _SYMBOL)(torch.cuda.current_stream(dev).cuda_stream, DTYPES[dtype], *cargs,
                                                int(bool(align_upsample)), int(bool(align_sample))))


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "SpyNetLevelLayer_gpu_forward_lp"]
