"""ctypes binding of libmemc_hip_blend_grad.so (include/memc_warp_blend_grad.h): the float32 backward of one direction of
the fused dual warp + occlusion blend for callers that do not want the image gradient.

The library is loaded on first use, not at import: users of ``my_package`` that never train never touch it.  The blend's
backward requires it: a call without it raises RuntimeError (there is no fallback for a missing library).

Arguments are float32 torch CUDA tensors of 4 dimensions.  Return value: the C function's int -- 0 enqueued, 1 a shape the
kernel does not cover (nothing touched: the caller composes the warp's entry points), -1 a failed check.  Work is enqueued
on the current HIP stream of the tensors' device; nothing synchronises.
"""
import ctypes
import os
import threading

import torch

from ..my_lib_lp import _Tensor4 as Tensor4, _describe as describe   # the same descriptors (lazy: loads nothing)

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libmemc_hip_blend_grad.so")

_lib = None
_lock = threading.Lock()


def lib():
    """The loaded library (loaded once, on first use)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        "libmemc_hip_blend_grad.so not found at %s -- build it with `make -C %s` (or `python -c 'import "
                        "__graft_entry__ as g; g.build()'` at the repo root); the blend's fused backward has no fallback"
                        % (LIB_PATH, os.path.join(_PKG_ROOT, "csrc")))
                L = ctypes.CDLL(LIB_PATH)
                L.memc_blend_grad_version.restype = ctypes.c_char_p
                L.memc_blend_grad_last_kernel_path.restype = ctypes.c_char_p
                f = L.FilterInterpolationBlendLayer_gpu_backward
                f.restype = ctypes.c_int
                f.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(Tensor4)] * 8
                _lib = L
    return _lib


def version():
    return lib().memc_blend_grad_version().decode()


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "fi_blend_bwd:tiled_c3"; "" before the first."""
    return lib().memc_blend_grad_last_kernel_path().decode()


def FilterInterpolationBlendLayer_gpu_backward(input, flow, filter, occlusion, gradoutput, gradflow, gradfilter,
                                               gradocclusion):
    """gradflow, gradfilter and gradocclusion (all assigned: no zero fill needed) of ONE direction of
    occlusion0 * FI(input0, flow0, filter0) + occlusion1 * FI(input2, flow1, filter1) for the blend's raw gradoutput."""
    symbol = "FilterInterpolationBlendLayer_gpu_backward"
    cfunc = getattr(lib(), symbol)
    tensors = (input, flow, filter, occlusion, gradoutput, gradflow, gradfilter, gradocclusion)
    dev = input.device
    cargs = []
    for i, t in enumerate(tensors):
        cargs.append(ctypes.byref(describe(t, symbol, i)))
        if t.device != dev:
            raise TypeError("%s: all tensors must live on the same device" % symbol)
        if t.dtype != torch.float32:
            raise TypeError("%s arg %d: expected float32, got %s" % (symbol, i, t.dtype))
    with torch.cuda.device(dev):
        return int(cfunc(torch.cuda.current_stream(dev).cuda_stream, *cargs))


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "FilterInterpolationBlendLayer_gpu_backward"]
