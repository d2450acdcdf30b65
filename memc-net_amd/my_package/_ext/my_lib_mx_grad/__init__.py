"""ctypes binding of libmemc_hip_mx_grad.so (include/memc_warp_mx_grad.h): the RGB adaptive-warp backward on MIXED tensors
-- a float32 image and a float32 gradoutput, float16 / bfloat16 filter taps and tap gradient, the flow and its gradient in
float32 or the taps' dtype.  This is the backward of the call torch.autocast makes (my_lib_mx is its forward).

The library is loaded on first use, not at import: users of ``my_package`` that never differentiate a mixed call never
touch it.  It is required for such calls: one without it raises RuntimeError (there is no fallback for a missing library).

Arguments are torch CUDA tensors of 4 dimensions; gradinput1 is None or a float32 buffer that the kernel adds into.  Return
value: the C function's int -- 0 enqueued, 1 a call the kernel does not cover (nothing touched: the caller promotes to
float32), -1 a failed check.  Work is enqueued on the current HIP stream of the tensors' device; nothing synchronises.
"""
import ctypes
import os
import threading

import torch

from ..my_lib_lp import DTYPES, _Tensor4 as Tensor4, _describe as describe   # the same descriptors (lazy: loads nothing)

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libmemc_hip_mx_grad.so")

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
                        "libmemc_hip_mx_grad.so not found at %s -- build it with `make -C %s` (or `python -c 'import "
                        "__graft_entry__ as g; g.build()'` at the repo root); the mixed-precision backward has no fallback"
                        % (LIB_PATH, os.path.join(_PKG_ROOT, "csrc")))
                L = ctypes.CDLL(LIB_PATH)
                L.memc_mx_grad_version.restype = ctypes.c_char_p
                L.memc_mx_grad_last_kernel_path.restype = ctypes.c_char_p
                f = L.FilterInterpolationLayer_gpu_backward_mx
                f.restype = ctypes.c_int
                f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(Tensor4)] * 7
                _lib = L
    return _lib


def version():
    return lib().memc_mx_grad_version().decode()


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "fi_bwd_mx:tiled_c3" (with the image
    gradient) or "fi_bwd_mx:tiled_c3_noimage"; "" before the first one."""
    return lib().memc_mx_grad_last_kernel_path().decode()


def FilterInterpolationLayer_gpu_backward_mx(input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3):
    """gradinput2 / gradinput3 (assigned) and, unless gradinput1 is None, gradinput1 (float32, added into) of
    FilterInterpolation(input1 (float32), input2 (flow), input3 (half taps)) for gradoutput (float32).  Tap dtype:
    input3's, flow dtype: input2's."""
    symbol = "FilterInterpolationLayer_gpu_backward_mx"
    cfunc = getattr(lib(), symbol)
    f32, t, ft = torch.float32, input3.dtype, input2.dtype
    tensors = (input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3)
    dtypes = (f32, ft, t, f32, f32, ft, t)       # tensors[i] must be of dtypes[i]: the C side sees bytes and cannot tell
    dev = input1.device
    cargs = []
    for i, (x, dt) in enumerate(zip(tensors, dtypes)):
        if x is None and i == 4:
            cargs.append(None)                               # NULL: the image gradient is not wanted
            continue
        cargs.append(ctypes.byref(describe(x, symbol, i)))
        if x.device != dev:
            raise TypeError("%s: all tensors must live on the same device" % symbol)
        if x.dtype != dt:
            raise TypeError("%s arg %d: expected %s, got %s" % (symbol, i, dt, x.dtype))
    with torch.cuda.device(dev):
        return int(cfunc(torch.cuda.current_stream(dev).cuda_stream, DTYPES[t], DTYPES[ft], *cargs))


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "FilterInterpolationLayer_gpu_backward_mx"]
