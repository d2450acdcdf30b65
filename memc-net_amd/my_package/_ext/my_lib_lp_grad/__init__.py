"""ctypes binding of libmemc_hip_lp_grad.so (include/memc_warp_lp_grad.h): the RGB adaptive-warp backward on float16 /
bfloat16 tensors.

The library is loaded on first use, not at import: float32 users of ``my_package`` never touch it.  It is required for the
backward of half warps: a call without it raises RuntimeError, exactly as for my_lib_lp.

Arguments are torch CUDA tensors of 4 dimensions: image, taps and tap gradient of one dtype (float16 or bfloat16), flow
and flow gradient float32 or that dtype, gradoutput float32 or that dtype, gradinput1 None or a float32 buffer that the
kernel adds into.  Return value: the C function's int -- 0 enqueued, 1 a shape the kernel does not cover (nothing
touched: the caller widens to float32), -1 a failed check.  Work is enqueued on the current HIP stream of the tensors'
device; nothing synchronises.
"""
import ctypes
import os
import threading

import torch

from ..my_lib_lp import DTYPES, _Tensor4 as Tensor4, _describe as describe   # the same descriptors (lazy: loads nothing)

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libmemc_hip_lp_grad.so")

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
                        "libmemc_hip_lp_grad.so not found at %s -- build it with `make -C %s` (or `python -c 'import "
                        "__graft_entry__ as g; g.build()'` at the repo root); the half-precision backward has no fallback"
                        % (LIB_PATH, os.path.join(_PKG_ROOT, "csrc")))
                L = ctypes.CDLL(LIB_PATH)
                L.memc_lp_grad_version.restype = ctypes.c_char_p
                L.memc_lp_grad_last_kernel_path.restype = ctypes.c_char_p
                f = L.FilterInterpolationLayer_gpu_backward_lp
                f.restype = ctypes.c_int
                f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(Tensor4)] * 7
                _lib = L
    return _lib


def version():
    return lib().memc_lp_grad_version().decode()


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "fi_bwd_lp:tiled_c3" (with the image
    gradient) or "fi_bwd_lp:tiled_c3_noimage"; "" before the first one."""
    return lib().memc_lp_grad_last_kernel_path().decode()


def FilterInterpolationLayer_gpu_backward_lp(input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3):
    """gradinput2 / gradinput3 (assigned) and, unless gradinput1 is None, gradinput1 (float32, added into) of
    FilterInterpolation(input1, input2 (flow), input3 (taps)) for gradoutput.  Payload dtype: input1's, flow dtype:
    input2's, gradoutput dtype: its own."""
    symbol = "FilterInterpolationLayer_gpu_backward_lp"
    cfunc = getattr(lib(), symbol)
    tensors = (input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3)
    dev = input1.device
    cargs = []
    for i, t in enumerate(tensors):
        if t is None and i == 4:
            cargs.append(None)                               # NULL: the image gradient is not wanted
            continue
        cargs.append(ctypes.byref(describe(t, symbol, i)))
        if t.device != dev:
            raise TypeError("%s: all tensors must live on the same device" % symbol)
    with torch.cuda.device(dev):
        return int(cfunc(torch.cuda.current_stream(dev).cuda_stream, DTYPES[input1.dtype], DTYPES[input2.dtype],
                         DTYPES[gradoutput.dtype], *cargs))


__all__ = ["LIB_PATH", "DTYPES", "lib", "version", "last_kernel_path", "FilterInterpolationLayer_gpu_backward_lp"]
