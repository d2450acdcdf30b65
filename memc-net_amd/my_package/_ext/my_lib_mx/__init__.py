"""ctypes binding of libmemc_hip_mx.so (include/memc_warp_mx.h): the RGB adaptive-warp forward and the fused dual warp +
occlusion blend on MIXED tensors -- float32 image(s) and output, float16 / bfloat16 filter taps and occlusions, the flow in
float32 or the taps' dtype.  This is the call torch.autocast makes: the frames stay float32, the heads return half tensors.

The library is loaded on first use, not at import: users of ``my_package`` that never make a mixed call never touch it.
It is required for such calls: one without it raises RuntimeError (there is no fallback for a missing library).

Arguments are torch CUDA tensors of 4 dimensions.  Return value: the C function's int -- 0 enqueued, 1 a call the kernels
do not cover (nothing touched: the caller promotes to float32), -1 a failed check.  Work is enqueued on the current HIP
stream of the tensors' device; nothing synchronises.
"""
import ctypes
import os
import threading

import torch

from ..my_lib_lp import DTYPES, _Tensor4 as Tensor4, _describe as describe   # the same descriptors (lazy: loads nothing)

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libmemc_hip_mx.so")

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
                        "libmemc_hip_mx.so not found at %s -- build it with `make -C %s` (or `python -c 'import "
                        "__graft_entry__ as g; g.build()'` at the repo root); mixed-precision warps have no fallback"
                        % (LIB_PATH, os.path.join(_PKG_ROOT, "csrc")))
                L = ctypes.CDLL(LIB_PATH)
                L.memc_mx_version.restype = ctypes.c_char_p
                L.memc_mx_last_kernel_path.restype = ctypes.c_char_p
                for name, n in (("FilterInterpolationLayer_gpu_forward_mx", 4),
                                ("FilterInterpolationBlendLayer_gpu_forward_mx", 9)):
                    f = getattr(L, name)
                    f.restype = ctypes.c_int
                    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(Tensor4)] * n
                _lib = L
    return _lib


def version():
    return lib().memc_mx_version().decode()


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "fi_fwd_mx:tiled_c3" or
    "fi_blend_mx:tiled_c3"; "" before the first."""
    return lib().memc_mx_last_kernel_path().decode()


def _call(symbol, taps, flow, tensors, dtypes):
    """tensors[i] must be of dtypes[i]: the C side sees bytes and cannot tell"""
    cfunc = getattr(lib(), symbol)
    dev = tensors[0].device
    cargs = []
    for i, (t, dt) in enumerate(zip(tensors, dtypes)):
        cargs.append(ctypes.byref(describe(t, symbol, i)))
        if t.device != dev:
            raise TypeError("%s: all tensors must live on the same device" % symbol)
        if t.dtype != dt:
            raise TypeError("%s arg %d: expected %s, got %s" % (symbol, i, dt, t.dtype))
    with torch.cuda.device(dev):
        return int(cfunc(torch.cuda.current_stream(dev).cuda_stream, DTYPES[taps.dtype], DTYPES[flow.dtype], *cargs))


def FilterInterpolationLayer_gpu_forward_mx(input1, input2, input3, output):
    """output (float32) = FilterInterpolation(input1 (float32), input2 (flow), input3 (half taps))."""
    f32, t, ft = torch.float32, input3.dtype, input2.dtype
    return _call("FilterInterpolationLayer_gpu_forward_mx", input3, input2, (input1, input2, input3, output),
                 (f32, ft, t, f32))


def FilterInterpolationBlendLayer_gpu_forward_mx(input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1,
                                                 output):
    """output (float32) = occlusion0 * FI(input0, flow0, filter0) + occlusion1 * FI(input2, flow1, filter1): float32
    images, half taps and occlusions; nothing is rounded."""
    f32, t, ft = torch.float32, filter0.dtype, flow0.dtype
    return _call("FilterInterpolationBlendLayer_gpu_forward_mx", filter0, flow0,
                 (input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1, output),
                 (f32, f32, ft, ft, t, t, t, t, f32))


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "FilterInterpolationLayer_gpu_forward_mx",
           "FilterInterpolationBlendLayer_gpu_forward_mx"]
