"""ctypes binding of libmemc_hip_lp.so (include/memc_warp_lp.h): the adaptive-warp forward and the fused dual warp +
occlusion blend on float16 / bfloat16 tensors.

The library is loaded on first use, not at import: float32 users of ``my_package`` never touch it.  It is required for
half tensors: a call without it raises RuntimeError (there is no fallback).

Arguments are torch CUDA tensors of 4 dimensions.  The payload tensors (image, taps, occlusions, output) share one dtype,
float16 or bfloat16; the flow is float32 or that dtype.  Return value: the C function's int (0 ok, -1 failed check).
Work is enqueued on the current HIP stream of the tensors' device; nothing synchronises.
"""
import ctypes
import os
import threading

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libmemc_hip_lp.so")

# memc_dtype of include/memc_warp_lp.h
DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}

_lib = None
_lock = threading.Lock()


class _Tensor4(ctypes.Structure):
    """memc_tensor4 of include/memc_warp.h"""
    _fields_ = [("data", ctypes.c_void_p),
                ("size", ctypes.c_int64 * 4),
                ("stride", ctypes.c_int64 * 4)]


def lib():
    """The loaded library (loaded once, on first use)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        "libmemc_hip_lp.so not found at %s -- build it with `make -C %s` (or `python -c 'import "
                        "__graft_entry__ as g; g.build()'` at the repo root); half-precision warps have no fallback"
                        % (LIB_PATH, os.path.join(_PKG_ROOT, "csrc")))
                L = ctypes.CDLL(LIB_PATH)
                L.memc_lp_version.restype = ctypes.c_char_p
                L.memc_lp_last_kernel_path.restype = ctypes.c_char_p
                for name, n in (("FilterInterpolationLayer_gpu_forward_lp", 4),
                                ("FilterInterpolationBlendLayer_gpu_forward_lp", 9)):
                    f = getattr(L, name)
                    f.restype = ctypes.c_int
                    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(_Tensor4)] * n
                _lib = L
    return _lib


def version():
    return lib().memc_lp_version().decode()


def last_kernel_path():
    """The kernel family the most recent call of THIS thread took, e.g. "fi_fwd_lp:tiled_c3"; "direct" is the
    one-lane-per-site fallback (filter sizes other than 4, widths not a multiple of four or below 8, misaligned views)."""
    return lib().memc_lp_last_kernel_path().decode()


def _describe(t, symbol, position):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s arg %d: expected a torch.Tensor, got %s" % (symbol, position, type(t).__name__))
    if not t.is_cuda:
        raise TypeError("%s arg %d: expected a CUDA (HIP) tensor; these operators have no CPU path" % (symbol, position))
    if t.dtype not in DTYPES:
        raise TypeError("%s arg %d: expected float16, bfloat16 or float32, got %s" % (symbol, position, t.dtype))
    if t.dim() != 4:
        raise TypeError("%s arg %d: expected a 4-D NCHW tensor, got %d-D" % (symbol, position, t.dim()))
    d = _Tensor4()
    d.data = t.data_ptr()
    d.size[:] = t.shape
    d.stride[:] = t.stride()
    return d


def _call(symbol, payload, flow, tensors):
    cfunc = getattr(lib(), symbol)
    dev = tensors[0].device
    cargs = []
    for i, t in enumerate(tensors):
        cargs.append(ctypes.byref(_describe(t, symbol, i)))
        if t.device != dev:
            raise TypeError("%s: all tensors must live on the same device" % symbol)
    with torch.cuda.device(dev):
        return int(cfunc(torch.cuda.current_stream(dev).cuda_stream, DTYPES[payload.dtype], DTYPES[flow.dtype], *cargs))


def FilterInterpolationLayer_gpu_forward_lp(input1, input2, input3, output):
    """output = FilterInterpolation(input1, input2 (flow), input3 (taps)); payload dtype: input1's, flow dtype: input2's."""
    return _call("FilterInterpolationLayer_gpu_forward_lp", input1, input2, (input1, input2, input3, output))


def FilterInterpolationBlendLayer_gpu_forward_lp(input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1,
                                                 output):
    """output = occlusion0 * FI(input0, flow0, filter0) + occlusion1 * FI(input2, flow1, filter1), rounded once."""
    return _call("FilterInterpolationBlendLayer_gpu_forward_lp", input0, flow0,
                 (input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1, output))


__all__ = ["LIB_PATH", "DTYPES", "lib", "version", "last_kernel_path", "FilterInterpolationLayer_gpu_forward_lp",
           "FilterInterpolationBlendLayer_gpu_forward_lp"]
