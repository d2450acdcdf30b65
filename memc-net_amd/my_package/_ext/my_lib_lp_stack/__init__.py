"""ctypes binding of libmemc_hip_lp_stack.so (include/memc_warp_lp_stack.h): the STACKED adaptive-warp forward on float16 /
bfloat16 tensors -- the warps of several neighbours written straight into channel slices of one wider tensor, the flow and
the taps stored to slices of their own on the way.  This is the call the rectifier input of a MEMC_Net_VE cast to half
precision is made of.

The library is loaded on first use, not at import: users of ``my_package`` that never make a stacked half call never touch
it.  It is required for such calls: one without it raises RuntimeError (there is no fallback for a missing library).

Arguments are torch CUDA tensors of 4 dimensions and five ints.  input1, taps and out share one dtype, float16 or
bfloat16; the flow is of that dtype or float32 (anything else: TypeError).  Return value: the C function's int -- 0
enqueued, 1 a call the kernel does not cover (nothing touched: the caller composes it), -1 a failed check.  Work is
enqueued on the current HIP stream of the tensors' device; nothing synchronises.
"""
import ctypes

import torch

from .._satellite import DTYPES, Satellite, Tensor4, describe

_SYMBOL = "FilterInterpolationStackLayer_gpu_forward_lp"
_SAT = Satellite("libmemc_hip_lp_stack.so", "memc_lp_stack",
                 "the stacked half-precision warp has no fallback for a missing library", {})
# the entry point takes five ints BEHIND the descriptors (Satellite's table spells leading dtype codes only)
_SAT.table.append((_SYMBOL, ctypes.c_int,
                   [ctypes.c_void_p] + [ctypes.c_int] * 2 + [ctypes.POINTER(Tensor4)] * 4 + [ctypes.c_int] * 5))
LIB_PATH, lib, version = _SAT.path, _SAT.lib, _SAT.version
_HALF = (torch.float16, torch.bfloat16)


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "fi_fwd_stack_lp:tiled_c3" or
    "fi_fwd_stack_lp:tiled_c4n"; "" before the first."""
    return _SAT.last_kernel_path()


def FilterInterpolationStackLayer_gpu_forward_lp(input1, flow, taps, out, n_neighbours, c_base, skip, flow_base=-1,
                                                 tap_base=-1):
    """out[b, c_base + slot(n) * C + c] = FilterInterpolation(input1, flow, taps)[n * B + b, c], slot(n) = n + (skip >= 0 and
    n >= skip); with flow_base / tap_base >= 0 also out[b, flow_base + 2 * n + i] = flow[n * B + b, i] (a float32 flow
    rounded to out's dtype) and out[b, tap_base + 16 * n + k] = taps[n * B + b, k].  Payload dtype: input1's."""
    tensors = (input1, flow, taps, out)
    cargs = [ctypes.byref(describe(t, _SYMBOL, i)) for i, t in enumerate(tensors)]
    dev, payload = input1.device, input1.dtype
    if payload not in _HALF:
        raise TypeError("%s arg 0: expected torch.float16 or torch.bfloat16, got %s" % (_SYMBOL, payload))
    for i, t in enumerate(tensors):
        if t.device != dev:
            raise TypeError("%s: all tensors must live on the same device" % _SYMBOL)
        if t.dtype != payload and not (i == 1 and t.dtype == torch.float32):
            raise TypeError("%s arg %d: expected %s%s, got %s" % (_SYMBOL, i, payload, " or torch.float32" if i == 1 else "",
                                                                  t.dtype))
    with torch.cuda.device(dev):
        return int(getattr(_SAT.lib(), _SYMBOL)(torch.cuda.current_stream(dev).cuda_stream, DTYPES[payload],
                                                DTYPES[flow.dtype], *cargs, int(n_neighbours), int(c_base), int(skip),
                                                int(flow_base), int(tap_base)))


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "FilterInterpolationStackLayer_gpu_forward_lp"]
