"""ctypes binding of libmemc_hip_blend_grad.so (include/memc_warp_blend_grad.h): the float32 backward of one direction of
the fused dual warp + occlusion blend for callers that do not want the image gradient.

The library is loaded on first use, not at import: users of ``my_package`` that never train never touch it.  The blend's
backward requires it: a call without it raises RuntimeError (there is no fallback for a missing library).

Arguments are float32 torch CUDA tensors of 4 dimensions (the mixed-precision pattern of my_lib_mx_blend_grad is forwarded
there).  Return value: the C function's int -- 0 enqueued, 1 a shape the
kernel does not cover (nothing touched: the caller composes the warp's entry points), -1 a failed check.  Work is enqueued
on the current HIP stream of the tensors' device; nothing synchronises.
"""
import torch

from .. import my_lib_mx_blend_grad
from .._satellite import Satellite

_SAT = Satellite("libmemc_hip_blend_grad.so", "memc_blend_grad", "the blend's fused backward has no fallback",
                 {"FilterInterpolationBlendLayer_gpu_backward": (0, 8)}, dtype_name=lambda dt: "float32")
LIB_PATH, lib, version = _SAT.path, _SAT.lib, _SAT.version


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "fi_blend_bwd:tiled_c3"; "" before the first."""
    return _SAT.last_kernel_path()


def _mixed(input, flow, filter, occlusion, gradoutput, gradflow, gradfilter, gradocclusion):
    """the storage libmemc_hip_mx_blend_grad.so takes: a float32 image and gradoutput, taps, occlusion and their gradients
    of ONE half dtype, the flow and its gradient in float32 or that dtype"""
    dt = [getattr(x, "dtype", None) for x in (input, flow, filter, occlusion, gradoutput, gradflow, gradfilter, gradocclusion)]
    t = dt[2]
    return (t in (torch.float16, torch.bfloat16) and dt[0] == dt[4] == torch.float32 and dt[3] == dt[6] == dt[7] == t and
            dt[1] in (torch.float32, t) and dt[5] == dt[1])


def FilterInterpolationBlendLayer_gpu_backward(input, flow, filter, occlusion, gradoutput, gradflow, gradfilter,
                                               gradocclusion):
    """gradflow, gradfilter and gradocclusion (all assigned: no zero fill needed) of ONE direction of
    occlusion0 * FI(input0, flow0, filter0) + occlusion1 * FI(input2, flow1, filter1) for the blend's raw gradoutput.
    The layer's one door to the fused blend backward: eight float32 tensors go to libmemc_hip_blend_grad.so; a float32
    image and gradoutput beside float16 / bfloat16 taps and occlusion (flow in float32 or that dtype, each gradient of its
    input's dtype) are forwarded to my_lib_mx_blend_grad (whose last_kernel_path reports that call); any other mix of
    dtypes is a TypeError."""
    args = (input, flow, filter, occlusion, gradoutput, gradflow, gradfilter, gradocclusion)
    if _mixed(*args):
        return my_lib_mx_blend_grad.FilterInterpolationBlendLayer_gpu_backward_mx(*args)
    return _SAT.call("FilterInterpolationBlendLayer_gpu_backward", (), args, dtypes=(torch.float32,) * 8)


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "FilterInterpolationBlendLayer_gpu_backward"]
