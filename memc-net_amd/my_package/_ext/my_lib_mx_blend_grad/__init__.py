"""ctypes binding of libmemc_hip_mx_blend_grad.so (include/memc_warp_mx_blend_grad.h): the backward of one direction of the
fused dual warp + occlusion blend on MIXED tensors -- a float32 image and a float32 gradoutput, float16 / bfloat16 filter
taps and occlusion and their gradients, the flow and its gradient in float32 or the taps' dtype -- for callers that do not
want the image gradient.  This is the blend's backward of the call torch.autocast makes (my_lib_mx is its forward).

The library is loaded on first use, not at import: users of ``my_package`` that never differentiate a mixed blend never
touch it.  It is required for such calls: one without it raises RuntimeError (there is no fallback for a missing library).

Arguments are torch CUDA tensors of 4 dimensions.  Return value: the C function's int -- 0 enqueued, 1 a call the kernel
does not cover (nothing touched: the caller promotes to float32), -1 a failed check.  Work is enqueued on the current HIP
stream of the tensors' device; nothing synchronises.

The layer reaches this binding through my_lib_blend_grad.FilterInterpolationBlendLayer_gpu_backward, its one door to the
fused blend backward whatever the storage.
"""
import torch

from .._satellite import Satellite

_SAT = Satellite("libmemc_hip_mx_blend_grad.so", "memc_mx_blend_grad", "the mixed-precision blend backward has no fallback",
                 {"FilterInterpolationBlendLayer_gpu_backward_mx": (2, 8)})
LIB_PATH, lib, version = _SAT.path, _SAT.lib, _SAT.version


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "fi_blend_bwd_mx:tiled_c3"; "" before the
    first one."""
    return _SAT.last_kernel_path()


def FilterInterpolationBlendLayer_gpu_backward_mx(input, flow, filter, occlusion, gradoutput, gradflow, gradfilter,
                                                  gradocclusion):
    """gradflow, gradfilter and gradocclusion (all assigned: no zero fill needed) of ONE direction of the blend of input
    (float32), flow, filter and occlusion (half) for the blend's raw gradoutput (float32).  Tap dtype: filter's, flow
    dtype: flow's."""
    f32, t, ft = torch.float32, filter.dtype, flow.dtype
    return _SAT.call("FilterInterpolationBlendLayer_gpu_backward_mx", (filter, flow),
                     (input, flow, filter, occlusion, gradoutput, gradflow, gradfilter, gradocclusion),
                     dtypes=(f32, ft, t, t, f32, ft, t, t))


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "FilterInterpolationBlendLayer_gpu_backward_mx"]
