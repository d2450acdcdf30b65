"""ctypes binding of libmemc_hip_mx_grad.so (include/memc_warp_mx_grad.h): the RGB adaptive-warp backward on MIXED tensors
-- a float32 image and a float32 gradoutput, float16 / bfloat16 filter taps and tap gradient, the flow and its gradient in
float32 or the taps' dtype.  This is the backward of the call torch.autocast makes (my_lib_mx is its forward).

The library is loaded on first use, not at import: users of ``my_package`` that never differentiate a mixed call never
touch it.  It is required for such calls: one without it raises RuntimeError (there is no fallback for a missing library).

Arguments are torch CUDA tensors of 4 dimensions; gradinput1 is None or a float32 buffer that the kernel adds into.  Return
value: the C function's int -- 0 enqueued, 1 a call the kernel does not cover (nothing touched: the caller promotes to
float32), -1 a failed check.  Work is enqueued on the current HIP stream of the tensors' device; nothing synchronises.
"""
import torch

from .._satellite import Satellite

_SAT = Satellite("libmemc_hip_mx_grad.so", "memc_mx_grad", "the mixed-precision backward has no fallback",
                 {"FilterInterpolationLayer_gpu_backward_mx": (2, 7)})
LIB_PATH, lib, version = _SAT.path, _SAT.lib, _SAT.version


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "fi_bwd_mx:tiled_c3" (with the image
    gradient) or "fi_bwd_mx:tiled_c3_noimage"; "" before the first one."""
    return _SAT.last_kernel_path()


def FilterInterpolationLayer_gpu_backward_mx(input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3):
    """gradinput2 / gradinput3 (assigned) and, unless gradinput1 is None, gradinput1 (float32, added into) of
    FilterInterpolation(input1 (float32), input2 (flow), input3 (half taps)) for gradoutput (float32).  Tap dtype:
    input3's, flow dtype: input2's."""
    f32, t, ft = torch.float32, input3.dtype, input2.dtype
    return _SAT.call("FilterInterpolationLayer_gpu_backward_mx", (input3, input2),
                     (input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3),
                     optional=(4,), dtypes=(f32, ft, t, f32, f32, ft, t))   # NULL: the image gradient is not wanted


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "FilterInterpolationLayer_gpu_backward_mx"]
