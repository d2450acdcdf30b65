"""ctypes binding of libmemc_hip_mx.so (include/memc_warp_mx.h): the RGB adaptive-warp forward and the fused dual warp +
occlusion blend on MIXED tensors -- float32 image(s) and output, float16 / bfloat16 filter taps and occlusions, the flow in
float32 or the taps' dtype.  This is the call torch.autocast makes: the frames stay float32, the heads return half tensors.

The library is loaded on first use, not at import: users of ``my_package`` that never make a mixed call never touch it.
It is required for such calls: one without it raises RuntimeError (there is no fallback for a missing library).

Arguments are torch CUDA tensors of 4 dimensions.  Return value: the C function's int -- 0 enqueued, 1 a call the kernels
do not cover (nothing touched: the caller promotes to float32), -1 a failed check.  Work is enqueued on the current HIP
stream of the tensors' device; nothing synchronises.
"""
import torch

from .._satellite import Satellite

_SAT = Satellite("libmemc_hip_mx.so", "memc_mx", "mixed-precision warps have no fallback",
                 {"FilterInterpolationLayer_gpu_forward_mx": (2, 4), "FilterInterpolationBlendLayer_gpu_forward_mx": (2, 9)})
LIB_PATH, lib, version = _SAT.path, _SAT.lib, _SAT.version


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "fi_fwd_mx:tiled_c3" or
    "fi_blend_mx:tiled_c3"; "" before the first."""
    return _SAT.last_kernel_path()


def FilterInterpolationLayer_gpu_forward_mx(input1, input2, input3, output):
    """output (float32) = FilterInterpolation(input1 (float32), input2 (flow), input3 (half taps))."""
    f32, t, ft = torch.float32, input3.dtype, input2.dtype
    return _SAT.call("FilterInterpolationLayer_gpu_forward_mx", (input3, input2), (input1, input2, input3, output),
                     dtypes=(f32, ft, t, f32))


def FilterInterpolationBlendLayer_gpu_forward_mx(input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1,
                                                 output):
    """output (float32) = occlusion0 * FI(input0, flow0, filter0) + occlusion1 * FI(input2, flow1, filter1): float32
    images, half taps and occlusions; nothing is rounded."""
    f32, t, ft = torch.float32, filter0.dtype, flow0.dtype
    return _SAT.call("FilterInterpolationBlendLayer_gpu_forward_mx", (filter0, flow0),
                     (input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1, output),
                     dtypes=(f32, f32, ft, ft, t, t, t, t, f32))


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "FilterInterpolationLayer_gpu_forward_mx",
           "FilterInterpolationBlendLayer_gpu_forward_mx"]
