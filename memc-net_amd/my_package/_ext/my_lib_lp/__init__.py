"""ctypes binding of libmemc_hip_lp.so (include/memc_warp_lp.h): the adaptive-warp forward and the fused dual warp +
occlusion blend on float16 / bfloat16 tensors.

The library is loaded on first use, not at import: float32 users of ``my_package`` never touch it.  It is required for
half tensors: a call without it raises RuntimeError (there is no fallback).

Arguments are torch CUDA tensors of 4 dimensions.  The payload tensors (image, taps, occlusions, output) share one dtype,
float16 or bfloat16; the flow is float32 or that dtype.  Return value: the C function's int (0 ok, -1 failed check).
Work is enqueued on the current HIP stream of the tensors' device; nothing synchronises.
"""
from .._satellite import DTYPES, Satellite, Tensor4 as _Tensor4, describe as _describe   # noqa: F401  (re-exported)

_SAT = Satellite("libmemc_hip_lp.so", "memc_lp", "half-precision warps have no fallback",
                 {"FilterInterpolationLayer_gpu_forward_lp": (2, 4), "FilterInterpolationBlendLayer_gpu_forward_lp": (2, 9)})
LIB_PATH, lib, version = _SAT.path, _SAT.lib, _SAT.version


def last_kernel_path():
    """The kernel family the most recent call of THIS thread took, e.g. "fi_fwd_lp:tiled_c3"; "direct" is the
    one-lane-per-site fallback (filter sizes other than 4, widths not a multiple of four or below 8, misaligned views)."""
    return _SAT.last_kernel_path()


def FilterInterpolationLayer_gpu_forward_lp(input1, input2, input3, output):
    """output = FilterInterpolation(input1, input2 (flow), input3 (taps)); payload dtype: input1's, flow dtype: input2's."""
    return _SAT.call("FilterInterpolationLayer_gpu_forward_lp", (input1, input2), (input1, input2, input3, output))


def FilterInterpolationBlendLayer_gpu_forward_lp(input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1,
                                                 output):
    """output = occlusion0 * FI(input0, flow0, filter0) + occlusion1 * FI(input2, flow1, filter1), rounded once."""
    return _SAT.call("FilterInterpolationBlendLayer_gpu_forward_lp", (input0, flow0),
                     (input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1, output))


__all__ = ["LIB_PATH", "DTYPES", "lib", "version", "last_kernel_path", "FilterInterpolationLayer_gpu_forward_lp",
           "FilterInterpolationBlendLayer_gpu_forward_lp"]
