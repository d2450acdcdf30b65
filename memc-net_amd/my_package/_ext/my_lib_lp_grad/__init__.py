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
from .._satellite import DTYPES, Satellite

_SAT = Satellite("libmemc_hip_lp_grad.so", "memc_lp_grad", "the half-precision backward has no fallback",
                 {"FilterInterpolationLayer_gpu_backward_lp": (3, 7)})
LIB_PATH, lib, version = _SAT.path, _SAT.lib, _SAT.version


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "fi_bwd_lp:tiled_c3" (with the image
    gradient) or "fi_bwd_lp:tiled_c3_noimage"; "" before the first one."""
    return _SAT.last_kernel_path()


def FilterInterpolationLayer_gpu_backward_lp(input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3):
    """gradinput2 / gradinput3 (assigned) and, unless gradinput1 is None, gradinput1 (float32, added into) of
    FilterInterpolation(input1, input2 (flow), input3 (taps)) for gradoutput.  Payload dtype: input1's, flow dtype:
    input2's, gradoutput dtype: its own."""
    return _SAT.call("FilterInterpolationLayer_gpu_backward_lp", (input1, input2, gradoutput),
                     (input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3),
                     optional=(4,))                          # NULL: the image gradient is not wanted


__all__ = ["LIB_PATH", "DTYPES", "lib", "version", "last_kernel_path", "FilterInterpolationLayer_gpu_backward_lp"]
