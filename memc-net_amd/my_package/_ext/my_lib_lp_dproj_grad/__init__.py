"""ctypes binding of libmemc_hip_lp_dproj_grad.so (include/memc_warp_lp_dproj_grad.h): the backward of
DepthFlowProjectionLayer on a float16 / bfloat16 flow, depth, gradoutput and gradients beside the float32 count and the
float32 output of the (float32) forward.  This is the depth-weighted projection's backward of a model cast to bfloat16 /
float16.

The library is loaded on first use, not at import: users of ``my_package`` that never ask for this route never touch it.
It is required for such calls: one without it raises RuntimeError (there is no fallback for a missing library).

Arguments are torch CUDA tensors of 4 dimensions.  Return value: the C function's int -- 0 enqueued, 1 a call the kernel
does not cover (nothing touched: the caller widens and takes my_lib.DepthFlowProjectionLayer_gpu_backward), -1 a failed
check.  Work is enqueued on the current HIP stream of the tensors' device; nothing synchronises.
"""
import torch

from .._satellite import Satellite

_SYMBOL = "DepthFlowProjectionLayer_gpu_backward_lp"
_SAT = Satellite("libmemc_hip_lp_dproj_grad.so", "memc_lp_dproj_grad",
                 "the half-precision depth projection backward has no fallback", {_SYMBOL: (1, 7)})
LIB_PATH, lib, version = _SAT.path, _SAT.lib, _SAT.version


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "dproj_bwd_lp:tiled"; "" before the first one."""
    return _SAT.last_kernel_path()


def DepthFlowProjectionLayer_gpu_backward_lp(input1, input2, count, output, gradoutput, gradinput1, gradinput2):
    """gradinput1 and gradinput2 (assigned in every element: no zero fill needed) of the projection of the flow input1
    weighted by the depth input2, for gradoutput and the forward's count and output.  input1, input2, gradoutput,
    gradinput1 and gradinput2 are of ONE half dtype, count and output are float32; any other pattern -- a float32 flow, a
    depth or a gradient of another dtype, a half count or output -- is a TypeError."""
    t = getattr(input1, "dtype", None)
    if t not in (torch.float16, torch.bfloat16):
        raise TypeError("%s arg 0: expected a float16 or bfloat16 flow, got %s (float32 calls: my_lib)" % (_SYMBOL, t))
    return _SAT.call(_SYMBOL, (input1,), (input1, input2, count, output, gradoutput, gradinput1, gradinput2),
                     dtypes=(t, t, torch.float32, torch.float32, t, t, t))


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "DepthFlowProjectionLayer_gpu_backward_lp"]
