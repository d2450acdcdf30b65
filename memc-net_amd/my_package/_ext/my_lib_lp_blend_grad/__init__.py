"""ctypes binding of libmemc_hip_lp_blend_grad.so (include/memc_warp_lp_blend_grad.h): the backward of one direction of the
fused dual warp + occlusion blend on float16 / bfloat16 tensors -- a half image, half filter taps and occlusion and their
gradients, the flow and its gradient in float32 or that dtype, gradoutput in float32 or that dtype -- for callers that do
not want the image gradient.  This is the blend's backward of a model cast to bfloat16 / float16 (my_lib_lp is its forward).

The library is loaded on first use, not at import: users of ``my_package`` that never ask for this route never touch it.
It is required for such calls: one without it raises RuntimeError (there is no fallback for a missing library).

Arguments are torch CUDA tensors of 4 dimensions.  Return value: the C function's int -- 0 enqueued, 1 a call the kernel
does not cover (nothing touched: the caller composes the warp's entry points), -1 a failed check.  Work is enqueued on the
current HIP stream of the tensors' device; nothing synchronises.

A binding of its own: my_lib_blend_grad.FilterInterpolationBlendLayer_gpu_backward, the door of the float32 and mixed
kernels, rejects half images and never comes here.  The layer calls this one only where it was constructed with
``fused_half_backward=True``.
"""
import torch

from .._satellite import Satellite

_SYMBOL = "FilterInterpolationBlendLayer_gpu_backward_lp"
_SAT = Satellite("libmemc_hip_lp_blend_grad.so", "memc_lp_blend_grad", "the half-precision blend backward has no fallback",
                 {_SYMBOL: (3, 8)})
LIB_PATH, lib, version = _SAT.path, _SAT.lib, _SAT.version


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "fi_blend_bwd_lp:tiled_c3"; "" before the
    first one."""
    return _SAT.last_kernel_path()


def FilterInterpolationBlendLayer_gpu_backward_lp(input, flow, filter, occlusion, gradoutput, gradflow, gradfilter,
                                                  gradocclusion):
    """gradflow, gradfilter and gradocclusion (all assigned: no zero fill needed) of ONE direction of the blend of input,
    filter and occlusion (ONE half dtype) and flow (float32 or that dtype) for the blend's raw gradoutput (float32 or that
    dtype).  Payload dtype: input's, flow dtype: flow's, gradoutput dtype: gradoutput's; any other pattern -- a float32
    image, taps of another dtype, a gradient not of its input's dtype -- is a TypeError."""
    t, ft, gt = (getattr(x, "dtype", None) for x in (input, flow, gradoutput))
    if t not in (torch.float16, torch.bfloat16):
        raise TypeError("%s arg 0: expected a float16 or bfloat16 image, got %s (float32 and mixed calls: "
                        "my_lib_blend_grad)" % (_SYMBOL, t))
    for i, d in ((1, ft), (4, gt)):
        if d not in (torch.float32, t):
            raise TypeError("%s arg %d: expected float32 or %s, got %s" % (_SYMBOL, i, t, d))
    return _SAT.call(_SYMBOL, (input, flow, gradoutput),
                     (input, flow, filter, occlusion, gradoutput, gradflow, gradfilter, gradocclusion),
                     dtypes=(t, ft, t, t, gt, ft, t, t))


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "FilterInterpolationBlendLayer_gpu_backward_lp"]
