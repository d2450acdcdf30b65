"""ctypes binding of libmemc_hip_lp_bl.so (include/memc_warp_lp_bl.h): the plain bilinear warp (Interpolation /
InterpolationCh) on a float16 / bfloat16 image and output beside a flow of that dtype or float32 -- forward for any channel
count, backward for RGB.  This is the bilinear warp of a model cast to bfloat16 / float16.

The library is loaded on first use, not at import: users of ``my_package`` that never ask for this route never touch it.
It is required for such calls: one without it raises RuntimeError (there is no fallback for a missing library).

Arguments are torch CUDA tensors of 4 dimensions.  Return value: the C function's int -- 0 enqueued, 1 (backward only) a
call the kernel does not cover (nothing touched: the caller widens and takes my_lib's float32 backward), -1 a failed check.
Work is enqueued on the current HIP stream of the tensors' device; nothing synchronises.
"""
import torch

from .._satellite import Satellite

_FWD = ("InterpolationLayer_gpu_forward_lp", "InterpolationChLayer_gpu_forward_lp")
_BWD = ("InterpolationLayer_gpu_backward_lp", "InterpolationChLayer_gpu_backward_lp")
_SAT = Satellite("libmemc_hip_lp_bl.so", "memc_lp_bl", "the half-precision bilinear warp has no fallback",
                 dict([(s, (2, 3)) for s in _FWD] + [(s, (2, 5)) for s in _BWD]))
LIB_PATH, lib, version = _SAT.path, _SAT.lib, _SAT.version


def last_kernel_path():
    """The kernel family the most recent enqueued call of THIS thread took: "bl_fwd_lp:tiled_c3", "bl_fwd_lp:tiled_chunks",
    "bl_fwd_lp:direct" or "bl_bwd_lp:tiled_c3"; "" before the first one."""
    return _SAT.last_kernel_path()


def _dtypes(symbol, input1, input2):
    """(image dtype, flow dtype) of a call: a half image, a flow of that dtype or float32 -- anything else is a TypeError"""
    t, ft = getattr(input1, "dtype", None), getattr(input2, "dtype", None)
    if t not in (torch.float16, torch.bfloat16):
        raise TypeError("%s arg 0: expected a float16 or bfloat16 image, got %s (float32 calls: my_lib)" % (symbol, t))
    if ft not in (torch.float32, t):
        raise TypeError("%s arg 1: expected a float32 or %s flow, got %s" % (symbol, t, ft))
    return t, ft


def _forward(symbol, input1, input2, output):
    t, ft = _dtypes(symbol, input1, input2)
    return _SAT.call(symbol, (input1, input2), (input1, input2, output), dtypes=(t, ft, t))


def _backward(symbol, input1, input2, gradoutput, gradinput1, gradinput2):
    t, ft = _dtypes(symbol, input1, input2)
    return _SAT.call(symbol, (input1, input2), (input1, input2, gradoutput, gradinput1, gradinput2),
                     dtypes=(t, ft, t, torch.float32, ft))


def InterpolationLayer_gpu_forward_lp(input1, input2, output):
    """output (assigned in every element) = the bilinear warp of the RGB image input1 by the flow input2.  input1 and output
    are of ONE half dtype, input2 of that dtype or float32; any other pattern is a TypeError."""
    return _forward(_FWD[0], input1, input2, output)


def InterpolationChLayer_gpu_forward_lp(input1, input2, output):
    """The same for any channel count."""
    return _forward(_FWD[1], input1, input2, output)


def InterpolationLayer_gpu_backward_lp(input1, input2, gradoutput, gradinput1, gradinput2):
    """The backward of that warp: gradinput1, a FLOAT32 buffer of input1's shape and layout that the kernel adds into (zero
    it first, round it afterwards), and gradinput2, of the flow's dtype, assigned at every site.  gradoutput is of input1's
    dtype.  1: not covered (nothing touched)."""
    return _backward(_BWD[0], input1, input2, gradoutput, gradinput1, gradinput2)


def InterpolationChLayer_gpu_backward_lp(input1, input2, gradoutput, gradinput1, gradinput2):
    """The same for any channel count (the kernel covers three: every other count returns 1)."""
    return _backward(_BWD[1], input1, input2, gradoutput, gradinput1, gradinput2)


__all__ = ["LIB_PATH", "lib", "version", "last_kernel_path", "InterpolationLayer_gpu_forward_lp",
           "InterpolationChLayer_gpu_forward_lp", "InterpolationLayer_gpu_backward_lp",
           "InterpolationChLayer_gpu_backward_lp"]
