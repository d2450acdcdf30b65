"""FilterInterpolationLayer -- flow sample fused with the per-pixel 4x4 (fs x fs) adaptive filter.

Mirrors my_package/functions/FilterInterpolationLayer.py of the reference: same class name, same call
surface (`FilterInterpolationLayer()(input1, input2, input3)`), same zero-filled caller-allocated buffers,
same gradients (gradinput1, gradinput2, gradinput3).  The reference is a legacy instance-style
autograd.Function (rejected by torch >= 1.3); here the instance is a thin callable over a static Function.

Differences, all deliberate:
  * the reference hands the ORIGINAL (possibly non-contiguous) tensors to C while caching contiguous copies
    (:14-16,29), so a non-contiguous input makes C return -1 and a zero tensor comes back silently;
    here the contiguous copies are what the kernel sees;
  * a non-zero return code raises instead of being ignored (:29) / printed (:56-57);
  * CPU tensors raise (the reference's CPU branch dies with NameError);
  * float16 / bfloat16 and mixed precision, by the dtypes of the call (functions/_common.py: payload_dtype is
    torch.promote_types over input1 and input3; "half" is float16 or bfloat16; the flow stays float32 or the half dtype,
    any other flow dtype is cast to float32; "covered" is three channels, the 4x4 filter, a width that is a multiple of
    four from 8 on: lp_backward_covered).  A library declines with return code 1 and has touched nothing then.

    image, taps        forward                      backward                                   where the library declines
    -----------------  ---------------------------  -----------------------------------------  ------------------------------
    float32, float32   libmemc_hip                  libmemc_hip                                (raises)
    half, half         libmemc_hip_lp, any shape    covered: libmemc_hip_lp_grad on the saved  widened to float32: libmemc_hip,
                                                    tensors and the gradoutput as it arrives   each gradient cast back
                                                    (92 B per site; widened: 168 B and the
                                                    casts); not covered: as declined
    float32, half,     libmemc_hip_mx on the        libmemc_hip_mx_grad on the saved tensors   forward: flow and taps widened,
    covered            tensors as they are (60 B    as they are and the float32 gradoutput     libmemc_hip; backward: widened,
    (mx_covered)       per site; promoted: 204)     (104 B per site; promoted: about 360)      libmemc_hip, gradients cast back
    any other mix      cast to the payload dtype: one of the first two rows

    Every half or mixed kernel does the float32 kernel's arithmetic on the exactly widened values and rounds each stored
    value once; the image gradient is a float32 buffer (NULL where autograd does not ask for it: _gradinput1_buffer),
    cast to the image's dtype afterwards.  The mixed routes' flow and tap gradients are those of the promoted call, bit
    for bit.  Each library in turn, with its timings: INTEGRATION.md.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import my_package._ext.my_lib as my_lib
import my_package._ext.my_lib_lp as my_lib_lp
import my_package._ext.my_lib_lp_grad as my_lib_lp_grad
import my_package._ext.my_lib_mx as my_lib_mx
import my_package._ext.my_lib_mx_grad as my_lib_mx_grad
from ._common import LOWP, cast, cast_like, check, declined, f32c, flow_dtype, payload_dtype, require_gpu


class _FilterInterpolationFunction(Function):
    @staticmethod
    def forward(ctx, input1, input2, input3):
        require_gpu("FilterInterpolationLayer", input1, input2, input3)
        input1, input2, input3 = f32c(input1), f32c(input2), f32c(input3)
        # the reference zero-fills (:26); the forward kernels write EVERY element (invalid sites copy the input,
        # tests/test_gpu_parity.py::test_forward_outputs_need_no_zero_fill), so the memset -- a quarter of the
        # call's time at 720p -- is skipped.  The C entry point still accepts zero-filled buffers, of course.
        output = torch.empty_like(input1)
        err = my_lib.FilterInterpolationLayer_gpu_forward(input1, input2, input3, output)
        check(err, "FilterInterpolationLayer_gpu_forward")
        ctx.save_for_backward(input1, input2, input3)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        input1, input2, input3 = ctx.saved_tensors
        return _backward_fp32(input1, input2, input3, f32c(gradoutput), ctx.needs_input_grad[0])


def _gradinput1_buffer(input1, input3, want1):
    """The float32 gradinput1 a backward entry point is handed.  None (a NULL pointer) where autograd does not ask for it
    and the libraries serve one -- three channels, the 4x4 filter and a width that is a multiple of four (include/memc_warp.h;
    the warped frames are data in the reference's networks, MEMC_Net_star.py:266-277): the RGB kernel then skips its
    accumulation and this layer its zero fill.  Decided up front, so no first call fails; any other call that wants none
    gets a buffer that is thrown away.  The buffer is the accumulation target, zero-filled (reference :46) -- except where
    the library STORES gradinput1 on every path (four and more channels with the 4x4 filter; include/memc_warp.h:
    memc_gradinput1_is_stored): the memset would be a fifth of the call's traffic."""
    if not want1 and input1.size(1) == 3 and input3.size(1) == 16 and input1.size(3) % 4 == 0:
        return None
    stored = my_lib.gradinput1_is_stored(int(input3.size(1) ** 0.5 + 1e-6), input1.size(1))     # fs as my_lib.c:925
    return (torch.empty_like if stored else torch.zeros_like)(input1, dtype=torch.float32)


def _backward_fp32(input1, input2, input3, gradoutput, want1):
    """(gradinput1 or None, gradinput2, gradinput3) of float32 tensors through the reference-API entry point"""
    gradinput1 = _gradinput1_buffer(input1, input3, want1)
    # the reference zero-fills these two as well (:47-48); the backward kernels DEFINE every element of them
    # (invalid sites store zero; tests/test_gpu_parity.py::test_backward_defines_flow_and_tap_gradients), so
    # 72 B/site of memsets -- a seventh of the call at 720p -- are skipped
    gradinput2 = torch.empty_like(input2)
    gradinput3 = torch.empty_like(input3)
    err = my_lib.FilterInterpolationLayer_gpu_backward(
        input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3)
    if err != 0 and gradinput1 is None:
        # the library declines a NULL gradinput1 for reasons this layer does not duplicate (a plane beyond 32-bit offsets,
        # say): once more with a buffer that is thrown away -- one branch, taken on failure only (round-5 review)
        err = my_lib.FilterInterpolationLayer_gpu_backward(
            input1, input2, input3, gradoutput, torch.zeros_like(input1), gradinput2, gradinput3)
    check(err, "FilterInterpolationLayer_gpu_backward")
    return (gradinput1 if want1 else None), gradinput2, gradinput3


def _backward_widened(saved, gradoutput, want1):
    """the fallback of the half and the mixed Function: the float32 backward on the saved tensors and the gradoutput
    widened (a float32 one passes as it is), each gradient cast back to its input's dtype"""
    input1, input2, input3 = (t.float().contiguous() for t in saved)
    return cast_like(_backward_fp32(input1, input2, input3, gradoutput.float().contiguous(), want1), saved)


def lp_backward_covered(input1, input3):
    """What libmemc_hip_lp_grad.so's kernel takes (include/memc_warp_lp_grad.h): three channels, 16 taps, a width that is a
    multiple of four from 8 on.  (Views it declines all the same -- misaligned, say -- come back as return code 1.)"""
    return input1.size(1) == 3 and input3.size(1) == 16 and input1.size(3) % 4 == 0 and input1.size(3) >= 8


def backward_lp(input1, input2, input3, gradoutput, gradinput1):
    """(gradinput2, gradinput3) of half input1 / input3 on libmemc_hip_lp_grad.so, gradinput1 (None or float32, zero-filled)
    added into; None where the library does not cover the call (return code 1: nothing was touched)"""
    gradinput2 = torch.empty_like(input2)                # every element is written (invalid sites store zero)
    gradinput3 = torch.empty_like(input3)
    err = my_lib_lp_grad.FilterInterpolationLayer_gpu_backward_lp(
        input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3)
    if declined(err, "FilterInterpolationLayer_gpu_backward_lp"):
        return None
    return gradinput2, gradinput3


def _backward_lp(input1, input2, input3, gradoutput, want1):
    """_backward_fp32 on half tensors: the same gradinput1 decision (so the kernel takes the float32 library's PART for the
    call), gradinput1 float32; None where the library does not cover the call"""
    gradinput1 = _gradinput1_buffer(input1, input3, want1)
    if gradoutput.dtype not in (input1.dtype, torch.float32):
        gradoutput = gradoutput.float()
    grads = backward_lp(input1, input2, input3, gradoutput.contiguous(), gradinput1)
    if grads is None:
        return None
    return (gradinput1 if want1 else None,) + grads


class _FilterInterpolationLpFunction(Function):
    """float16 / bfloat16: forward on libmemc_hip_lp.so; backward on libmemc_hip_lp_grad.so where it covers the call, else
    widened to float32"""

    @staticmethod
    def forward(ctx, input1, input2, input3):
        input1, input2, input3 = input1.contiguous(), input2.contiguous(), input3.contiguous()
        output = torch.empty_like(input1)                    # every element is written
        err = my_lib_lp.FilterInterpolationLayer_gpu_forward_lp(input1, input2, input3, output)
        check(err, "FilterInterpolationLayer_gpu_forward_lp")
        ctx.save_for_backward(input1, input2, input3)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        saved = ctx.saved_tensors
        grads = None
        if lp_backward_covered(saved[0], saved[2]):
            grads = _backward_lp(*saved, gradoutput, ctx.needs_input_grad[0])
        if grads is None:
            return _backward_widened(saved, gradoutput, ctx.needs_input_grad[0])
        return cast_like(grads, saved)


def mx_covered(image, taps):
    """The mixed call libmemc_hip_mx.so takes (include/memc_warp_mx.h): a float32 image, half taps, and the shapes of
    lp_backward_covered.  (Views it declines all the same come back as return code 1.)"""
    return image.dtype == torch.float32 and taps.dtype in LOWP and lp_backward_covered(image, taps)


def _backward_mx(input1, input2, input3, gradoutput, want1):
    """_backward_fp32 on the mixed tensors as they are (libmemc_hip_mx_grad.so): the same gradinput1 decision for this
    shape (so the kernel takes the float32 library's PART for the call); None where the library declines the call
    (return code 1: nothing was touched)"""
    gradinput1 = torch.zeros_like(input1) if want1 else None     # (mx_covered: a NULL gradinput1 is served)
    gradinput2 = torch.empty_like(input2)                # every element is written (invalid sites store zero)
    gradinput3 = torch.empty_like(input3)
    err = my_lib_mx_grad.FilterInterpolationLayer_gpu_backward_mx(
        input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3)
    if declined(err, "FilterInterpolationLayer_gpu_backward_mx"):
        return None
    return gradinput1, gradinput2, gradinput3


class _FilterInterpolationMxFunction(Function):
    """a float32 image, float16 / bfloat16 taps, the flow in float32 or the taps' dtype: forward on libmemc_hip_mx.so
    (where it declines: promoted to float32, the float32 kernel); backward on libmemc_hip_mx_grad.so (where it declines:
    the promoted call's, on the widened tensors)"""

    @staticmethod
    def forward(ctx, input1, input2, input3):
        input1, input2, input3 = input1.contiguous(), input2.contiguous(), input3.contiguous()
        output = torch.empty_like(input1)                    # every element is written
        err = my_lib_mx.FilterInterpolationLayer_gpu_forward_mx(input1, input2, input3, output)
        if declined(err, "FilterInterpolationLayer_gpu_forward_mx"):      # the promoted route
            err = my_lib.FilterInterpolationLayer_gpu_forward(input1, input2.float(), input3.float(), output)
            check(err, "FilterInterpolationLayer_gpu_forward")
        ctx.save_for_backward(input1, input2, input3)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        saved, gradoutput = ctx.saved_tensors, f32c(gradoutput)
        grads = _backward_mx(*saved, gradoutput, ctx.needs_input_grad[0])
        if grads is not None:                                # each gradient in its input's dtype already
            return grads
        return _backward_widened(saved, gradoutput, ctx.needs_input_grad[0])      # the promoted route


class FilterInterpolationLayer(object):
    def __init__(self):
        super(FilterInterpolationLayer, self).__init__()

    def __call__(self, input1, input2, input3):
        require_gpu("FilterInterpolationLayer", input1, input2, input3)
        if mx_covered(input1, input3):
            return _FilterInterpolationMxFunction.apply(input1, cast(input2, flow_dtype(input2, input3.dtype)), input3)
        dtype = payload_dtype(input1, input3)
        if dtype == torch.float32:
            return _FilterInterpolationFunction.apply(cast(input1, dtype), cast(input2, dtype), cast(input3, dtype))
        return _FilterInterpolationLpFunction.apply(cast(input1, dtype), cast(input2, flow_dtype(input2, dtype)),
                                                    cast(input3, dtype))

    forward = __call__
