"""InterpolationLayer -- plain bilinear backward-warp, 3 channels only (my_lib_cuda.c:373).

Mirrors my_package/functions/InterpolationLayer.py of the reference (same class name and call surface:
`InterpolationLayer()(input1, input2)`, gradients for the image and the flow); see
FilterInterpolationLayer.py in this directory for the list of deliberate differences.

A float16 / bfloat16 image (a model cast to that dtype) beside a flow of that dtype or float32 has two routes, chosen by
the class switch `native_half`.  False: `_common.host_widened` -- the tensors are widened to float32 on the host, the
float32 Function runs and its results are cast back.  True: the half kernels of my_lib_lp_bl
(include/memc_warp_lp_bl.h) on the tensors as they are -- the forward reads and writes that dtype; autograd keeps the
image and the flow in their own dtypes, with no float32 copies; the backward reads gradoutput in that dtype, adds the image
gradient into a zero-filled float32 buffer that is cast afterwards, and writes the flow gradient in the flow's dtype.  The
output and the flow gradient are the same bits on both routes; the image gradient is the same sum in another order.  A
backward that the half kernel does not cover (return code 1: other channel counts than three, widths that are not a
multiple of four from 8 on) widens the saved tensors and runs the float32 backward, its results cast as host_widened casts
them.  Every other dtype pattern (a float32 image beside a half flow) takes host_widened; float32 calls take exactly the
old path.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import my_package._ext.my_lib as my_lib
import my_package._ext.my_lib_lp_bl as my_lib_lp_bl
from ._common import LOWP, check, declined, f32c, host_widened, require_gpu


def _make_bilinear_function(label, fwd_name, bwd_name):
    class _BilinearFunction(Function):
        @staticmethod
        def forward(ctx, input1, input2):
            require_gpu(label, input1, input2)
            input1, input2 = f32c(input1), f32c(input2)
            output = torch.empty_like(input1)     # reference zero-fills (:25); every element is written (invalid: 0)
            check(getattr(my_lib, fwd_name)(input1, input2, output), fwd_name)
            ctx.save_for_backward(input1, input2)
            return output

        @staticmethod
        @once_differentiable
        def backward(ctx, gradoutput):
            input1, input2 = ctx.saved_tensors
            gradoutput = f32c(gradoutput)
            # accumulation target, zero-filled (reference :40-41) -- except for four and more channels,
            # for which the library STORES it on every path (include/memc_warp.h)
            stored = my_lib.gradinput1_is_stored(0, input1.size(1))     # the library's own rule (include/memc_warp.h)
            gradinput1 = torch.empty_like(input1) if stored else torch.zeros_like(input1)
            gradinput2 = torch.empty_like(input2)               # assigned at every site (invalid: 0)
            check(getattr(my_lib, bwd_name)(input1, input2, gradoutput, gradinput1, gradinput2), bwd_name)
            return gradinput1, gradinput2

    _BilinearFunction.__name__ = "_%sFunction" % label
    return _BilinearFunction


def _make_bilinear_lp_function(label, fwd_name, bwd_name):
    """The Function of the half route: a float16 / bfloat16 image, a flow of that dtype or float32 (native_route)."""
    fwd_lp_name, bwd_lp_name = fwd_name + "_lp", bwd_name + "_lp"

    class _BilinearLpFunction(Function):
        @staticmethod
        def forward(ctx, input1, input2):
            require_gpu(label, input1, input2)
            if not native_route(input1, input2):
                raise TypeError("expected a float16 or bfloat16 image and a flow of that dtype or float32, got %s and %s"
                                % (input1.dtype, input2.dtype))
            input1, input2 = input1.contiguous(), input2.contiguous()
            output = torch.empty_like(input1)     # every element is written (invalid: 0)
            check(getattr(my_lib_lp_bl, fwd_lp_name)(input1, input2, output), fwd_lp_name)
            ctx.save_for_backward(input1, input2)       # as the network holds them: no float32 copy lives on
            return output

        @staticmethod
        @once_differentiable
        def backward(ctx, gradoutput):
            input1, input2 = ctx.saved_tensors
            gradoutput = gradoutput.contiguous()
            wide = torch.zeros_like(input1, dtype=torch.float32)    # the kernel's tiles add into it: float32, zeroed
            gradinput2 = torch.empty_like(input2)                   # assigned at every site (invalid: 0)
            err = getattr(my_lib_lp_bl, bwd_lp_name)(input1, input2, gradoutput, wide, gradinput2)
            if declined(err, bwd_lp_name):        # not covered: the widened route's arithmetic on the saved tensors
                stored = my_lib.gradinput1_is_stored(0, input1.size(1))
                if stored:
                    wide = torch.empty_like(wide)
                wide2 = torch.empty_like(input2, dtype=torch.float32)
                check(getattr(my_lib, bwd_name)(input1.float(), input2.float(), gradoutput.float(), wide, wide2), bwd_name)
                gradinput2 = wide2.to(input2.dtype)
            return wide.to(input1.dtype), gradinput2

    _BilinearLpFunction.__name__ = "_%sLpFunction" % label
    return _BilinearLpFunction


def native_route(input1, input2):
    """The dtype pattern of the half kernels: a float16 / bfloat16 image, a flow of that dtype or float32."""
    return input1.dtype in LOWP and input2.dtype in (torch.float32, input1.dtype)


_InterpolationFunction = _make_bilinear_function(
    "InterpolationLayer", "InterpolationLayer_gpu_forward", "InterpolationLayer_gpu_backward")
_InterpolationLpFunction = _make_bilinear_lp_function(
    "InterpolationLayer", "InterpolationLayer_gpu_forward", "InterpolationLayer_gpu_backward")


class InterpolationLayer(object):
    # float16 / bfloat16 images: True -- the half kernels (_InterpolationLpFunction); False -- host_widened, the float32
    # Function between casts.  Output and flow gradient are the same bits either way (tests/test_gpu_lp_bilinear.py).
    native_half = True

    def __init__(self):
        super(InterpolationLayer, self).__init__()

    def __call__(self, input1, input2):
        if self.native_half and native_route(input1, input2):
            return _InterpolationLpFunction.apply(input1, input2)
        return host_widened(_InterpolationFunction.apply, input1, input1, input2)     # fp16 / bf16: widened on the host

    forward = __call__
