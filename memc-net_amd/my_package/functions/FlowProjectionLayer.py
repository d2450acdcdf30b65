"""FlowProjectionLayer -- forward-splat of -flow to the intermediate frame, count-normalised, optionally
hole-filled.

Mirrors my_package/functions/FlowProjectionLayer.py of the reference: `FlowProjectionLayer(requires_grad)`
then `layer(input1)`; `fillhole = 1 if requires_grad == False else 0` (:15), so holes are filled only at
inference; `count` is kept for backward (:37).  Deliberate differences as listed in
FilterInterpolationLayer.py of this directory.

A float16 / bfloat16 flow (a model cast to that dtype): the forward has no half kernel -- its hole filling reads
neighbours' results back, which a half output would round twice -- so the flow is widened, the float32 kernels run and the
result is cast back, the values `_common.host_widened` returns.  The backward is a pure gather and has one
(my_lib_lp_proj_grad, include/memc_warp_lp_proj_grad.h): `_FlowProjectionLpFunction` keeps the flow in its own dtype and
the float32 count, and its backward reads gradoutput and writes the gradient in that dtype -- bit for bit the widened
route's gradient, without its two cast passes and without a float32 copy of the flow held from forward to backward.
`FlowProjectionLayer.native_half_backward` chooses between the two routes.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import my_package._ext.my_lib as my_lib
import my_package._ext.my_lib_lp_proj_grad as my_lib_lp_proj_grad
from ._common import LOWP, check, declined, f32c, host_widened, require_gpu


class _FlowProjectionFunction(Function):
    @staticmethod
    def forward(ctx, input1, fillhole):
        require_gpu("FlowProjectionLayer", input1)
        input1 = f32c(input1)
        # the reference zero-fills both (:27-28); the forward pass here DEFINES every element of them on every
        # path (tests/test_gpu_parity.py::test_projection_forward_needs_no_zero_fill): no memsets
        count = input1.new_empty((input1.size(0), 1, input1.size(2), input1.size(3)))
        output = torch.empty_like(input1)
        # a workspace from torch's allocator instead of a block the library keeps (include/memc_warp.h, "EXTENSION:
        # workspace"): the call owns nothing afterwards and a HIP-graph capture records the same kernels as an eager call
        ws = my_lib.flow_projection_workspace(input1, fillhole)
        err = my_lib.FlowProjectionLayer_gpu_forward_ws(input1, count, output, int(fillhole), ws)
        check(err, "FlowProjectionLayer_gpu_forward_ws")
        ctx.save_for_backward(input1, count)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        input1, count = ctx.saved_tensors
        gradoutput = f32c(gradoutput)
        gradinput1 = torch.empty_like(input1)     # reference zero-fills (:54); the kernel stores every element
        err = my_lib.FlowProjectionLayer_gpu_backward(input1, count, gradoutput, gradinput1)
        check(err, "FlowProjectionLayer_gpu_backward")
        return gradinput1, None


class _FlowProjectionLpFunction(Function):
    """A float16 / bfloat16 flow: the float32 forward on the widened flow, its result cast back (host_widened's values); the
    half flow and the float32 count are what is kept, and the backward is the half kernel's."""

    @staticmethod
    def forward(ctx, input1, fillhole):
        require_gpu("FlowProjectionLayer", input1)
        if input1.dtype not in LOWP:
            raise TypeError("expected a float16 or bfloat16 tensor, got %s" % input1.dtype)
        input1 = input1.contiguous()
        wide = input1.float()
        count = wide.new_empty((wide.size(0), 1, wide.size(2), wide.size(3)))
        output = torch.empty_like(wide)
        ws = my_lib.flow_projection_workspace(wide, fillhole)
        err = my_lib.FlowProjectionLayer_gpu_forward_ws(wide, count, output, int(fillhole), ws)
        check(err, "FlowProjectionLayer_gpu_forward_ws")
        ctx.save_for_backward(input1, count)      # the flow as the network holds it: no float32 copy lives on
        return output.to(input1.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        input1, count = ctx.saved_tensors
        gradoutput = gradoutput.contiguous()
        gradinput1 = torch.empty_like(input1)     # the kernel stores every element
        err = my_lib_lp_proj_grad.FlowProjectionLayer_gpu_backward_lp(input1, count, gradoutput, gradinput1)
        if declined(err, "FlowProjectionLayer_gpu_backward_lp"):       # not covered: the widened route's arithmetic
            wide = torch.empty_like(input1, dtype=torch.float32)
            err = my_lib.FlowProjectionLayer_gpu_backward(input1.float(), count, gradoutput.float(), wide)
            check(err, "FlowProjectionLayer_gpu_backward")
            gradinput1 = wide.to(input1.dtype)
        return gradinput1, None


class FlowProjectionLayer(object):
    # float16 / bfloat16 flows: True -- the half backward kernel (_FlowProjectionLpFunction); False -- host_widened, the
    # float32 Function between two casts.  The gradients are the same bits either way (tests/test_gpu_lp_proj_grad.py).
    native_half_backward = True

    def __init__(self, requires_grad):
        super(FlowProjectionLayer, self).__init__()
        self.requires_grad = requires_grad

    def __call__(self, input1):
        self.fillhole = 1 if self.requires_grad == False else 0    # noqa: E712 -- as the reference, :15
        if input1.dtype in LOWP and self.native_half_backward:
            return _FlowProjectionLpFunction.apply(input1, self.fillhole)
        return host_widened(_FlowProjectionFunction.apply, input1, input1, self.fillhole)   # fp16 / bf16: widened

    forward = __call__
