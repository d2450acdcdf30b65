"""DepthFlowProjectionLayer -- FlowProjection weighted by a per-pixel depth map.

The reference ships the C entry points (my_lib_cuda.h:101-117, my_lib.h:92-108) but no Python wrapper; this
one follows the pattern of its FlowProjectionLayer.py: `DepthFlowProjectionLayer(requires_grad)` then
`layer(input1, input2)` with input1 = flow [N,2,H,W], input2 = depth [N,1,H,W];
`fillhole = 1 if requires_grad == False else 0`.  Backward needs the forward output (my_lib.c:1844-1869),
which is therefore saved together with `count`.

A float16 / bfloat16 flow and depth (a model cast to that dtype): the forward has no half kernel -- its hole filling reads
neighbours' results back, which a half output would round twice -- so flow and depth are widened, the float32 kernels run
and the result is cast back, the values `_common.host_widened` returns.  The backward is a pure gather and has one
(my_lib_lp_dproj_grad, include/memc_warp_lp_dproj_grad.h): `_DepthFlowProjectionLpFunction` keeps the flow and the depth in
their own dtype beside the float32 count and the float32 output, and its backward reads gradoutput and writes both
gradients in that dtype -- bit for bit the widened route's gradients, without its three cast passes and without float32
copies of flow and depth held from forward to backward.  `DepthFlowProjectionLayer.native_half_backward` chooses between
the two routes; a half flow beside a float32 depth (or the other way round) and float32 calls take the old one.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import my_package._ext.my_lib as my_lib
import my_package._ext.my_lib_lp_dproj_grad as my_lib_lp_dproj_grad
from ._common import LOWP, check, declined, f32c, host_widened, require_gpu


class _DepthFlowProjectionFunction(Function):
    @staticmethod
    def forward(ctx, input1, input2, fillhole):
        require_gpu("DepthFlowProjectionLayer", input1, input2)
        input1, input2 = f32c(input1), f32c(input2)
        count = input1.new_empty((input1.size(0), 1, input1.size(2), input1.size(3)))   # defined by the forward pass
        output = torch.empty_like(input1)                                               # (see FlowProjectionLayer)
        # a workspace from torch's allocator instead of a block the library keeps (include/memc_warp.h, "EXTENSION:
        # workspace"): the call owns nothing afterwards and a HIP-graph capture records the same kernels as an eager call
        ws = my_lib.flow_projection_workspace(input1, fillhole, depth=True)
        err = my_lib.DepthFlowProjectionLayer_gpu_forward_ws(input1, input2, count, output, int(fillhole), ws)
        check(err, "DepthFlowProjectionLayer_gpu_forward_ws")
        ctx.save_for_backward(input1, input2, count, output)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        input1, input2, count, output = ctx.saved_tensors
        gradoutput = f32c(gradoutput)
        gradinput1 = torch.empty_like(input1)     # stored by the kernel, element by element (see FlowProjectionLayer)
        gradinput2 = torch.empty_like(input2)
        err = my_lib.DepthFlowProjectionLayer_gpu_backward(
            input1, input2, count, output, gradoutput, gradinput1, gradinput2)
        check(err, "DepthFlowProjectionLayer_gpu_backward")
        return gradinput1, gradinput2, None


class _DepthFlowProjectionLpFunction(Function):
    """A float16 / bfloat16 flow and depth: the float32 forward on the widened tensors, its result cast back
    (host_widened's values); the half flow, the half depth, the float32 count and the float32 output are what is kept, and
    the backward is the half kernel's."""

    @staticmethod
    def forward(ctx, input1, input2, fillhole):
        require_gpu("DepthFlowProjectionLayer", input1, input2)
        if input1.dtype not in LOWP or input2.dtype != input1.dtype:
            raise TypeError("expected a flow and a depth of one dtype, float16 or bfloat16, got %s and %s"
                            % (input1.dtype, input2.dtype))
        input1, input2 = input1.contiguous(), input2.contiguous()
        wide1, wide2 = input1.float(), input2.float()
        count = wide1.new_empty((wide1.size(0), 1, wide1.size(2), wide1.size(3)))
        output = torch.empty_like(wide1)
        ws = my_lib.flow_projection_workspace(wide1, fillhole, depth=True)
        err = my_lib.DepthFlowProjectionLayer_gpu_forward_ws(wide1, wide2, count, output, int(fillhole), ws)
        check(err, "DepthFlowProjectionLayer_gpu_forward_ws")
        ctx.save_for_backward(input1, input2, count, output)   # flow and depth as the network holds them: no float32 copy
        return output.to(input1.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        input1, input2, count, output = ctx.saved_tensors
        gradoutput = gradoutput.contiguous()
        gradinput1 = torch.empty_like(input1)     # the kernel stores every element of both
        gradinput2 = torch.empty_like(input2)
        err = my_lib_lp_dproj_grad.DepthFlowProjectionLayer_gpu_backward_lp(
            input1, input2, count, output, gradoutput, gradinput1, gradinput2)
        if declined(err, "DepthFlowProjectionLayer_gpu_backward_lp"):  # not covered: the widened route's arithmetic
            wide1 = torch.empty_like(input1, dtype=torch.float32)
            wide2 = torch.empty_like(input2, dtype=torch.float32)
            err = my_lib.DepthFlowProjectionLayer_gpu_backward(
                input1.float(), input2.float(), count, output, gradoutput.float(), wide1, wide2)
            check(err, "DepthFlowProjectionLayer_gpu_backward")
            gradinput1, gradinput2 = wide1.to(input1.dtype), wide2.to(input2.dtype)
        return gradinput1, gradinput2, None


class DepthFlowProjectionLayer(object):
    # a float16 / bfloat16 flow and depth of one dtype: True -- the half backward kernel (_DepthFlowProjectionLpFunction);
    # False -- host_widened, the float32 Function between casts.  The gradients are the same bits either way
    # (tests/test_gpu_lp_dproj_grad.py).  Set by profiles/r23_half_depth_projection_backward.txt.
    native_half_backward = True

    def __init__(self, requires_grad):
        super(DepthFlowProjectionLayer, self).__init__()
        self.requires_grad = requires_grad

    def __call__(self, input1, input2):
        self.fillhole = 1 if self.requires_grad == False else 0    # noqa: E712
        if self.native_half_backward and input1.dtype in LOWP and input2.dtype == input1.dtype:
            return _DepthFlowProjectionLpFunction.apply(input1, input2, self.fillhole)
        return host_widened(_DepthFlowProjectionFunction.apply, input1, input1, input2, self.fillhole)   # fp16 / bf16: widened

    forward = __call__
