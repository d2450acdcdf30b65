"""`DepthFlowProjectionModule(requires_grad=True)(input1, input2)` -- flow projection weighted by a depth map
[B,1,H,W].  The reference ships the C entry points (`DepthFlowProjectionLayer_*`, my_lib.h:92-108) but no Python
wrapper; this is that wrapper, with FlowProjectionModule's constructor.  A float16 / bfloat16 flow and depth of one dtype come
back in that dtype: the forward runs the float32 kernels on the widened tensors, the backward the half kernel of
my_lib_lp_dproj_grad while `DepthFlowProjectionLayer.native_half_backward` is on (functions/DepthFlowProjectionLayer.py)."""
from ._operator_module import operator_module

DepthFlowProjectionModule = operator_module("DepthFlowProjectionModule", ("input1", "input2"), options=(("requires_grad", True),))
