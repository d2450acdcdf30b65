"""`FlowProjectionModule(requires_grad=True)(input1)` -- flow [B,2,H,W] projected to the middle frame; holes are
filled only when no gradient is wanted (the layer's `fillhole = not requires_grad` policy).  Surface of the
reference's module of this name.  A float16 / bfloat16 flow comes back in its dtype: the forward runs the float32 kernels
on the widened flow, the backward the half kernel of my_lib_lp_proj_grad while `FlowProjectionLayer.native_half_backward`
is on (functions/FlowProjectionLayer.py)."""
from ._operator_module import operator_module

FlowProjectionModule = operator_module("FlowProjectionModule", ("input1",), options=(("requires_grad", True),))
