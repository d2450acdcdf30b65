"""`FilterInterpolationBlendModule()(input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1)` --
EXTENSION (no reference module of this name): the two adaptive warps of a frame pair and their occlusion-weighted
blend as one operator (functions/FilterInterpolationBlendLayer.py).  `fused_half_backward=True` (off by default): the backward
of a pure float16 / bfloat16 call runs one kernel of libmemc_hip_lp_blend_grad.so per direction whose image needs no gradient."""
from ._operator_module import operator_module

FilterInterpolationBlendModule = operator_module("FilterInterpolationBlendModule", ("input0", "input2", "flow0", "flow1", "filter0", "filter1", "occlusion0", "occlusion1"),
                                                 options=(("fused_half_backward", False),))
