"""`InterpolationChModule()(input1, input2)` -- bilinear warp, any channel count. The reference ships the C entry points
(`InterpolationChLayer_*`, my_lib.h:49-61) but no Python wrapper for them; this is that wrapper. A float16 / bfloat16
image beside a flow of that dtype or float32 comes back in its dtype: the half kernels of my_lib_lp_bl run on the
tensors as they are while the layer's `native_half` is on (functions/InterpolationChLayer.py)."""
from ._operator_module import operator_module

InterpolationChModule = operator_module("InterpolationChModule", ("input1", "input2"))
