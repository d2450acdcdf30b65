"""InterpolationChLayer ("Interpolation_ch") -- plain bilinear backward-warp for any channel count.

The reference ships the C entry points (my_lib_cuda.h:53-68, my_lib.h:49-61) but no Python wrapper; this one
follows the pattern of its InterpolationLayer.py.  On the GPU both share one kernel
(my_lib_cuda.c:519,579).

A float16 / bfloat16 image beside a flow of that dtype or float32: the two routes of InterpolationLayer.py, chosen by the
class switch `native_half` -- the half kernels of my_lib_lp_bl on the tensors as they are (forward: any channel count;
backward: three channels, every other count widens the saved tensors and runs the float32 backward), or
`_common.host_widened`.
"""
from ._common import host_widened
from .InterpolationLayer import _make_bilinear_function, _make_bilinear_lp_function, native_route

_InterpolationChFunction = _make_bilinear_function(
    "InterpolationChLayer", "InterpolationChLayer_gpu_forward", "InterpolationChLayer_gpu_backward")
_InterpolationChLpFunction = _make_bilinear_lp_function(
    "InterpolationChLayer", "InterpolationChLayer_gpu_forward", "InterpolationChLayer_gpu_backward")


class InterpolationChLayer(object):
    # float16 / bfloat16 images: True -- the half kernels (_InterpolationChLpFunction); False -- host_widened
    native_half = True

    def __init__(self):
        super(InterpolationChLayer, self).__init__()

    def __call__(self, input1, input2):
        if self.native_half and native_route(input1, input2):
            return _InterpolationChLpFunction.apply(input1, input2)
        return host_widened(_InterpolationChFunction.apply, input1, input1, input2)   # fp16 / bf16: widened on the host

    forward = __call__
