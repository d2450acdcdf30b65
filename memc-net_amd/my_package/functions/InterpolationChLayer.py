"""InterpolationChLayer ("Interpolation_ch") -- plain bilinear backward-warp for any channel count.

The reference ships the C entry points (my_lib_cuda.h:53-68, my_lib.h:49-61) but no Python wrapper; this one
follows the pattern of its InterpolationLayer.py.  On the GPU both share one kernel
(my_lib_cuda.c:519,579).
"""
from ._common import host_widened
from .InterpolationLayer import _make_bilinear_function

_InterpolationChFunction = _make_bilinear_function(
    "InterpolationChLayer", "InterpolationChLayer_gpu_forward", "InterpolationChLayer_gpu_backward")


class InterpolationChLayer(object):
    def __init__(self):
        super(InterpolationChLayer, self).__init__()

    def __call__(self, input1, input2):
        return host_widened(_InterpolationChFunction.apply, input1, input1, input2)   # fp16 / bf16: widened on the host

    forward = __call__
