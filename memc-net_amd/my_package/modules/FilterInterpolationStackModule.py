"""`FilterInterpolationStackModule()(out, input1, flow, taps, c_base, skip, flow_base=-1, tap_base=-1, detach=False)` --
EXTENSION (no reference module of this name): the warps of several neighbours, stacked on the batch axis, written into
channel slices of the caller's `out`, the flows and taps into slices of their own
(functions/FilterInterpolationStackLayer.py).  Written out rather than made by `operator_module`: its forward takes
ints and defaults beside its tensors."""
from torch.nn import Module

from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer


class FilterInterpolationStackModule(Module):
    def __init__(self):
        super(FilterInterpolationStackModule, self).__init__()
        self.f = FilterInterpolationStackLayer()

    def extra_repr(self):
        return "layer=%s" % type(self.f).__name__

    def forward(self, out, input1, flow, taps, c_base, skip, flow_base=-1, tap_base=-1, detach=False):
        return self.f(out, input1, flow, taps, c_base, skip, flow_base, tap_base, detach)
