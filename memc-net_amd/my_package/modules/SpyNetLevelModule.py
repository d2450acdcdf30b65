"""`SpyNetLevelModule(align_upsample, align_sample)(first, second, coarse)` -- EXTENSION (no reference module of this
name): the 8-channel input of one SPyNet pyramid level, [first, second warped with the upsampled and doubled coarser flow,
that flow] (functions/SpyNetLevelLayer.py).  Written out rather than made by `operator_module`: its constructor takes the
two `align_corners` flags."""
from torch.nn import Module

from my_package.functions.SpyNetLevelLayer import SpyNetLevelLayer


class SpyNetLevelModule(Module):
    def __init__(self, align_upsample=False, align_sample=False):
        super(SpyNetLevelModule, self).__init__()
        self.f = SpyNetLevelLayer(align_upsample, align_sample)

    def extra_repr(self):
        return "layer=%s, align_upsample=%s, align_sample=%s" % (type(self.f).__name__, self.f.align_upsample,
                                                                 self.f.align_sample)

    def forward(self, first, second, coarse):
        return self.f(first, second, coarse)
