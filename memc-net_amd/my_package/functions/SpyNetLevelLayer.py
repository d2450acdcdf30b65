"""SpyNetLevelLayer -- EXTENSION, no reference counterpart.

SPyNet, the flow estimator of `MEMC_Net_s`, refines its flow over up to six pyramid levels.  At each level the reference
(networks/SPyNet/Network.py:159-168, :120-134) upsamples the coarser flow x2 and doubles it, replicate-pads a row or column
where the level's size is odd, normalises the flow, adds a `linspace` grid, permutes, calls `grid_sample` on the second
frame and concatenates

    level_input = cat(first, second warped with the upsampled flow, upsampled flow)          [B, 8, H, W]

for the level's convolutions: nine or ten launches per level and direction, most of them on tiny tensors.  Here one launch
of libmemc_hip_spynet.so (include/memc_spynet.h) writes the eight channels.

    SpyNetLevelLayer(align_upsample, align_sample)(first, second, coarse) -> [B, 8, H, W]

with first, second [B, 3, H, W] and coarse [B, 2, h, w], H in {2h, 2h + 1}, W in {2w, 2w + 1}.  `align_upsample` is the
`align_corners` of the x2 upsampling, `align_sample` that of `grid_sample`: two flags because PyTorch 0.4.0 to 1.2 had
exactly the combination (False, True); the unmodified reference under a current PyTorch computes (False, False), the
PyTorch 0.2 its checkpoints were trained with (True, True).

The kernel serves inference in float32.  The torch expression (`_composed`, the exact composed route) runs instead
  * on CPU tensors, on other dtypes than float32 and under autocast,
  * where the library declines the call (planes beyond 32-bit offsets, a w-stride other than 1),
  * with the class attribute `fused` set to False,
  * whenever gradients are enabled and an input requires one: there is NO BACKWARD KERNEL -- such a call keeps torch's
    autograd through the composed route.  (In a training step of SPyNet that is every level but the coarsest: its frames
    are data and its coarse flow is zeros, no input wants a gradient, its output is constant with respect to the
    parameters, and it takes the kernel.)
Values: the upsampled flow and the copy of `first` equal the composed route's to within fp32 rounding (bit for bit where the
arithmetic is exact); the warp computes the sample position directly instead of through grid_sample's normalise /
un-normalise round trip, the same function to within fp32 rounding (tests/test_spynet_level_spec.py).
"""
import torch
import torch.nn.functional as F

import my_package._ext.my_lib_spynet as my_lib_spynet
from ._common import declined


def _composed(first, second, coarse, align_upsample, align_sample):
    """the reference's sequence, device- and dtype-agnostic, `align_corners` of both samplings explicit"""
    up = F.interpolate(coarse, scale_factor=2, mode="bilinear", align_corners=align_upsample) * 2.0
    if up.size(2) != first.size(2):
        up = F.pad(up, [0, 0, 0, 1], "replicate")
    if up.size(3) != first.size(3):
        up = F.pad(up, [0, 1, 0, 0], "replicate")
    b, _c, h, w = second.shape
    horizontal = torch.linspace(-1.0, 1.0, w, device=up.device, dtype=up.dtype).view(1, 1, 1, w).expand(b, 1, h, w)
    vertical = torch.linspace(-1.0, 1.0, h, device=up.device, dtype=up.dtype).view(1, 1, h, 1).expand(b, 1, h, w)
    grid = torch.cat([horizontal, vertical], 1)
    flow = torch.cat([up[:, 0:1] / ((w - 1.0) / 2.0), up[:, 1:2] / ((h - 1.0) / 2.0)], 1)
    warped = F.grid_sample(second, (grid + flow).permute(0, 2, 3, 1), mode="bilinear", padding_mode="zeros",
                           align_corners=align_sample)
    return torch.cat([first, warped, up], 1)


class SpyNetLevelLayer(object):
    """`SpyNetLevelLayer(align_upsample, align_sample)(first, second, coarse)` returns the level's [B, 8, H, W] input.
    Forward only: a call that needs gradients takes the torch expression and torch's autograd."""

    fused = True                                   # False: the torch expression for every call

    def __init__(self, align_upsample=False, align_sample=False):
        self.align_upsample, self.align_sample = bool(align_upsample), bool(align_sample)

    def _kernel_serves(self, tensors):
        if not self.fused or torch.is_autocast_enabled():
            return False
        if not all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 for t in tensors):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))

    def __call__(self, first, second, coarse):
        if self._kernel_serves((first, second, coarse)):
            out = first.new_empty((first.size(0), 8, first.size(2), first.size(3)))
            err = my_lib_spynet.SpyNetLevelLayer_gpu_forward(first, second, coarse, out, self.align_upsample,
                                                             self.align_sample)
            if not declined(err, "SpyNetLevelLayer_gpu_forward"):
                return out
        return _composed(first, second, coarse, self.align_upsample, self.align_sample)

    forward = __call__
