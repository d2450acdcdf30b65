"""MEMC_Net_s (the small model of the paper, the one the reference's Middlebury demo documents), build-owned.

Interface and state-dict keys of the reference class (networks/MEMC_Net_s.py:12-325): `forward(input)` with `input`
[3, B, 3, H, W] when training (frame0, ground truth, frame2) or [2, B, 3, H, W] at inference (H, W multiples of 32), the
four return values of the sibling classes.  State-dict keys are the reference's, so its checkpoints load (checked in
tests/test_network_s.py against vectors recorded from the reference class itself).

Per pass: SPyNet (networks/_spynet.py) estimates the flow in both directions at full resolution, which is halved
(`div_flow` is 1 and nothing is upsampled) and projected to t = 0.5; ONE U-Net with batch norm (the reference's lighter
get_MonoNet5: a convolution per stage) and two heads estimates the 4 x 4 filters; there are no occlusion networks -- both
"occlusions" are the first filter plane of direction 0 -- and the two adaptive warps are averaged; the plain 8-convolution
rectifier (`get_RectifyNet2(41, 3)`, a flat ModuleList: `rectifyNet.0.weight` ... `rectifyNet.14.weight`) reads

    blended 3 | flows 2 x 2 | filters 2 x 16 | occlusions 2 x 1

and its output is added to the blended frame.

Differences, deliberate:
  * no file I/O in the constructor (the reference's SPyNet loads `.t7` weights through torch.utils.serialization when
    training=True); use `load_state_dict`;
  * `align_corners` is a constructor argument, as on the other classes (networks/_base.py): it sets the U-Net's bilinear
    upsamplings and both samplings of SPyNet's pyramid levels (the x2 flow upsampling and `grid_sample`).
"""
import warnings

import torch
import torch.nn as nn

from my_package.modules.FilterInterpolationModule import FilterInterpolationModule
from my_package.modules.FlowProjectionModule import FlowProjectionModule

from ._blocks import TRUNK_S, run_unet, unet_head, unet_trunk
from ._spynet import SPyNet


class MEMC_Net_s(nn.Module):
    div_flow = 1                                       # no scaling is used in SPyNet

    def __init__(self, channel=3, filter_size=4, training=True, align_corners=False):
        super().__init__()
        self.filter_size = filter_size
        self.training = training
        self.align_corners = align_corners
        fs2 = filter_size * filter_size
        self.initScaleNets_filter = unet_trunk(2 * channel, align_corners, tokens=TRUNK_S)
        self.initScaleNets_filter1 = unet_head(fs2)
        self.initScaleNets_filter2 = unet_head(fs2)
        mods, ch = [], channel + 2 * 2 + 2 * fs2 + 2 * 1            # 3 + 4 + 32 + 2
        for _ in range(7):
            mods += [nn.Conv2d(ch, 64, (3, 3), 1, (1, 1)), nn.ReLU(inplace=False)]
            ch = 64
        mods.append(nn.Conv2d(64, channel, (3, 3), 1, (1, 1)))
        self.rectifyNet = nn.ModuleList(mods)
        self._initialize_weights()                     # reference :31, before SPyNet exists (:34)
        self.flownets = SPyNet(training, align_upsample=align_corners, align_sample=align_corners)

    def load_state_dict(self, state_dict, *args, **kwargs):
        """Warns once where published (PyTorch 0.2, align_corners=True semantics) weights may be going into a model built
        with align_corners=False: see MEMCNetBase.load_state_dict; silenced the same way."""
        warn = kwargs.pop("warn_align_corners", getattr(self, "warn_align_corners", True))
        if warn and not self.align_corners and not getattr(self, "_warned_align_corners", False):
            self._warned_align_corners = True
            warnings.warn("%s was built with align_corners=False (what the reference's code does under current "
                          "PyTorch).  Checkpoints published with MEMC-Net were trained with PyTorch 0.2 "
                          "(align_corners=True semantics): construct the model with align_corners=True to reproduce "
                          "their results." % type(self).__name__, stacklevel=2)
        return super().load_state_dict(state_dict, *args, **kwargs)

    def _initialize_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight.data, a=0, mode="fan_in")
                if m.bias is not None:
                    m.bias.data.zero_()
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    # ---- pieces -----------------------------------------------------------------------------------------
    def _projected_flow(self, first, second):
        """full-resolution single-direction flow, halved for the middle frame (:153-154), projected to t = 0.5"""
        flow = self.flownets(first, second) / 2.0
        # holes are filled only when no gradient is needed (FlowProjectionLayer.py:15)
        return FlowProjectionModule(flow.requires_grad)(flow)

    def _rectify(self, x):
        for m in self.rectifyNet:
            x = m(x)
        return x

    # ---- forward ----------------------------------------------------------------------------------------
    def forward(self, input):
        if self.training:
            assert input.size(0) == 3
            frame0, frame1, frame2 = input[0], input[1], input[2]
        else:
            assert input.size(0) == 2
            frame0, frame2 = input[0], input[1]
        both = torch.cat((frame0, frame2), dim=1)

        flows = [self._projected_flow(frame0, frame2), self._projected_flow(frame2, frame0)]
        feat = run_unet(self.initScaleNets_filter, both)
        filters = [run_unet(self.initScaleNets_filter1, feat), run_unet(self.initScaleNets_filter2, feat)]
        occlusions = [filters[0][:, :1], filters[0][:, :1]]

        warp = FilterInterpolationModule()
        blended = warp(frame0, flows[0], filters[0]) / 2.0 + warp(frame2, flows[1], filters[1]) / 2.0

        rect_in = torch.cat((blended, flows[0], flows[1], filters[0], filters[1], occlusions[0], occlusions[1]), dim=1)
        rectified = blended + self._rectify(rect_in)

        if self.training:
            return [blended - frame1, rectified - frame1], [flows], [filters], [occlusions]
        return [blended, rectified], flows, filters, occlusions
