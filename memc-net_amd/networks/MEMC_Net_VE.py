"""MEMC_Net_VE, build-owned: video enhancement (denoising, deblocking, super-resolution) of the centre frame of a septuplet.

Interface of the reference class (networks/MEMC_Net_VE.py:27-290): the constructor's keyword arguments as
demo_Vimeo_VE.py:40-42 passes them; `forward(inputs, y=None)` with `inputs` a list of seven [B, 3, H, W] frames (H, W
multiples of 64) and, when training, the ground truth `y` of the centre frame.  Inference returns the rectified centre
frame, or `(rectified, flow, filter)` under `debug`; training returns the seven residuals against `y` (the six warped
neighbours', the rectified centre's in place 3).  State-dict keys are the reference's, so its checkpoints load (checked in
tests/test_network_ve.py against vectors recorded from the reference class itself).

Per pass: FlowNetS and one U-Net (with batch norm, the reference's get_MonoNet5) estimate a flow and a 4 x 4 filter from
(centre, neighbour) for each of the six neighbours, stacked on the batch axis; each neighbour and its 64-channel context
are warped towards the centre; the rectifier reads, in this channel order,

    7 x 64 context (0..447) | 6 x 2 flow (448..459) | 6 x 16 taps (460..555) | 7 x 3 frames (556..576)

(the centre's context and frame unwarped in slot 3) and its output is added to the centre frame.

Differences, deliberate:
  * no file I/O in the constructor (the reference loads "models/flownets_pytorch.pth" when training=True and downloads
    ResNet-18, :85,:94); use `load_state_dict`;
  * `align_corners` of the bilinear upsamplings is a constructor argument, as on the other classes (networks/_base.py);
  * `fused_stack`: the rectifier input is allocated once and filled by two stacked warps
    (my_package.modules.FilterInterpolationStackModule, an extension of this repository's my_package) instead of twelve
    FilterInterpolationModule calls and torch.cat.  Same values bit for bit (tests/test_gpu_stack.py; a model cast to
    float16 / bfloat16: tests/test_gpu_lp_stack.py).
"""
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from my_package.modules.FilterInterpolationModule import FilterInterpolationModule
try:        # extension of this repository's my_package; absent from the reference's
    from my_package.modules.FilterInterpolationStackModule import FilterInterpolationStackModule
except ImportError:
    FilterInterpolationStackModule = None

from ._blocks import ContextConv, FlowEstimator, Rectifier, run_unet, unet_head, unet_trunk

N_FRAMES, CENTRE = 7, 3


class MEMC_Net_VE(nn.Module):
    div_flow = 20                                      # FlowNetS predicts flow / 20

    def __init__(self, batch=128, channel=3, width=100, height=100, scale_num=3, scale_ratio=2, temporal=False,
                 filter_size=4, offset_scale=1, save_which=0, debug=False, cuda_available=False, cuda_id=0, training=True,
                 align_corners=False):
        super().__init__()
        self.scale_num, self.scale_ratio = scale_num, scale_ratio
        self.filter_size = filter_size
        self.cuda_available, self.cuda_id = cuda_available, cuda_id
        self.offset_scale = offset_scale
        self.training = training
        self.align_corners = align_corners
        self.save_which, self.debug = save_which, debug
        # the rectifier input filled by two stacked warps instead of twelve warps and torch.cat: measured x0.37 / x0.39 of
        # the composed route's time (314 against 845 us, 904 against 2305 us: 1 / 4 septuplets of 320 x 512,
        # profiles/r24_ve_stack.txt), faster in both groups, so on by default; a whole inference step x0.97 (21.3 against
        # 21.9 ms): the dense layers dominate.  On the GPU, for float32 and for a model cast to float16 / bfloat16
        # (FilterInterpolationStackLayer.native_half has that route's numbers); autocast and mixed dtypes take the composed
        # route whatever this says
        self.fused_stack = True
        fs2 = filter_size * filter_size
        self.ctx_ch = 64
        self.initScaleNets_filter = unet_trunk(2 * channel, align_corners, batch_norm=True)
        self.initScaleNets_filter1 = unet_head(fs2)
        self.rectifyNet = Rectifier(N_FRAMES * channel + N_FRAMES * self.ctx_ch + (N_FRAMES - 1) * (2 + fs2),
                                    blocks=10, feats=128)
        self._initialize_weights()                     # reference :80, :106-124
        self.flownets = FlowEstimator()                # these two keep their own initialisation
        self.ctxNet = ContextConv()

    def load_state_dict(self, state_dict, *args, **kwargs):
        """Warns once where published (PyTorch 0.2, align_corners=True semantics) weights may be going into a model built
        with align_corners=False: see MEMCNetBase.load_state_dict; silenced the same way."""
        warn = kwargs.pop("warn_align_corners", getattr(self, "warn_align_corners", True))
        if warn and not self.align_corners and not getattr(self, "_warned_align_corners", False):
            self._warned_align_corners = True
            warnings.warn("%s was built with align_corners=False; checkpoints published with MEMC-Net were trained with "
                          "PyTorch 0.2 (align_corners=True semantics): construct the model with align_corners=True to "
                          "reproduce their results." % type(self).__name__, stacklevel=2)
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
    def _flow(self, pairs):
        """quarter-resolution flow centre -> neighbour, at full resolution (no halving, no projection: :292-296)"""
        return F.interpolate(self.div_flow * self.flownets(pairs), scale_factor=4, mode="bilinear",
                             align_corners=self.align_corners)

    def _estimate(self, inputs):
        """(flow [6B, 2, H, W], taps [6B, 16, H, W]) of the six neighbours, neighbour-major: row n * B + b"""
        pairs = torch.cat([torch.cat((inputs[CENTRE], inputs[i]), dim=1) for i in range(N_FRAMES) if i != CENTRE], dim=0)
        return self._flow(pairs), run_unet(self.initScaleNets_filter1, run_unet(self.initScaleNets_filter, pairs))

    def _use_stack(self, inputs, flow, taps):
        # one dtype throughout -- float32, or float16 / bfloat16 for a cast model -- and no autocast (under it torch.cat
        # promotes the rectifier input to float32 while the warps stay half: the composed route's business)
        dtype = flow.dtype
        return (self.fused_stack and FilterInterpolationStackModule is not None and not torch.is_autocast_enabled()
                and dtype in (torch.float32, torch.float16, torch.bfloat16)
                and all(t.is_cuda and t.dtype == dtype for t in tuple(inputs) + (flow, taps))
                and self.ctxNet.conv1.weight.dtype == dtype)

    def _rectifier_input_composed(self, inputs, flow, taps, contexts=None):
        """twelve warps and torch.cat: the reference's sequence (:205-256; tests/golden/ve_call_trace.json)"""
        batch = inputs[0].size(0)
        context = (lambda i: contexts[i]) if contexts is not None else (lambda i: self.ctxNet(inputs[i]))
        warped, warped_ctx = [], []
        for i in range(N_FRAMES):
            if i == CENTRE:
                warped.append(inputs[CENTRE])
                warped_ctx.append(context(CENTRE))
                continue
            rows = slice((i - (i > CENTRE)) * batch, (i - (i > CENTRE) + 1) * batch)
            warped.append(FilterInterpolationModule()(inputs[i], flow[rows], taps[rows]))
            warped_ctx.append(FilterInterpolationModule()(context(i), flow[rows], taps[rows]).detach())
        nbrs = [slice(n * batch, (n + 1) * batch) for n in range(N_FRAMES - 1)]
        flow_taps = torch.cat([flow[r] for r in nbrs] + [taps[r] for r in nbrs], dim=1)
        return torch.cat((torch.cat(warped_ctx, dim=1), flow_taps, torch.cat(warped, dim=1)), dim=1), warped

    def _rectifier_input_stacked(self, inputs, flow, taps, contexts=None):
        """the same tensor, allocated once: ctxNet on the seven frames in one batch (the neighbours first, so that they
        are one view), two stacked warps (the contexts without gradient, the frames with the flow and tap pass-through),
        the centre's context and frame copied in"""
        batch, channel, ctx = inputs[0].size(0), inputs[0].size(1), self.ctx_ch
        order = [i for i in range(N_FRAMES) if i != CENTRE] + [CENTRE]
        nbr_rows = (N_FRAMES - 1) * batch
        frames = torch.cat([inputs[i] for i in order], dim=0)
        if contexts is None:
            feats = self.ctxNet(frames)
        elif torch.is_tensor(contexts):                   # stacked already: the six neighbours' rows, then the centre's
            feats = contexts
        else:
            feats = torch.cat([contexts[i] for i in order], dim=0)
        flow_base = N_FRAMES * ctx
        tap_base = flow_base + 2 * (N_FRAMES - 1)
        frame_base = tap_base + taps.size(1) * (N_FRAMES - 1)
        out = frames.new_empty((batch, frame_base + N_FRAMES * channel) + tuple(frames.shape[2:]))
        stack = FilterInterpolationStackModule()
        out = stack(out, feats[:nbr_rows], flow, taps, 0, CENTRE, detach=True)
        out = stack(out, frames[:nbr_rows], flow, taps, frame_base, CENTRE, flow_base, tap_base)
        out[:, CENTRE * ctx:(CENTRE + 1) * ctx] = feats[nbr_rows:]
        out[:, frame_base + CENTRE * channel:frame_base + (CENTRE + 1) * channel] = inputs[CENTRE]
        warped = [inputs[CENTRE] if i == CENTRE else
                  out[:, frame_base + i * channel:frame_base + (i + 1) * channel] for i in range(N_FRAMES)]
        return out, warped

    def _rectifier_input(self, inputs, flow, taps, contexts=None):
        if self._use_stack(inputs, flow, taps):
            return self._rectifier_input_stacked(inputs, flow, taps, contexts)
        return self._rectifier_input_composed(inputs, flow, taps, contexts)

    def rectifier_input(self, inputs, flow=None, taps=None, contexts=None):
        """The [B, 577, H, W] tensor the rectifier reads for these seven frames, by the route `fused_stack` selects.  `flow`
        and `taps` ([6B, ...], neighbour-major) and `contexts` (seven [B, 64, H, W]) replace what the sub-networks would
        estimate: dense convolutions need not give the same bits twice, and with these handed in the two routes can be
        compared bit for bit."""
        if flow is None or taps is None:
            flow, taps = self._estimate(inputs)
        return self._rectifier_input(inputs, flow, taps, contexts)[0]

    # ---- forward ----------------------------------------------------------------------------------------
    def forward(self, inputs, y=None):
        assert len(inputs) == N_FRAMES
        flow, taps = self._estimate(inputs)
        rect_in, warped = self._rectifier_input(inputs, flow, taps)
        rectified = inputs[CENTRE] + self.rectifyNet(rect_in)
        if self.training:
            return [(rectified if i == CENTRE else warped[i]) - y for i in range(N_FRAMES)]
        if not self.debug:
            return rectified
        return rectified, flow, taps
