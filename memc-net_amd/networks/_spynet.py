"""SPyNet, the spatial-pyramid flow estimator of MEMC_Net_s, build-owned.

Interface and state-dict keys of the reference's `networks.SPyNet.Network` (networks/SPyNet/Network.py:57-172):
`forward(first, second)` returns the flow first -> second at the frames' resolution; six stacks of five 7 x 7 convolutions,
`moduleBasic.{0..5}.moduleBasic.{0,2,4,6,8}.{weight,bias}`, of which a pyramid of L levels uses the first L.

Per pass: both frames are normalised (`Preprocess`, with its channel flip) and average-pooled x2 while a side exceeds 32,
five times at most; from a zero flow of half the coarsest level's size (floored), each level upsamples and doubles the
flow, warps the second frame with it, runs its stack on [first, warped second, upsampled flow] and adds the upsampled flow.

Differences, deliberate:
  * device-agnostic: no `.cuda()`, no `Variable`, no grid cached on a fixed device;
  * reads no files: `training=True` does not look for `.t7` weights (torch.utils.serialization is gone from PyTorch) and the
    convolutions keep torch's default initialisation, which is what they have in the reference's MEMC_Net_s too
    (`_initialize_weights` runs before `flownets` exists, networks/MEMC_Net_s.py:31-34); use `load_state_dict`;
  * `align_upsample` / `align_sample`: the `align_corners` of the x2 upsampling and of `grid_sample`, explicit;
  * `fused_level`: a level's 8-channel input by one kernel (my_package.modules.SpyNetLevelModule, an extension of this
    repository's my_package) instead of nine or ten ATen launches, where that kernel serves the call: float32 CUDA tensors,
    no autocast, no gradient wanted;
  * `fused_level_backward`: in a training step, where a level's coarse flow wants a gradient and its frames are data, the
    level input through the same layer's autograd Function -- the forward kernel, and one backward kernel for the gradient
    of the coarse flow (libmemc_hip_spynet_grad.so) instead of torch's autograd through the torch expression.  Off by
    default;
  * `fused_level_half`: in a model cast to bfloat16 / float16, a level's input by the half-precision kernel
    (libmemc_hip_spynet_lp.so) where all three tensors are of one half dtype, autocast is off and no gradient is wanted,
    instead of the torch expression on half tensors.  Off by default: it changes the values a cast model computes (the
    kernel forms the sampling position in float32; the torch expression rounds its grid and flow to the half dtype first).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

try:        # extension of this repository's my_package; absent from the reference's
    from my_package.modules.SpyNetLevelModule import SpyNetLevelModule
except ImportError:
    SpyNetLevelModule = None

LEVELS = 6


class _Basic(nn.Module):
    def __init__(self):
        super().__init__()
        chans = (8, 32, 64, 32, 16, 2)
        mods = []
        for i in range(5):
            mods.append(nn.Conv2d(chans[i], chans[i + 1], kernel_size=7, stride=1, padding=3))
            if i < 4:
                mods.append(nn.ReLU(inplace=False))
        self.moduleBasic = nn.Sequential(*mods)

    def forward(self, x):
        return self.moduleBasic(x)


def preprocess(x):
    """Network.py:66-75: per-channel mean and deviation, then the channel order reversed"""
    blue = (x[:, 0:1] - 0.406) / 0.225
    green = (x[:, 1:2] - 0.456) / 0.224
    red = (x[:, 2:3] - 0.485) / 0.229
    return torch.cat([red, green, blue], 1)


def level_input_composed(first, second, coarse, align_upsample, align_sample):
    """Network.py:160-167 with :120-134 inlined: cat(first, second warped with the upsampled flow, upsampled flow).
    A copy of my_package.functions.SpyNetLevelLayer._composed, which is what runs wherever that layer exists; this one is
    reached only on a my_package WITHOUT the extension -- the reference's own, and the CPU stand-in that the network tests
    put in its place, neither of which has a `functions.SpyNetLevelLayer` to import it from.
    tests/test_gpu_network_s.py holds the two to the same bits."""
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


class SPyNet(nn.Module):
    def __init__(self, training=False, align_upsample=False, align_sample=False):
        super().__init__()
        self.align_upsample, self.align_sample = align_upsample, align_sample
        # a level's input by one kernel instead of the torch expression.  Measured (profiles/r26_spynet_level.txt, one MI355X,
        # batch 1, allocations included, routes alternating over seven rounds): x0.32 to x0.41 of the composed route's time at
        # every level but the largest (24 to 30 us against 69 to 75 us: the composed route is bound by its ten launches), x0.66
        # at 768 x 1344 (73 against 111 us); the whole SPyNet forward x0.90 at 256 x 448 (2133 against 2384 us) and x0.96 at
        # 768 x 1344 (9782 against 10175 us): the 7 x 7 convolutions dominate.  Faster by more than the larger spread in all
        # thirteen groups, so on by default.  Levels whose inputs want a gradient (in a training step: every level but
        # the coarsest, whose frames and zero flow want none), autocast and other dtypes than float32 take the torch
        # expression whatever this says
        self.fused_level = True
        # the gradient of a level's coarse flow by one kernel (my_package.functions.SpyNetLevelLayer.native_backward) instead
        # of torch's autograd through the torch expression.  Ships off whatever profiles/r27_spynet_level_backward.txt says:
        # the default training route is the one the existing tests pin
        self.fused_level_backward = False
        # a cast model's level input by the half kernel (my_package.functions.SpyNetLevelLayer.native_half) instead of the
        # torch expression on half tensors.  Ships off whatever profiles/r28_half_spynet_level.txt says: the kernel changes
        # the values a cast model computes (its sampling position is float32, not rounded to the half dtype)
        self.fused_level_half = False
        self.moduleBasic = nn.ModuleList([_Basic() for _ in range(LEVELS)])

    def level_input(self, first, second, coarse):
        """The [B, 8, H, W] input of one level's convolutions, by the route `fused_level` selects: the only place it is made.
        With my_package's extension it is the layer's business either way (its kernel, or its own torch expression for CPU
        tensors, other dtypes, autocast, declined calls, inputs that want a gradient and `fused_level = False`; with
        `fused_level_backward` its backward kernel where only the coarse flow wants a gradient, with `fused_level_half`
        its half kernel where all three tensors are of one half dtype)."""
        if SpyNetLevelModule is not None:
            level = SpyNetLevelModule(self.align_upsample, self.align_sample)
            level.f.fused = bool(self.fused_level)
            level.f.native_backward = bool(self.fused_level_backward)
            level.f.native_half = bool(self.fused_level_half)
            return level(first, second, coarse)
        return level_input_composed(first, second, coarse, self.align_upsample, self.align_sample)

    def pyramid(self, first, second):
        """the two preprocessed frames at every level, coarsest first (Network.py:147-155)"""
        first, second = [preprocess(first)], [preprocess(second)]
        for _ in range(LEVELS - 1):
            if first[0].size(2) > 32 or first[0].size(3) > 32:
                first.insert(0, F.avg_pool2d(first[0], kernel_size=2, stride=2))
                second.insert(0, F.avg_pool2d(second[0], kernel_size=2, stride=2))
        return first, second

    def forward(self, first, second):
        first, second = self.pyramid(first, second)
        flow = first[0].new_zeros((first[0].size(0), 2, first[0].size(2) // 2, first[0].size(3) // 2))
        for level in range(len(first)):
            x = self.level_input(first[level], second[level], flow)
            flow = self.moduleBasic[level](x) + x[:, 6:8]
        return flow
