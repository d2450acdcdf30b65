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

The forward kernel serves float32; with the class attribute `native_half` set, a second one (libmemc_hip_spynet_lp.so,
include/memc_spynet_lp.h) serves calls whose three tensors are all float16 or all bfloat16 -- see below.  The torch
expression (`_composed`, the exact composed route) runs instead
  * on CPU tensors, on other dtypes than float32 (half dtypes included while `native_half` is False) and under autocast,
  * where the library declines the call (planes beyond 32-bit offsets, a w-stride other than 1),
  * with the class attribute `fused` set to False,
  * whenever gradients are enabled and an input requires one -- such a call keeps torch's autograd through the composed
    route -- UNLESS `native_backward` is set and the gradient wanted is the one a training step of SPyNet needs: `coarse`
    requires one, `second` does not.  (In such a step that is every level but the coarsest: its frames are data and its
    coarse flow is zeros, no input wants a gradient, its output is constant with respect to the parameters, and it takes
    the forward kernel alone.)

The backward kernel (libmemc_hip_spynet_grad.so, include/memc_spynet_grad.h): with `native_backward = True` such a call goes
through a `torch.autograd.Function` whose forward is the forward kernel's call and whose backward is one launch for the
gradient of `coarse` -- frames that are data: no image gradient, no atomics, the same bits from run to run; the gradient of
`first` is gradoutput[:, 0:3], `second` gets none.  It saves `second` and `coarse`, not the output.  Where either library
declines, the Function composes: the forward returns `_composed`'s values, the backward recomputes `_composed` under
`enable_grad` and takes torch's gradient.  `native_backward` ships False (profiles/r27_spynet_level_backward.txt is what a
change of the default will rest on): a call where `second` requires a gradient, and every call while it is False, keep the
torch expression.
The half kernel: with `native_half = True` a call whose three tensors are CUDA, 4-D and of ONE half dtype T, outside
autocast and with no gradient wanted, allocates `out` in T and makes one launch of libmemc_hip_spynet_lp.so: the float32
kernel's arithmetic on the exactly widened inputs, every stored element rounded to T once -- bit for bit the float32 kernel
on the widened inputs followed by `.to(T)`.  Its values are NOT `_composed`'s on half tensors: the torch expression holds
the linspace grid, the normalised flow and their sum in T, so its sampling positions are rounded to T's grid (for bfloat16
about 0.9 px apart at a width of 448) before the warp; the kernel forms the position in float32 from the integer site index
and the unrounded upsampled flow.  That is why `native_half` ships False: it changes what a cast model computes, and
turning it on is a later decision that rests on profiles/r28_half_spynet_level.txt.  Half calls that want a gradient, mixed
dtypes and autocast keep the torch expression whatever it says; `native_backward` stays float32-only.
Values: the upsampled flow and the copy of `first` equal the composed route's to within fp32 rounding (bit for bit where the
arithmetic is exact); the warp computes the sample position directly instead of through grid_sample's normalise /
un-normalise round trip, the same function to within fp32 rounding (tests/test_spynet_level_spec.py).
"""
import torch
import torch.nn.functional as F

import my_package._ext.my_lib_spynet as my_lib_spynet
import my_package._ext.my_lib_spynet_grad as my_lib_spynet_grad
import my_package._ext.my_lib_spynet_lp as my_lib_spynet_lp
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


class _SpyNetLevelFunction(torch.autograd.Function):
    """The level input with the gradient of `coarse` by libmemc_hip_spynet_grad.so; `second` gets no gradient (the layer
    sends no call here whose `second` requires one)."""

    @staticmethod
    def forward(ctx, first, second, coarse, align_upsample, align_sample):
        ctx.flags = (align_upsample, align_sample)
        ctx.save_for_backward(second, coarse)
        out = first.new_empty((first.size(0), 8, first.size(2), first.size(3)))
        err = my_lib_spynet.SpyNetLevelLayer_gpu_forward(first, second, coarse, out, align_upsample, align_sample)
        if declined(err, "SpyNetLevelLayer_gpu_forward"):
            return _composed(first, second, coarse, align_upsample, align_sample)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gradoutput):
        second, coarse = ctx.saved_tensors
        gradfirst = gradoutput[:, 0:3] if ctx.needs_input_grad[0] else None
        gradcoarse = None
        if ctx.needs_input_grad[2]:
            if gradoutput.stride(3) != 1:              # sum().backward() hands over an expanded one
                gradoutput = gradoutput.contiguous()
            gradcoarse = torch.empty_like(coarse, memory_format=torch.contiguous_format)
            err = my_lib_spynet_grad.SpyNetLevelLayer_gpu_backward(second, coarse, gradoutput, gradcoarse, *ctx.flags)
            if declined(err, "SpyNetLevelLayer_gpu_backward"):
                with torch.enable_grad():
                    c = coarse.detach().requires_grad_(True)
                    first = torch.zeros_like(second)   # out[:, 0:3] is a copy: it carries nothing to `coarse`
                    gradcoarse, = torch.autograd.grad(_composed(first, second, c, *ctx.flags), c, gradoutput)
        return gradfirst, None, gradcoarse, None, None


class SpyNetLevelLayer(object):
    """`SpyNetLevelLayer(align_upsample, align_sample)(first, second, coarse)` returns the level's [B, 8, H, W] input.
    A call that needs gradients takes the torch expression and torch's autograd, unless `native_backward` is set and the
    gradient wanted is that of `coarse` (and of `first`) alone."""

    fused = True                                   # False: the torch expression for every call
    native_backward = False                        # True: the gradient of `coarse` by libmemc_hip_spynet_grad.so
    native_half = False                            # True: all-float16 / all-bfloat16 calls by libmemc_hip_spynet_lp.so

    def __init__(self, align_upsample=False, align_sample=False):
        self.align_upsample, self.align_sample = bool(align_upsample), bool(align_sample)

    def _kernel_serves(self, tensors):
        if not self.fused or torch.is_autocast_enabled():
            return False
        if not all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 for t in tensors):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))

    def _half_kernel_serves(self, tensors):
        if not (self.fused and self.native_half) or torch.is_autocast_enabled():
            return False
        dtype = tensors[0].dtype
        if dtype not in (torch.float16, torch.bfloat16):
            return False
        if not all(t.is_cuda and t.dtype == dtype and t.dim() == 4 for t in tensors):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))

    def _backward_kernel_serves(self, first, second, coarse):
        if not (self.fused and self.native_backward) or torch.is_autocast_enabled() or not torch.is_grad_enabled():
            return False
        if not all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 for t in (first, second, coarse)):
            return False
        return coarse.requires_grad and not second.requires_grad

    def __call__(self, first, second, coarse):
        if self._kernel_serves((first, second, coarse)):
            out = first.new_empty((first.size(0), 8, first.size(2), first.size(3)))
            err = my_lib_spynet.SpyNetLevelLayer_gpu_forward(first, second, coarse, out, self.align_upsample,
                                                             self.align_sample)
            if not declined(err, "SpyNetLevelLayer_gpu_forward"):
                return out
        elif self._half_kernel_serves((first, second, coarse)):
            out = first.new_empty((first.size(0), 8, first.size(2), first.size(3)))
            err = my_lib_spynet_lp.SpyNetLevelLayer_gpu_forward_lp(first, second, coarse, out, self.align_upsample,
                                                                   self.align_sample)
            if not declined(err, "SpyNetLevelLayer_gpu_forward_lp"):
                return out
        elif self._backward_kernel_serves(first, second, coarse):
            return _SpyNetLevelFunction.apply(first, second, coarse, self.align_upsample, self.align_sample)
        return _composed(first, second, coarse, self.align_upsample, self.align_sample)

    forward = __call__
