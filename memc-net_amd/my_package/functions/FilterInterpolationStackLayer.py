"""FilterInterpolationStackLayer -- EXTENSION, no reference counterpart.

`MEMC_Net_VE` warps the six neighbours of a septuplet's centre frame, and their 64-channel context features, with the
flow and the 16 filter planes estimated for each neighbour, and concatenates everything into the rectifier's input
(networks/MEMC_Net_VE.py:205-256 of the reference):

    rectify_input = cat(warped contexts (centre unwarped), flows, filters, warped frames (centre unwarped))

As twelve FilterInterpolation launches and a torch.cat every warped value is written, read and written again, and the
flows and taps are read a second time for the concatenation: about 1360 B per site and neighbour.  Here one launch warps
all neighbours of one kind -- stacked on the batch axis, row n * B + b -- straight into their channel slices of the
caller's tensor and stores the flow and taps it has loaded to theirs: about 752 B.

    layer(out, input1, flow, taps, c_base, skip, flow_base=-1, tap_base=-1, detach=False) -> out

    out[b, c_base + slot(n) * C + c] = FI(input1, flow, taps)[n * B + b, c],   slot(n) = n + (skip >= 0 and n >= skip)
    out[b, flow_base + 2 * n + i]    = flow[n * B + b, i]                      (flow_base >= 0)
    out[b, tap_base + 16 * n + k]    = taps[n * B + b, k]                      (tap_base >= 0)

with N = input1.size(0) // out.size(0) neighbours.  `out` is modified in place and returned; nothing else of it is touched.

Differentiable in input1, flow and taps: the backward pass is FilterInterpolationLayer's float32 entry point on the gathered
gradoutput slices (without an image gradient where input1 needs none) plus the gradoutput of the pass-through slices; a
gradient for `out` as it came in is the gradoutput with the written slices zeroed.  `detach=True` writes the slices without
gradient (the reference's `.detach()` on the context warps, :474).  float32 only: a half or mixed call, and a call the
kernel does not cover (channels neither 3 nor a multiple of 4, filters other than 4x4, widths or storage offsets that are
not 16-byte aligned, overlapping slices), is composed from FilterInterpolationLayer and `copy_` -- same values, no error.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import my_package._ext.my_lib as my_lib
import my_package._ext.my_lib_stack as my_lib_stack
from ._common import check, declined, f32c, require_gpu
from .FilterInterpolationLayer import FilterInterpolationLayer, _backward_fp32


def _slot(n, skip):
    return n + (1 if 0 <= skip <= n else 0)


def _slices(nb, channels, c_base, skip, flow_base, tap_base):
    """per neighbour n: (warp, flow or None, taps or None) channel slices of `out`"""
    return [(slice(c_base + _slot(n, skip) * channels, c_base + (_slot(n, skip) + 1) * channels),
             slice(flow_base + 2 * n, flow_base + 2 * n + 2) if flow_base >= 0 else None,
             slice(tap_base + 16 * n, tap_base + 16 * n + 16) if tap_base >= 0 else None) for n in range(nb)]


def _neighbours(out, input1):
    if out.dim() != 4 or input1.dim() != 4 or out.size(0) < 1 or input1.size(0) % out.size(0) != 0:
        raise ValueError("FilterInterpolationStackLayer: input1's rows %s are not a whole number of out's batch %s"
                         % (tuple(input1.shape), tuple(out.shape)))
    return input1.size(0) // out.size(0)


class _StackFunction(Function):
    @staticmethod
    def forward(ctx, out, input1, flow, taps, c_base, skip, flow_base, tap_base, detach):
        input1, flow, taps = f32c(input1), f32c(flow), f32c(taps)
        nb, batch = _neighbours(out, input1), out.size(0)
        sl = _slices(nb, input1.size(1), c_base, skip, flow_base, tap_base)
        err = my_lib_stack.FilterInterpolationStackLayer_gpu_forward(input1, flow, taps, out, nb, c_base, skip, flow_base,
                                                                     tap_base)
        if declined(err, "FilterInterpolationStackLayer_gpu_forward"):       # composed: one warp of the stack, copies
            warped = torch.empty_like(input1)
            check(my_lib.FilterInterpolationLayer_gpu_forward(input1, flow, taps, warped),
                  "FilterInterpolationLayer_gpu_forward")
            for n, (cw, cf, ct) in enumerate(sl):
                rows = slice(n * batch, (n + 1) * batch)
                out[:, cw].copy_(warped[rows])
                if cf is not None:
                    out[:, cf].copy_(flow[rows])
                if ct is not None:
                    out[:, ct].copy_(taps[rows])
        ctx.mark_dirty(out)
        ctx.slices, ctx.detach = sl, detach
        if not detach:
            ctx.save_for_backward(input1, flow, taps)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        gout = None
        if ctx.needs_input_grad[0]:                          # `out` as it came in: overwritten where a slice was written
            gout = gradoutput.clone()
            for cs in ctx.slices:
                for c in cs:
                    if c is not None:
                        gout[:, c].zero_()
        if ctx.detach:
            return (gout,) + (None,) * 8
        input1, flow, taps = ctx.saved_tensors
        gather = lambda i: torch.cat([gradoutput[:, cs[i]] for cs in ctx.slices], 0).float().contiguous()
        g1, g2, g3 = _backward_fp32(input1, flow, taps, gather(0), ctx.needs_input_grad[1])
        if ctx.slices[0][1] is not None:
            g2 += gather(1)
        if ctx.slices[0][2] is not None:
            g3 += gather(2)
        return gout, g1, g2, g3, None, None, None, None, None


def _composed(out, input1, flow, taps, c_base, skip, flow_base, tap_base, detach):
    """the same slices through FilterInterpolationLayer (whatever dtypes it takes) and autograd's own copy_"""
    nb, batch = _neighbours(out, input1), out.size(0)
    warped = FilterInterpolationLayer()(input1, flow, taps)
    if detach:
        warped, flow, taps = warped.detach(), flow.detach(), taps.detach()
    for n, (cw, cf, ct) in enumerate(_slices(nb, input1.size(1), c_base, skip, flow_base, tap_base)):
        rows = slice(n * batch, (n + 1) * batch)
        out[:, cw].copy_(warped[rows])
        if cf is not None:
            out[:, cf].copy_(flow[rows])
        if ct is not None:
            out[:, ct].copy_(taps[rows])
    return out


class FilterInterpolationStackLayer(object):
    """`FilterInterpolationStackLayer()(out, input1, flow, taps, c_base, skip, flow_base=-1, tap_base=-1, detach=False)`
    fills the slices of the caller's `out` and returns it."""

    def __call__(self, out, input1, flow, taps, c_base, skip, flow_base=-1, tap_base=-1, detach=False):
        require_gpu("FilterInterpolationStackLayer", out, input1, flow, taps)
        if all(t.dtype == torch.float32 for t in (out, input1, flow, taps)) and not torch.is_autocast_enabled():
            if detach:
                input1, flow, taps = input1.detach(), flow.detach(), taps.detach()
            return _StackFunction.apply(out, input1, flow, taps, int(c_base), int(skip), int(flow_base), int(tap_base),
                                        bool(detach))
        return _composed(out, input1, flow, taps, c_base, skip, flow_base, tap_base, detach)

    forward = __call__
