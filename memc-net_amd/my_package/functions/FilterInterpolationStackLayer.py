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
gradient (the reference's `.detach()` on the context warps, :474).  A call the kernel does not cover (channels neither 3
nor a multiple of 4, filters other than 4x4, widths or storage offsets that are not 16-byte aligned, overlapping slices)
is composed from FilterInterpolationLayer's entry point and `copy_` -- same values, no error.

float16 / bfloat16 (`native_half`, below): `out`, input1 and taps of one half dtype, the flow of that dtype or float32,
autocast off -- the same one launch on libmemc_hip_lp_stack.so (include/memc_warp_lp_stack.h; about 376 B per site and
neighbour against about 680 B composed), every warped value libmemc_hip_lp.so's bit for bit, a float32 flow stored as
`flow.to(out.dtype)`.  Where that library declines (as above, with 8-byte alignment): one
FilterInterpolationLayer_gpu_forward_lp call on the whole stack and `copy_`.  Backward: libmemc_hip_lp_grad.so on the
gathered gradoutput slices where it covers the call (three channels), else the float32 backward on the widened tensors;
each gradient is cast to its input's dtype and then the pass-through slices' gradoutput is added, which is the sum autograd
forms on the composed route.  Calls under autocast and calls of mixed dtypes keep the composed route (FilterInterpolationLayer
per dtype rule and `copy_`): under autocast torch.cat promotes the rectifier input to float32, another kernel contract.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import my_package._ext.my_lib as my_lib
import my_package._ext.my_lib_lp as my_lib_lp
import my_package._ext.my_lib_lp_stack as my_lib_lp_stack
import my_package._ext.my_lib_stack as my_lib_stack
from ._common import LOWP, cast_like, check, declined, f32c, require_gpu
from .FilterInterpolationLayer import (FilterInterpolationLayer, _backward_fp32, _backward_lp, _backward_widened,
                                       lp_backward_covered)


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


def _grad_of_out(ctx, gradoutput):
    """the gradient of `out` as it came in: the gradoutput, zero where a slice was written (`out` is overwritten there); None where nobody asks"""
    if not ctx.needs_input_grad[0]:
        return None
    gout = gradoutput.clone()
    for cs in ctx.slices:
        for c in cs:
            if c is not None:
                gout[:, c].zero_()
    return gout


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
        gout = _grad_of_out(ctx, gradoutput)
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


class _StackLpFunction(Function):
    """float16 / bfloat16: forward on libmemc_hip_lp_stack.so (where it declines: libmemc_hip_lp.so on the whole stack and
    copies); backward on libmemc_hip_lp_grad.so where it covers the call, else widened to float32"""

    @staticmethod
    def forward(ctx, out, input1, flow, taps, c_base, skip, flow_base, tap_base, detach):
        input1, flow, taps = input1.contiguous(), flow.contiguous(), taps.contiguous()
        nb, batch = _neighbours(out, input1), out.size(0)
        sl = _slices(nb, input1.size(1), c_base, skip, flow_base, tap_base)
        err = my_lib_lp_stack.FilterInterpolationStackLayer_gpu_forward_lp(input1, flow, taps, out, nb, c_base, skip,
                                                                           flow_base, tap_base)
        if declined(err, "FilterInterpolationStackLayer_gpu_forward_lp"):    # composed: one warp of the stack, copies
            warped = torch.empty_like(input1)
            check(my_lib_lp.FilterInterpolationLayer_gpu_forward_lp(input1, flow, taps, warped),
                  "FilterInterpolationLayer_gpu_forward_lp")
            for n, (cw, cf, ct) in enumerate(sl):
                rows = slice(n * batch, (n + 1) * batch)
                out[:, cw].copy_(warped[rows])
                if cf is not None:
                    out[:, cf].copy_(flow[rows])               # a float32 flow: rounded to out's dtype once
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
        gout = _grad_of_out(ctx, gradoutput)
        if ctx.detach:
            return (gout,) + (None,) * 8
        saved = ctx.saved_tensors
        gather = lambda i: torch.cat([gradoutput[:, cs[i]] for cs in ctx.slices], 0)      # noqa: E731
        grads = None
        if lp_backward_covered(saved[0], saved[2]):
            grads = _backward_lp(*saved, gather(0), ctx.needs_input_grad[1])
        if grads is None:
            grads = _backward_widened(saved, gather(0), ctx.needs_input_grad[1])
        # each gradient in its input's dtype first, then the pass-through's: the sum autograd forms on the composed route
        g1, g2, g3 = cast_like(grads, saved)
        if ctx.slices[0][1] is not None:
            g2 = g2 + gather(1).to(g2.dtype)
        if ctx.slices[0][2] is not None:
            g3 = g3 + gather(2).to(g3.dtype)
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

    # float16 / bfloat16 calls on libmemc_hip_lp_stack.so instead of composed from libmemc_hip_lp.so's warps and copy_.
    # Measured as MEMC_Net_VE runs the two routes (profiles/r25_ve_half_stack.txt, one MI355X, allocations included, routes
    # alternating over seven rounds): x0.353 of the composed route's time at 1 septuplet of 320 x 512 in bf16 (269 against
    # 762 us) and x0.347 in fp16 (261 against 752 us), x0.375 and x0.373 at 4 septuplets (732 against 1953 us, 729 against
    # 1952 us); the difference exceeds the larger of the two sides' spreads (at most 24 us) in all four groups, so on.  A
    # whole inference step: x0.96 (bf16), x0.95 (fp16).  Not measured: the kernels alone under a profiler, a training
    # step, other sizes than 320 x 512
    native_half = True

    def __call__(self, out, input1, flow, taps, c_base, skip, flow_base=-1, tap_base=-1, detach=False):
        require_gpu("FilterInterpolationStackLayer", out, input1, flow, taps)
        function = None
        if not torch.is_autocast_enabled():
            if all(t.dtype == torch.float32 for t in (out, input1, flow, taps)):
                function = _StackFunction
            elif (self.native_half and out.dtype in LOWP and input1.dtype == taps.dtype == out.dtype
                  and flow.dtype in (out.dtype, torch.float32)):
                function = _StackLpFunction
        if function is not None:
            if detach:
                input1, flow, taps = input1.detach(), flow.detach(), taps.detach()
            return function.apply(out, input1, flow, taps, int(c_base), int(skip), int(flow_base), int(tap_base),
                                  bool(detach))
        return _composed(out, input1, flow, taps, c_base, skip, flow_base, tap_base, detach)

    forward = __call__
