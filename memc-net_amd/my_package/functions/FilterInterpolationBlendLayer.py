"""FilterInterpolationBlendLayer -- EXTENSION, no reference counterpart.

    out = occlusion0 * FilterInterpolation(input0, flow0, filter0)
        + occlusion1 * FilterInterpolation(input2, flow1, filter1)

i.e. `FilterInterpolate` of networks/MEMC_Net_star.py:264-277 as ONE kernel (the two warped frames are never
written).  Differentiable; nothing but the inputs is kept for the backward pass.  Every kernel does float32 arithmetic on
the exactly widened values and rounds each stored value once; each gradient comes back in its input's dtype.

The routes, by the dtypes of the call ("half": float16 or bfloat16; "tiled": RGB, 4x4 filters, a width that is a multiple
of four from 8 on).  The backward is taken per direction d.  "composed" is _direction_backward: the warp's forward
recomputed, two elementwise passes, a zero-filled image gradient and the warp's whole backward, in float32.  "fused" is
ONE kernel on the raw gradoutput for a direction whose image needs no gradient (the frames of the networks are data):
flow, tap and occlusion gradients in one pass, image gradient None.  A library declines with return code 1 and has
touched nothing then.

  call                        forward                   backward of direction d                             where the library declines
  --------------------------  ------------------------  --------------------------------------------------  --------------------------
  float32, fused_supported    libmemc_hip, one kernel   no image gradient: fused, libmemc_hip_blend_grad    composed
                                                        (176 B per site); else composed, libmemc_hip
  float32, any other shape    two FilterInterpolationLayer calls and the blend in torch: same values, autograd's backward
  float32 images, half taps   libmemc_hip_mx on the     no image gradient: fused, on the saved tensors as   forward: widened, the
  and occlusions, tiled       tensors as they are       they are, libmemc_hip_mx_blend_grad (108 B per      float32 rows; backward:
  (blend_mx_covered: what     (112 B per site;          site; promoted: about 380); else the saved tensors  as "else"
  torch.autocast makes)       promoted: 416)            widened, the float32 rows, gradients cast back
  half payload                libmemc_hip_lp, any       composed on the widened tensors; where tiled, the   the warp's backward on
                              shape                     warp's backward on libmemc_hip_lp_grad (half image  libmemc_hip, widened
                                                        and taps, the float32 gradoutput * occlusion)
  half payload and            as above                  no image gradient: fused, on the saved tensors and  the row above
  fused_half_backward=True                              the gradoutput as it arrives (96 B per site),
                                                        libmemc_hip_lp_blend_grad; else the row above
  any other mix               cast to the payload dtype (functions/_common.py: payload_dtype over images, taps and
                              occlusions; the flows stay float32 or that dtype): the float32 or the half rows

The fused mixed gradients are the promoted call's, bit for bit; the fused half ones those of the float32 fused route on the
widened tensors, cast once.  float32 and mixed calls ignore fused_half_backward; without it a half call never reaches
libmemc_hip_lp_blend_grad.  Each library in turn, with its timings: INTEGRATION.md.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

import my_package._ext.my_lib as my_lib
import my_package._ext.my_lib_blend_grad as my_lib_blend_grad
import my_package._ext.my_lib_lp as my_lib_lp
import my_package._ext.my_lib_lp_blend_grad as my_lib_lp_blend_grad
import my_package._ext.my_lib_mx as my_lib_mx
from ._common import LOWP, cast, cast_like, check, declined, f32c, flow_dtype, payload_dtype, require_gpu
from .FilterInterpolationLayer import FilterInterpolationLayer, backward_lp, lp_backward_covered, mx_covered


def fused_supported(input0, filter0, *others):
    """What the fused kernel covers (the C side returns -1 for anything else): RGB, 16 taps, width a multiple of 4,
    a 1-channel occlusion, 16-byte aligned base pointers.  `others`: the remaining tensors of the call (their
    alignment and, for [B, 1, H, W] occlusions, their channel count are checked when given)."""
    if not (input0.size(1) == 3 and filter0.size(1) == 16 and input0.size(3) % 4 == 0):
        return False
    for t in (input0, filter0) + others:
        if t.is_cuda and t.data_ptr() % 16 != 0:            # e.g. a contiguous view with an odd storage offset
            return False
    return all(o.size(1) == 1 for o in others[-2:]) if len(others) >= 2 else True


def _warp(x, flow, filt):
    out = torch.empty_like(x)                                # every element is written
    check(my_lib.FilterInterpolationLayer_gpu_forward(x, flow, filt, out), "FilterInterpolationLayer_gpu_forward")
    return out


def _direction_backward(x, flow, filt, occ, gradoutput, half=None):
    """(image, flow, tap, occlusion) gradients of ONE direction occ * FI(x, flow, filt) of the blend, composed from the
    reference-API entry points: a forward recomputation, two elementwise passes, a zero-filled image gradient and the
    warp's whole backward.  half: the direction's float16 / bfloat16 (x, flow, filt) that the float32 arguments widen --
    the backward launch then runs on them (libmemc_hip_lp_grad.so) where the library covers it; its flow / tap
    gradients come back in their dtypes, the image gradient in float32."""
    warped = _warp(x, flow, filt)                            # recomputed, not stored by the forward pass
    g_occ = (gradoutput * warped).sum(dim=1, keepdim=True)
    g_warp = (gradoutput * occ).contiguous()
    g_x = torch.zeros_like(x)
    g_lp = None
    if half is not None and lp_backward_covered(half[0], half[2]):
        g_lp = backward_lp(half[0], half[1], half[2], g_warp, g_x)
    if g_lp is not None:
        g_flow, g_filt = g_lp
    else:
        g_flow, g_filt = torch.empty_like(flow), torch.empty_like(filt)
        check(my_lib.FilterInterpolationLayer_gpu_backward(x, flow, filt, g_warp, g_x, g_flow, g_filt),
              "FilterInterpolationLayer_gpu_backward")
    return g_x, g_flow, g_filt, g_occ


def _direction_backward_fused(x, flow, filt, occ, gradoutput):
    """(flow, tap, occlusion) gradients of ONE direction of the blend whose image wants no gradient, from ONE kernel on the
    tensors as they are and the raw gradoutput (every element of the three is assigned), each in its input's dtype:
    libmemc_hip_lp_blend_grad.so for a half image; else my_lib_blend_grad's door: libmemc_hip_blend_grad.so for float32
    tensors, libmemc_hip_mx_blend_grad.so for a float32 image beside half taps and occlusion.  None where the library
    declines the call (anything but RGB, 16 taps and a width that is a multiple of four from 8 on; a half view that is
    not made of 8-byte quads)."""
    g_flow, g_filt, g_occ = torch.empty_like(flow), torch.empty_like(filt), torch.empty_like(occ)
    if x.dtype in LOWP:
        name = "FilterInterpolationBlendLayer_gpu_backward_lp"
        err = my_lib_lp_blend_grad.FilterInterpolationBlendLayer_gpu_backward_lp(x, flow, filt, occ, gradoutput, g_flow,
                                                                                 g_filt, g_occ)
    else:
        name = "FilterInterpolationBlendLayer_gpu_backward"
        err = my_lib_blend_grad.FilterInterpolationBlendLayer_gpu_backward(x, flow, filt, occ, gradoutput, g_flow, g_filt,
                                                                           g_occ)
    return None if declined(err, name) else (g_flow, g_filt, g_occ)


def _blend_backward(saved, gradoutput, half=None, needs_image_grad=(True, True)):
    """gradients of occ0 * FI(in0, flow0, filt0) + occ1 * FI(in2, flow1, filt1) w.r.t. its eight inputs.  A direction
    whose image needs a gradient (needs_image_grad[d]), and every direction of a half call, is composed from the
    reference-API entry points (_direction_backward: a forward recomputation + a backward launch).  A float32 direction
    whose image needs none takes the fused kernel (_direction_backward_fused) where it covers the call: its image gradient
    is None.  half: the float16 / bfloat16 tensors that `saved` widens."""
    grads = [_direction_grads(saved[d::2], gradoutput, None if half is None else half[d:6:2], needs_image_grad[d])
             for d in (0, 1)]
    return _interleave(grads)


def _direction_grads(direction, gradoutput, half, needs_image_grad):
    """(image, flow, tap, occlusion) gradients of ONE float32 direction (x, flow, filt, occ): see _blend_backward"""
    x, flow, filt, occ = direction
    fused = None
    if half is None and not needs_image_grad:
        fused = _direction_backward_fused(x, flow, filt, occ, gradoutput)
    if fused is not None:
        return (None,) + fused
    return _direction_backward(x, flow, filt, occ, gradoutput, half)


def _interleave(grads):
    """the two directions' (image, flow, tap, occlusion) gradients in the order of the layer's eight inputs"""
    (gx0, gf0, gk0, go0), (gx2, gf1, gk1, go1) = grads
    return gx0, gx2, gf0, gf1, gk0, gk1, go0, go1


class _FilterInterpolationBlendFunction(Function):
    @staticmethod
    def forward(ctx, input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1):
        args = (input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1)
        require_gpu("FilterInterpolationBlendLayer", *args)
        args = tuple(f32c(t) for t in args)
        output = torch.empty_like(args[0])                   # every element is written
        check(my_lib.FilterInterpolationBlendLayer_gpu_forward(*args, output),
              "FilterInterpolationBlendLayer_gpu_forward")
        ctx.save_for_backward(*args)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        return _blend_backward(ctx.saved_tensors, f32c(gradoutput), needs_image_grad=ctx.needs_input_grad[:2])


class _FilterInterpolationBlendLpFunction(Function):
    """float16 / bfloat16: forward on libmemc_hip_lp.so; backward: float32 recomputation of the warps and occlusion
    gradients, the two warp backward launches on libmemc_hip_lp_grad.so where it covers them"""

    @staticmethod
    def forward(ctx, input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1):
        args = tuple(t.contiguous() for t in (input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1))
        output = torch.empty_like(args[0])                   # every element is written
        check(my_lib_lp.FilterInterpolationBlendLayer_gpu_forward_lp(*args, output),
              "FilterInterpolationBlendLayer_gpu_forward_lp")
        ctx.save_for_backward(*args)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        saved = ctx.saved_tensors
        grads = _blend_backward(tuple(t.float().contiguous() for t in saved), gradoutput.float().contiguous(), half=saved)
        return cast_like(grads, saved)


def _backward_on_saved(ctx, gradoutput, half):
    """The backward of the two Functions that hand the saved tensors to a fused kernel as they are.  Per direction: an
    image that wants no gradient takes _direction_backward_fused; where it does, or the library declines, the direction is
    widened, takes _direction_grads and each gradient is cast back.  half: a pure half call -- composed with the half
    tensors (so that libmemc_hip_lp_grad.so takes the warp's backward), the gradoutput widened once and only if some
    direction needs it; else a mixed call with a float32 gradoutput -- the float32 routes for the real need."""
    saved, grads, wide = ctx.saved_tensors, [], None
    for d in (0, 1):
        direction, fused = saved[d::2], None                 # (x, flow, filt, occ), contiguous already
        if not ctx.needs_input_grad[d]:
            fused = _direction_backward_fused(*direction, gradoutput)          # in the inputs' dtypes
        if fused is not None:
            grads.append((None,) + fused)
            continue
        if wide is None:
            wide = gradoutput.float().contiguous()
        g = _direction_grads(tuple(t.float().contiguous() for t in direction), wide, saved[d:6:2] if half else None,
                             half or ctx.needs_input_grad[d])
        grads.append(cast_like(g, direction))
    return _interleave(grads)


class _FilterInterpolationBlendLpFusedFunction(_FilterInterpolationBlendLpFunction):
    """float16 / bfloat16 with fused_half_backward: the forward of _FilterInterpolationBlendLpFunction, the backward on
    libmemc_hip_lp_blend_grad.so wherever a direction's image wants no gradient (_backward_on_saved)"""

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        return _backward_on_saved(ctx, gradoutput.contiguous(), half=True)


def _blend_forward_fp32(args):
    """the blend of eight contiguous float32 tensors: the fused kernel where it takes the call, else two warps"""
    if fused_supported(args[0], args[4], args[1], args[2], args[3], args[5], args[6], args[7]):
        output = torch.empty_like(args[0])                   # every element is written
        check(my_lib.FilterInterpolationBlendLayer_gpu_forward(*args, output),
              "FilterInterpolationBlendLayer_gpu_forward")
        return output
    return args[6] * _warp(args[0], args[2], args[4]) + args[7] * _warp(args[1], args[3], args[5])


class _FilterInterpolationBlendMxFunction(Function):
    """float32 images, float16 / bfloat16 taps and occlusions, flows in float32 or that dtype: forward on libmemc_hip_mx.so
    (where it declines: promoted to float32, the float32 kernels); backward on libmemc_hip_mx_blend_grad.so wherever a
    direction's image wants no gradient (_backward_on_saved)"""

    @staticmethod
    def forward(ctx, input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1):
        args = tuple(t.contiguous() for t in (input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1))
        output = torch.empty_like(args[0])                   # every element is written
        err = my_lib_mx.FilterInterpolationBlendLayer_gpu_forward_mx(*args, output)
        if declined(err, "FilterInterpolationBlendLayer_gpu_forward_mx"):      # the promoted route
            output = _blend_forward_fp32(tuple(t.float() for t in args))
        ctx.save_for_backward(*args)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, gradoutput):
        return _backward_on_saved(ctx, f32c(gradoutput), half=False)


def blend_mx_covered(input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1):
    """The mixed call libmemc_hip_mx.so takes (include/memc_warp_mx.h): float32 images, taps and occlusions of ONE half
    dtype, the two flows of one dtype (float32 or that one), RGB, 16 taps, a width that is a multiple of four from 8 on"""
    t = filter0.dtype
    return (mx_covered(input0, filter0) and input2.dtype == torch.float32 and input2.shape == input0.shape and
            all(x.dtype == t for x in (filter1, occlusion0, occlusion1)) and
            occlusion0.size(1) == 1 and occlusion1.size(1) == 1 and flow_dtype(flow0, t) == flow_dtype(flow1, t))


class FilterInterpolationBlendLayer(object):
    """`FilterInterpolationBlendLayer()(input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1)`;
    fused_half_backward: the backward of a pure float16 / bfloat16 call takes libmemc_hip_lp_blend_grad.so for every
    direction whose image needs no gradient (see the module's docstring)"""

    def __init__(self, fused_half_backward=False):
        self.fused_half_backward = fused_half_backward

    def __call__(self, input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1):
        require_gpu("FilterInterpolationBlendLayer", input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1)
        if blend_mx_covered(input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1):
            fdt = flow_dtype(flow0, filter0.dtype)
            return _FilterInterpolationBlendMxFunction.apply(input0, input2, cast(flow0, fdt), cast(flow1, fdt), filter0,
                                                             filter1, occlusion0, occlusion1)
        dtype = payload_dtype(input0, input2, filter0, filter1, occlusion0, occlusion1)
        if dtype != torch.float32:
            fdt = flow_dtype(flow0, dtype) if flow_dtype(flow0, dtype) == flow_dtype(flow1, dtype) else torch.float32
            function = _FilterInterpolationBlendLpFusedFunction if self.fused_half_backward \
                else _FilterInterpolationBlendLpFunction
            return function.apply(
                cast(input0, dtype), cast(input2, dtype), cast(flow0, fdt), cast(flow1, fdt), cast(filter0, dtype),
                cast(filter1, dtype), cast(occlusion0, dtype), cast(occlusion1, dtype))
        input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1 = (
            cast(t, dtype) for t in (input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1))
        if fused_supported(input0, filter0, input2, flow0, flow1, filter1, occlusion0, occlusion1):
            return _FilterInterpolationBlendFunction.apply(input0, input2, flow0, flow1, filter0, filter1,
                                                           occlusion0, occlusion1)
        warp = FilterInterpolationLayer()
        return occlusion0 * warp(input0, flow0, filter0) + occlusion1 * warp(input2, flow1, filter1)
