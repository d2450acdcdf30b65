/*
 * memc_warp_lp_blend_grad.h -- C ABI of libmemc_hip_lp_blend_grad.so: the backward of one direction of the fused dual
 * adaptive warp + occlusion blend (FilterInterpolationBlendLayer) on fp16 / bf16 storage -- a half image beside half filter
 * taps and occlusion -- for callers that do not want the image gradient, a hand-written HIP kernel for gfx950 (MI355X).
 *
 * This is the blend's backward of a model cast to bf16 / fp16 (FilterInterpolationBlendLayer_gpu_forward_lp of
 * include/memc_warp_lp.h is its forward).  A library of its own: libmemc_hip.so (include/memc_warp.h), the half warp
 * libraries (memc_warp_lp.h, memc_warp_lp_grad.h), the fp32 blend backward (memc_warp_blend_grad.h) and the mixed libraries
 * (memc_warp_mx.h, memc_warp_mx_grad.h, memc_warp_mx_blend_grad.h) are untouched by it.  memc_dtype comes from
 * memc_warp_lp.h.
 *
 * Contract: that of memc_warp_blend_grad.h -- ONE direction (input, flow, filter, occlusion) per call, the RAW gradoutput
 * of the blend, all three outputs ASSIGNED in every element, no atomics, nothing allocated, synchronised or kept between
 * calls, stream-capturable -- with the dtype rule of memc_warp_lp_grad.h:
 *   - payload dtype T (MEMC_F16 or MEMC_BF16): input (image), filter, occlusion, gradfilter and gradocclusion;
 *   - flow dtype: MEMC_F32 or T, for flow and gradflow;
 *   - gradoutput dtype: MEMC_F32 or T;
 *   - the arithmetic is that of FilterInterpolationBlendLayer_gpu_backward (memc_warp_blend_grad.h), in the same order, on
 *     the widened inputs (widening is exact); each gradient is rounded to its dtype ONCE, round-to-nearest-even, overflow
 *     to +-inf (exactly what torch's `tensor.to(T)` does).  So for the same inputs the three outputs equal, bit for bit,
 *     the fp32 library's results on the widened inputs rounded to their dtype;
 *   - at a site whose target lies outside the image gradfilter and gradflow are zero and gradocclusion is
 *     sum_c gradoutput_c * input_c, summed in fp32 and rounded once.
 *
 * Coverage (return 1 outside it): C == 3, 16 taps (fs == 4), a width that is a multiple of four from 8 on, every plane
 * within 32-bit byte offsets; T tensors with row / channel / batch strides that are multiples of four elements and 8-byte
 * aligned bases; fp32 tensors need dword alignment only.  There is no kernel for other shapes: the caller composes such a
 * call from the warp's entry points.
 *
 * Layout: NCHW, element strides (int64), w-stride 1; flow [B, 2, H, W], filter [B, 16, H, W], occlusion [B, 1, H, W];
 * gradoutput has input's shape and layout, gradflow flow's, gradfilter filter's, gradocclusion occlusion's.
 *
 * Return: 0 enqueued (an empty batch launches nothing and returns 0); 1 a well-formed call outside the coverage above --
 * nothing is touched or enqueued; -1 a failed descriptor check (before the device is touched: a payload dtype that is not
 * F16 / BF16, a flow or gradoutput dtype that is neither F32 nor the payload's, null data, negative or beyond-int32 sizes
 * and strides, a w-stride other than 1, a flow that is not [B, 2, H, W], a tap count that is not a square, an occlusion
 * that is not [B, 1, H, W], a gradient not of its input's shape and layout) or a launch error.
 */
#ifndef MEMC_WARP_LP_BLEND_GRAD_H
#define MEMC_WARP_LP_BLEND_GRAD_H

#include "memc_warp_lp.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Library / build identification: "memc_hip_lp_blend_grad 0.1 gfx950". */
const char *memc_lp_blend_grad_version(void);

/* Kernel family of the most recent enqueued call made BY THE CALLING THREAD: "fi_blend_bwd_lp:tiled_c3"; "" before the
 * first enqueued call (a declined or rejected call does not change it). */
const char *memc_lp_blend_grad_last_kernel_path(void);

/* gradflow (flow_dtype), gradfilter and gradocclusion (payload_dtype), all assigned, of one direction of the blend of
 * input, filter and occlusion (payload_dtype) and flow (flow_dtype) for its raw gradoutput (gradoutput_dtype). */
int FilterInterpolationBlendLayer_gpu_backward_lp(memc_stream_t stream, memc_dtype payload_dtype, memc_dtype flow_dtype,
                                                  memc_dtype gradoutput_dtype, const memc_tensor4 *input,
                                                  const memc_tensor4 *flow, const memc_tensor4 *filter,
                                                  const memc_tensor4 *occlusion, const memc_tensor4 *gradoutput,
                                                  const memc_tensor4 *gradflow, const memc_tensor4 *gradfilter,
                                                  const memc_tensor4 *gradocclusion);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_WARP_LP_BLEND_GRAD_H */
