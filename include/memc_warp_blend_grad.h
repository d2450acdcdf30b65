/*
 * memc_warp_blend_grad.h -- C ABI of libmemc_hip_blend_grad.so: the backward of one direction of the fused dual adaptive
 * warp + occlusion blend (FilterInterpolationBlendLayer) for callers that do not want the image gradient, fp32, a
 * hand-written HIP kernel for gfx950 (MI355X).
 *
 * A library of its own: libmemc_hip.so (include/memc_warp.h), libmemc_hip_lp.so (include/memc_warp_lp.h) and
 * libmemc_hip_lp_grad.so (include/memc_warp_lp_grad.h) are untouched by it.  memc_tensor4 / memc_stream_t come from
 * memc_warp.h (through memc_warp_lp.h).
 *
 * Contract:
 *   - the blend is  out = occlusion0 * FI(input0, flow0, filter0) + occlusion1 * FI(input2, flow1, filter1),  FI the
 *     adaptive warp (FilterInterpolation).  ONE call takes ONE direction (input, flow, filter, occlusion) and the RAW
 *     gradoutput of the blend -- not gradoutput * occlusion.  With, per tap k of a site's 4 x 4 window,
 *         s_k = sum_c gradoutput_c * pixel_c(k),   t_k = w_k * s_k     (w_k: the tap's bilinear weight; t_k is the
 *                                                                      warp's tap gradient for this gradoutput)
 *     it computes
 *         gradfilter[k]  = occlusion * t_k,
 *         gradflow       = occlusion * (gx, gy)         (gx, gy: the warp's flow gradient for this gradoutput),
 *         gradocclusion  = sum_k filter_k * t_k         (= sum_c gradoutput_c * FI(input, flow, filter)_c);
 *     at a site whose target lies outside the image the forward copies the input pixel (as FilterInterpolation does), so
 *     gradfilter and gradflow are zero there and gradocclusion = sum_c gradoutput_c * input_c;
 *   - there is no image gradient: a caller that wants one composes FilterInterpolationLayer_gpu_forward / _backward of
 *     include/memc_warp.h;
 *   - the three outputs are ASSIGNED, every element of them: they need no zero fill and may be handed over uninitialised;
 *   - no atomics: the results are a pure function of the inputs, bit for bit from run to run;
 *   - nothing is allocated, synchronised or kept between calls; work is enqueued asynchronously on `stream`, so a call
 *     is stream-capturable.
 *
 * Coverage (return 1 outside it): C == 3, 16 taps (fs == 4), a width that is a multiple of four from 8 on, every plane
 * within 32-bit byte offsets.  Bases and strides need dword alignment only.
 *
 * Layout: NCHW, element strides (int64), w-stride 1; flow [B, 2, H, W], filter [B, 16, H, W], occlusion [B, 1, H, W];
 * gradoutput has input's shape and layout, gradflow flow's, gradfilter filter's, gradocclusion occlusion's.
 *
 * Return: 0 enqueued (an empty batch launches nothing and returns 0); 1 a well-formed call outside the coverage above --
 * nothing is touched or enqueued, the caller composes the warp's entry points; -1 a failed descriptor check (before the
 * device is touched: null data, negative or beyond-int32 sizes and strides, a w-stride other than 1, a flow that is not
 * [B, 2, H, W], a tap count that is not a square, an occlusion that is not [B, 1, H, W], a gradoutput not of input's shape
 * and layout, a gradient not of its input's shape and layout) or a launch error.
 */
#ifndef MEMC_WARP_BLEND_GRAD_H
#define MEMC_WARP_BLEND_GRAD_H

#include "memc_warp_lp.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Library / build identification, e.g. "memc_hip_blend_grad 0.1 gfx950". */
const char *memc_blend_grad_version(void);

/* Kernel family of the most recent enqueued call made BY THE CALLING THREAD: "fi_blend_bwd:tiled_c3"; "" before the
 * first enqueued call. */
const char *memc_blend_grad_last_kernel_path(void);

/* gradflow, gradfilter and gradocclusion (all assigned) of one direction of the blend for its raw gradoutput. */
int FilterInterpolationBlendLayer_gpu_backward(memc_stream_t stream, const memc_tensor4 *input, const memc_tensor4 *flow,
                                               const memc_tensor4 *filter, const memc_tensor4 *occlusion,
                                               const memc_tensor4 *gradoutput, const memc_tensor4 *gradflow,
                                               const memc_tensor4 *gradfilter, const memc_tensor4 *gradocclusion);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_WARP_BLEND_GRAD_H */
