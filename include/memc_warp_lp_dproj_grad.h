/*
 * memc_warp_lp_dproj_grad.h -- C ABI of libmemc_hip_lp_dproj_grad.so: the backward of DepthFlowProjectionLayer on an fp16 /
 * bf16 flow, depth, gradoutput and gradients, a hand-written HIP kernel for gfx950 (MI355X).
 *
 * This is the depth-weighted projection's backward of a model cast to bf16 / fp16: the flow and the depth the network holds,
 * the gradient it hands down and the two gradients it expects are all of that type; the count and the forward's output are
 * what the float32 forward returned (DepthFlowProjectionLayer_gpu_forward of include/memc_warp.h -- the forward has no half
 * kernel).  A library of its own: libmemc_hip.so (include/memc_warp.h) and the other satellite libraries are untouched by
 * it.  memc_dtype comes from memc_warp_lp.h.
 *
 * Contract: that of DepthFlowProjectionLayer_gpu_backward (memc_warp.h) -- a pure gather, every element of gradinput1 and
 * gradinput2 ASSIGNED (no zero fill needed), no atomics, nothing allocated, synchronised or kept between calls,
 * stream-capturable -- with the dtype rule of the half libraries:
 *   - payload dtype T (MEMC_F16 or MEMC_BF16): input1 (the flow), input2 (the depth), gradoutput, gradinput1 and
 *     gradinput2; count and output (the forward's result) are float32;
 *   - the arithmetic is that of DepthFlowProjectionLayer_gpu_backward's tiled kernel, in the same order, in float32 on the
 *     widened inputs (widening is exact): per target cell 1.0f / count, then gradoutput * that; per site, with d its depth
 *     and (fx, fy) its flow, over the four corners top-left, top-right, bottom-left, bottom-right
 *     gx += -qx * d, gy += -qy * d, then gd += -qx * (fx - out_x) over the four, then gd += -qy * (fy - out_y); each
 *     gradient element is rounded to T ONCE, round-to-nearest-even, overflow to +-inf (exactly what torch's `tensor.to(T)`
 *     does).  So for the same inputs gradinput1 and gradinput2 equal, bit for bit, the fp32 library's results on the
 *     widened inputs rounded to T;
 *   - a site whose target lies outside the image gets zero in all three gradient planes.
 *
 * Coverage (return 1 outside it): a width that is a multiple of four from 8 on; input1, input2, gradoutput, gradinput1 and
 * gradinput2 with row / channel / batch strides that are multiples of four elements and 8-byte aligned bases; a
 * dword-aligned count and output; every plane within 32-bit byte offsets.  There is no half kernel for other calls: the
 * caller widens and takes DepthFlowProjectionLayer_gpu_backward.
 *
 * Layout: NCHW, element strides (int64), w-stride 1; input1 [B, 2, H, W], input2 and count [B, 1, H, W]; output, gradoutput
 * and gradinput1 have input1's shape and layout (the same element strides, whatever their storage), gradinput2 has input2's.
 *
 * Return: 0 enqueued (an empty batch launches nothing and returns 0); 1 a well-formed call outside the coverage above --
 * nothing is touched or enqueued; -1 a failed descriptor check (before the device is touched: a payload dtype that is not
 * F16 / BF16, a null descriptor or null data, negative or beyond-int32 sizes and strides, a w-stride other than 1, an
 * input1 that is not [B, 2, H, W], an input2 or a count that is not [B, 1, H, W], an output, gradoutput or gradinput1 not
 * of input1's shape and layout, a gradinput2 not of input2's) or a launch error.
 */
#ifndef MEMC_WARP_LP_DPROJ_GRAD_H
#define MEMC_WARP_LP_DPROJ_GRAD_H

#include "memc_warp_lp.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Library / build identification: "memc_hip_lp_dproj_grad 0.1 gfx950". */
const char *memc_lp_dproj_grad_version(void);

/* Kernel family of the most recent enqueued call made BY THE CALLING THREAD: "dproj_bwd_lp:tiled"; "" before the first
 * enqueued call (a declined or rejected call does not change it). */
const char *memc_lp_dproj_grad_last_kernel_path(void);

/* gradinput1 and gradinput2 (payload_dtype, assigned) of the depth-weighted projection of input1 by input2 (payload_dtype)
 * for gradoutput (payload_dtype), the float32 count and the float32 output of the forward. */
int DepthFlowProjectionLayer_gpu_backward_lp(memc_stream_t stream, memc_dtype payload_dtype, const memc_tensor4 *input1,
                                             const memc_tensor4 *input2, const memc_tensor4 *count,
                                             const memc_tensor4 *output, const memc_tensor4 *gradoutput,
                                             const memc_tensor4 *gradinput1, const memc_tensor4 *gradinput2);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_WARP_LP_DPROJ_GRAD_H */
