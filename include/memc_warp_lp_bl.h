/*
 * memc_warp_lp_bl.h -- C ABI of libmemc_hip_lp_bl.so: the plain bilinear backward warp (Interpolation / InterpolationCh) on
 * fp16 / bf16 storage, forward and RGB backward, hand-written HIP kernels for gfx950 (MI355X).
 *
 * This is the bilinear warp of a model cast to bf16 / fp16: the image and the output are of that type, the flow is of that
 * type or float32.  A library of its own: libmemc_hip.so (include/memc_warp.h) and the other satellite libraries are
 * untouched by it.  memc_dtype and memc_tensor4 come from memc_warp_lp.h.
 *
 * Numerics contract:
 *   - payload dtype T (MEMC_F16 or MEMC_BF16): input1 (the image), output, gradoutput;
 *   - flow dtype FT: MEMC_F32 or T, for input2 (the flow) and gradinput2 (its gradient), decoded in the kernel;
 *   - every input is widened to float32 exactly; the arithmetic is that of InterpolationLayer_gpu_forward / _backward
 *     (include/memc_warp.h) in the same order: per site and channel w00 * TL + w01 * TR + w10 * BL + w11 * BR; sites whose
 *     target lies outside the image store 0;
 *   - every stored element of the output and of gradinput2 is rounded to its dtype ONCE, round-to-nearest-even, overflow to
 *     +-inf (exactly what torch's `tensor.to(T)` does).  So for the same inputs they equal, bit for bit, the fp32 library's
 *     results on the widened inputs rounded to their dtype (with a float32 flow gradinput2 is not rounded at all);
 *   - gradinput2 is ASSIGNED at every site (0 at sites outside the image): it needs no zero fill;
 *   - gradinput1 (the image gradient) is a FLOAT32 buffer of input1's shape and element layout that the kernel ADDS into
 *     (its tiles' boxes overlap and are flushed with fp32 atomics, which a T target could not take without rounding each
 *     add): the caller zero-fills it and rounds it to T afterwards.  As in the fp32 library it is not bit-reproducible
 *     from run to run where more than one order of the adds rounds differently.
 *
 * Forward: any well-formed call is served whose planes lie within int ELEMENT offsets -- (H - 1) * input1's row stride
 * + W at most INT32_MAX: every forward kernel forms a site's four source offsets as `row * row_stride + column` in int; a
 * view beyond that returns 1 with nothing touched (the flow's offsets are 64-bit: its row stride has no limit).  The tiled
 * kernels ("bl_fwd_lp:tiled_c3" for C == 3, "bl_fwd_lp:tiled_chunks" for any other channel count) take the coverage
 * below; everything else -- any width, stride and alignment -- takes the one-lane-per-site kernel ("bl_fwd_lp:direct").
 *
 * Backward: C == 3 inside the coverage below ("bl_bwd_lp:tiled_c3"); every other well-formed call returns 1 with nothing
 * touched: the caller widens to float32 and takes InterpolationLayer_gpu_backward.
 *
 * Coverage of the tiled kernels: a width that is a multiple of four from 8 on; T tensors with row / channel / batch strides
 * that are multiples of four elements and 8-byte aligned bases; float32 tensors (a float32 flow and its gradient,
 * gradinput1) dword aligned; for the backward every plane within 32-bit byte offsets.
 *
 * Layout: NCHW, element strides (int64), w-stride 1; input1 [B, C, H, W], input2 [B, 2, H, W]; output, gradoutput and
 * gradinput1 have input1's shape and layout, gradinput2 input2's.  The Interpolation entry points insist on C == 3, the
 * InterpolationCh ones take any channel count.
 *
 * Return: 0 enqueued (an empty batch enqueues nothing and returns 0); 1 a well-formed call outside the coverage (the
 * backward's; the forward: only a plane beyond int element offsets) -- nothing is touched or enqueued; -1 a failed
 * descriptor check (before the device is touched: a payload dtype that is not F16 / BF16, a flow dtype that is neither
 * F32 nor the payload's, a null descriptor or null data, negative or beyond-int32 sizes and strides, a w-stride other
 * than 1, a flow that is not [B, 2, H, W], an output / gradoutput / gradinput1 / gradinput2 of another shape or layout,
 * Interpolation with C != 3) or a launch error.  Work is enqueued asynchronously on `stream`; nothing is allocated,
 * synchronised or kept between calls; every call is stream-capturable.
 */
#ifndef MEMC_WARP_LP_BL_H
#define MEMC_WARP_LP_BL_H

#include "memc_warp_lp.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Library / build identification: "memc_hip_lp_bl 0.1 gfx950". */
const char *memc_lp_bl_version(void);

/* Kernel family of the most recent enqueued call made BY THE CALLING THREAD: "bl_fwd_lp:tiled_c3", "bl_fwd_lp:tiled_chunks",
 * "bl_fwd_lp:direct" or "bl_bwd_lp:tiled_c3"; "" before the first enqueued call (a declined, rejected or empty call does
 * not change it). */
const char *memc_lp_bl_last_kernel_path(void);

/* output (payload_dtype, assigned in every element) = the bilinear warp of input1 (payload_dtype) by input2 (flow_dtype). */
int InterpolationLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype payload_dtype, memc_dtype flow_dtype,
                                      const memc_tensor4 *input1, const memc_tensor4 *input2, const memc_tensor4 *output);
int InterpolationChLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype payload_dtype, memc_dtype flow_dtype,
                                        const memc_tensor4 *input1, const memc_tensor4 *input2, const memc_tensor4 *output);

/* The backward of that warp for gradoutput (payload_dtype): gradinput1 (float32, zero-filled by the caller, added into),
 * gradinput2 (flow_dtype, assigned). */
int InterpolationLayer_gpu_backward_lp(memc_stream_t stream, memc_dtype payload_dtype, memc_dtype flow_dtype,
                                       const memc_tensor4 *input1, const memc_tensor4 *input2,
                                       const memc_tensor4 *gradoutput, const memc_tensor4 *gradinput1,
                                       const memc_tensor4 *gradinput2);
int InterpolationChLayer_gpu_backward_lp(memc_stream_t stream, memc_dtype payload_dtype, memc_dtype flow_dtype,
                                         const memc_tensor4 *input1, const memc_tensor4 *input2,
                                         const memc_tensor4 *gradoutput, const memc_tensor4 *gradinput1,
                                         const memc_tensor4 *gradinput2);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_WARP_LP_BL_H */
