/*
 * memc_warp_mx_grad.h -- C ABI of libmemc_hip_mx_grad.so: the RGB backward of the adaptive warp (FilterInterpolation) on
 * MIXED storage -- an fp32 image and an fp32 gradoutput beside fp16 / bf16 filter taps -- a hand-written HIP kernel for
 * gfx950 (MI355X).
 *
 * This is the backward of the call torch.autocast makes (include/memc_warp_mx.h is its forward): the frames are the
 * network's input and stay float32, the output of the mixed forward is float32 and so is its gradient, the heads' taps
 * are half.  A library of its own: libmemc_hip.so (include/memc_warp.h, fp32), the half libraries (memc_warp_lp.h,
 * memc_warp_lp_grad.h) and the mixed forward (memc_warp_mx.h) are untouched by it.  memc_dtype comes from memc_warp_lp.h.
 *
 * Numerics contract (that of memc_warp_lp_grad.h with the image and gradoutput in fp32):
 *   - tap dtype T (MEMC_F16 or MEMC_BF16): input3 (filter taps) and gradinput3 (tap gradient);
 *   - flow dtype: MEMC_F32 or T, for input2 (flow) and gradinput2 (flow gradient);
 *   - input1 (image) and gradoutput are fp32;
 *   - gradinput1 (image gradient): NULL, or an fp32 buffer of input1's shape and layout that the kernel ADDS into (its
 *     tiles' boxes overlap and are flushed with fp32 atomics); the caller zero-fills it;
 *   - the arithmetic is that of FilterInterpolationLayer_gpu_backward's RGB kernel (include/memc_warp.h), in the same order,
 *     on the widened inputs (widening is exact); gradinput2 and gradinput3 are rounded to their dtype ONCE,
 *     round-to-nearest-even, overflow to +-inf (exactly what torch's `tensor.to(T)` does).  So for the same inputs they
 *     equal, bit for bit, the fp32 library's results on the widened inputs rounded to their dtype, provided the same
 *     choice of gradinput1: a NULL gradinput1 takes the fp32 library's NULL path, a buffer its whole backward (the two
 *     sum gradinput2 of sites whose window no LDS band covers in different orders).  gradinput1 itself is, as in the fp32
 *     library, not bit-reproducible from run to run (atomics); with gradinput1 == NULL there are no atomics at all;
 *   - gradinput2 and gradinput3 are fully written (sites outside the image get zeros); nothing needs a zero fill but
 *     gradinput1.
 *
 * Coverage (return 1 outside it): C == 3, 16 taps (fs == 4), a width that is a multiple of four from 8 on, every plane
 * within 32-bit byte offsets; T tensors with row / channel / batch strides that are multiples of four elements and 8-byte
 * aligned bases (those of libmemc_hip_lp.so's tiled kernels); fp32 tensors need dword alignment only, as in libmemc_hip.so.
 * There is no kernel for other shapes: the caller promotes such a call to fp32, as it did before this library existed.
 *
 * Layout: NCHW, element strides (int64, memc_tensor4 of include/memc_warp.h), w-stride 1; gradoutput and gradinput1 have
 * input1's layout, gradinput2 input2's, gradinput3 input3's.
 *
 * Return: 0 enqueued (an empty batch launches nothing and returns 0); 1 a well-formed call outside the coverage above --
 * nothing is touched or enqueued; -1 a failed descriptor check (before the device is touched: a tap dtype that is not
 * F16 / BF16, a flow dtype that is neither F32 nor the taps', mismatched shapes or layouts, a tap count that is not a
 * square, null data, a w-stride other than 1, strides beyond int32, a gradinput1 not of input1's shape and layout) or a
 * launch error.  Work is enqueued asynchronously on `stream`; nothing is allocated or kept, so a call can be captured in a
 * graph.
 */
#ifndef MEMC_WARP_MX_GRAD_H
#define MEMC_WARP_MX_GRAD_H

#include "memc_warp_lp.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Library / build identification: "memc_hip_mx_grad 0.1 gfx950". */
const char *memc_mx_grad_version(void);

/* Kernel family of the most recent enqueued call made BY THE CALLING THREAD: "fi_bwd_mx:tiled_c3" (with the image
 * gradient), "fi_bwd_mx:tiled_c3_noimage" (gradinput1 == NULL); "" before the first enqueued call (a declined or rejected
 * call does not change it). */
const char *memc_mx_grad_last_kernel_path(void);

/* The backward of output (fp32) = FilterInterpolation(input1 (fp32), input2 (flow, flow_dtype), input3 (taps, tap_dtype))
 * for gradoutput (fp32): gradinput1 (NULL, or fp32, zero-filled, added into), gradinput2 (flow_dtype), gradinput3
 * (tap_dtype). */
int FilterInterpolationLayer_gpu_backward_mx(memc_stream_t stream, memc_dtype tap_dtype, memc_dtype flow_dtype,
                                             const memc_tensor4 *input1, const memc_tensor4 *input2,
                                             const memc_tensor4 *input3, const memc_tensor4 *gradoutput,
                                             const memc_tensor4 *gradinput1, const memc_tensor4 *gradinput2,
                                             const memc_tensor4 *gradinput3);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_WARP_MX_GRAD_H */
