/*
 * memc_warp_mx.h -- C ABI of libmemc_hip_mx.so: the RGB adaptive warp (FilterInterpolation) forward and the fused dual
 * warp + occlusion blend on MIXED storage -- an fp32 image and an fp32 output beside fp16 / bf16 filter taps and
 * occlusions -- hand-written HIP kernels for gfx950 (MI355X).
 *
 * This is the call torch.autocast makes: the frames are the network's input and stay float32, the heads return half taps
 * and occlusions.  A library of its own: libmemc_hip.so (include/memc_warp.h, fp32) and the half libraries
 * (include/memc_warp_lp.h, memc_warp_lp_grad.h) are untouched by it.  memc_dtype comes from memc_warp_lp.h.
 *
 * Numerics contract:
 *   - tap dtype T (MEMC_F16 or MEMC_BF16): the filter taps and, in the blend, the occlusions;
 *   - flow dtype: MEMC_F32 or T;
 *   - the image(s) and the output are fp32;
 *   - every input is widened to fp32 exactly; the arithmetic is that of libmemc_hip_lp.so's kernels (the fp32 kernels' tap
 *     products, quadrant sums and bilinear blend, in their order); the blend is two products and one sum;
 *   - nothing is rounded: the output is the fp32 value;
 *   - sites whose target is outside the image copy the input pixel;
 *   - every output element is assigned (no zero fill needed); no atomics: results are bit-reproducible.
 *
 * Coverage (return 1 outside it): C == 3, 16 taps (fs == 4), a width that is a multiple of four from 8 on, every plane
 * within 32-bit byte offsets; T tensors with row / channel / batch strides that are multiples of four elements and 8-byte
 * aligned bases (those of libmemc_hip_lp.so's tiled kernels); fp32 tensors need dword alignment only, as in libmemc_hip.so.
 * There is no kernel for other shapes: the caller promotes such a call to fp32, as it did before this library existed.
 *
 * Layout: NCHW, element strides (int64, memc_tensor4 of include/memc_warp.h), w-stride 1; the output has the image's
 * layout; in the blend both directions' tensors share their layouts and the occlusions are [B, 1, H, W].
 *
 * Return: 0 enqueued (an empty batch launches nothing and returns 0); 1 a well-formed call outside the coverage above --
 * nothing is touched or enqueued; -1 a failed descriptor check (before the device is touched: a tap dtype that is not
 * F16 / BF16, a flow dtype that is neither F32 nor the taps', mismatched shapes or layouts, a tap count that is not a
 * square, an occlusion that is not [B, 1, H, W], null data, a w-stride other than 1, strides beyond int32) or a launch
 * error.  Work is enqueued asynchronously on `stream`; nothing is allocated or kept, so a call can be captured in a graph.
 */
#ifndef MEMC_WARP_MX_H
#define MEMC_WARP_MX_H

#include "memc_warp_lp.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Library / build identification: "memc_hip_mx 0.1 gfx950". */
const char *memc_mx_version(void);

/* Kernel family of the most recent enqueued call made BY THE CALLING THREAD: "fi_fwd_mx:tiled_c3" or
 * "fi_blend_mx:tiled_c3"; "" before the first enqueued call (a declined or rejected call does not change it). */
const char *memc_mx_last_kernel_path(void);

/* output (fp32) = FilterInterpolation(input1 (fp32), input2 (flow, flow_dtype), input3 (taps, tap_dtype)). */
int FilterInterpolationLayer_gpu_forward_mx(memc_stream_t stream, memc_dtype tap_dtype, memc_dtype flow_dtype,
                                            const memc_tensor4 *input1, const memc_tensor4 *input2,
                                            const memc_tensor4 *input3, const memc_tensor4 *output);

/* output (fp32) = occlusion0 * FilterInterpolation(input0, flow0, filter0)
 *               + occlusion1 * FilterInterpolation(input2, flow1, filter1)
 * input0, input2: fp32; filter*, occlusion*: tap_dtype; flow*: flow_dtype. */
int FilterInterpolationBlendLayer_gpu_forward_mx(memc_stream_t stream, memc_dtype tap_dtype, memc_dtype flow_dtype,
                                                 const memc_tensor4 *input0, const memc_tensor4 *input2,
                                                 const memc_tensor4 *flow0, const memc_tensor4 *flow1,
                                                 const memc_tensor4 *filter0, const memc_tensor4 *filter1,
                                                 const memc_tensor4 *occlusion0, const memc_tensor4 *occlusion1,
                                                 const memc_tensor4 *output);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_WARP_MX_H */
