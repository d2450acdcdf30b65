/*
 * memc_warp_lp.h -- C ABI of libmemc_hip_lp.so: the adaptive-warp forward (FilterInterpolation) and the fused dual warp +
 * occlusion blend on fp16 / bf16 tensors, hand-written HIP kernels for gfx950 (MI355X).
 *
 * A separate library: libmemc_hip.so and include/memc_warp.h (fp32, the reference's contract) are untouched by it.
 *
 * Numerics contract:
 *   - payload dtype T (MEMC_F16 or MEMC_BF16): the image / features, the filter taps, the occlusions (blend) and the output
 *     are all of type T;
 *   - flow dtype: MEMC_F32 or T, decoded in the kernel;
 *   - all arithmetic is fp32: inputs are widened exactly; the tap products, the quadrant sums and the bilinear blend are
 *     those of the fp32 kernels of libmemc_hip.so, in the same order;
 *   - the output is rounded to T once, round-to-nearest-even; overflow goes to +-inf, exactly as torch's `tensor.to(T)`;
 *   - sites outside the image copy the input pixel (exact);
 *   - semantics are otherwise FilterInterpolationLayer_gpu_forward's (include/memc_warp.h), filter sizes other than 4 and
 *     small widths included.
 *
 * Layout: NCHW, element strides (int64, as memc_tensor4 of include/memc_warp.h; `data` is the device pointer of the T or
 * fp32 elements), w-stride 1; `output` has input1's layout.  The tiled kernels take fs == 4, widths that are a multiple of
 * four (from 8 on), row / channel / batch strides that are multiples of four elements and 8-byte aligned base pointers;
 * every other shape is served by a one-lane-per-site kernel (same results, slower): see memc_lp_last_kernel_path().
 *
 * Return: 0 on success (an empty batch launches nothing and returns 0), -1 on a failed descriptor check (before the device
 * is touched: wrong dtype enum, a flow dtype that is neither fp32 nor the payload's, mismatched shapes or layouts, strides
 * beyond int32) or a launch error.  Work is enqueued asynchronously on `stream`; nothing is allocated or kept.
 */
#ifndef MEMC_WARP_LP_H
#define MEMC_WARP_LP_H

#include "memc_warp.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef enum memc_dtype { MEMC_F32 = 0, MEMC_F16 = 1, MEMC_BF16 = 2 } memc_dtype;

/* Library / build identification, e.g. "memc_hip_lp 0.1 gfx950". */
const char *memc_lp_version(void);

/* Kernel family of the most recent call made BY THE CALLING THREAD: "fi_fwd_lp:tiled_c3", "fi_fwd_lp:tiled_c4n",
 * "fi_fwd_lp:direct", "fi_blend_lp:tiled_c3", "fi_blend_lp:direct"; "" before the first call. */
const char *memc_lp_last_kernel_path(void);

/* output = FilterInterpolation(input1, input2 (flow), input3 (fs*fs filter taps)); input1 / input3 / output of
 * payload_dtype, input2 of flow_dtype. */
int FilterInterpolationLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype payload_dtype, memc_dtype flow_dtype,
                                            const memc_tensor4 *input1, const memc_tensor4 *input2,
                                            const memc_tensor4 *input3, const memc_tensor4 *output);

/* output = occlusion0 * FilterInterpolation(input0, flow0, filter0) + occlusion1 * FilterInterpolation(input2, flow1, filter1),
 * computed in fp32 (two products, one sum) and rounded once.  input0 / input2 / output share one layout, flow0 / flow1
 * one, filter0 / filter1 one, occlusion0 / occlusion1 ([N, 1, H, W]) one.  Flows of flow_dtype, everything else of
 * payload_dtype. */
int FilterInterpolationBlendLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype payload_dtype, memc_dtype flow_dtype,
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

#endif /* MEMC_WARP_LP_H */
