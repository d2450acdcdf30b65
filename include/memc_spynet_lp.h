/*
 * memc_spynet_lp.h -- C ABI of libmemc_hip_spynet_lp.so: the input of one SPyNet pyramid level on fp16 / bf16 tensors -- the
 * coarser flow upsampled x2 and doubled, the second frame warped with it, and both concatenated behind the first frame --
 * as one hand-written HIP kernel for gfx950 (MI355X).
 *
 * This is the step the flow estimator (SPyNet) of a MEMC_Net_s cast to bfloat16 / float16 runs at each of up to six pyramid
 * levels and in both directions.  A library of its own: libmemc_hip_spynet.so (include/memc_spynet.h, fp32) is untouched by
 * it.
 *
 * Tensors (ALL of one dtype T, MEMC_F16 or MEMC_BF16; NCHW, element strides; memc_tensor4 of include/memc_warp.h, `data`
 * the device pointer of the T elements):
 *   first [B, 3, H, W], second [B, 3, H, W], coarse [B, 2, h, w], out [B, 8, H, W], each with its OWN b / c / h strides;
 *   H is 2h or 2h + 1, W is 2w or 2w + 1, H and W are at least 2.
 *
 * Semantics: SpyNetLevelLayer_gpu_forward's (include/memc_spynet.h), with `align_upsample` and `align_sample` as there.
 *
 * Numerics contract:
 *   - every input is widened to fp32 exactly; the arithmetic is the fp32 kernel's, in the fp32 kernel's order (one text:
 *     memc_spynet_level.hpp); the sample position is formed in fp32 from the integer site index and the UNROUNDED fp32
 *     upsampled flow -- no position, grid or normalised flow is ever held in T;
 *   - out[:, 3:6] and out[:, 6:8] are rounded to T once, round-to-nearest-even, overflow to +-inf, exactly as torch's
 *     `tensor.to(T)`; out[:, 0:3] is a copy of first's 16-bit patterns (a NaN keeps its payload);
 *   - so `out` equals, bit for bit, SpyNetLevelLayer_gpu_forward on the widened inputs followed by one `.to(T)`, for the
 *     same kernel family;
 *   - every element of `out` is assigned exactly once, no atomics, no workspace.  The position is clamped into
 *     [-2, W + 1] x [-2, H + 1] before any conversion to int and a NaN position counts as outside: no flow value, however
 *     large or non-finite, makes the kernel read outside `second`; the warped value for a non-finite flow is otherwise
 *     unspecified (up and first are still exact).
 *
 * Kernel families: "spynet_level_lp:quad", four consecutive sites per lane with 8-byte loads of `first` and 8-byte stores,
 * for widths that are a multiple of four from 8 on, 8-byte aligned bases of `first` and `out` and b / c / h strides of those
 * two that are multiples of four elements (`second` and `coarse` are gathered element by element: no such condition);
 * "spynet_level_lp:direct", one lane per site, for every other call.
 *
 * Return: 0 enqueued (B == 0 launches nothing and returns 0); 1 a well-formed call that is declined -- a w-stride other
 * than 1, a plane beyond 32-bit in-plane offsets ((h - 1) * row stride + w above INT32_MAX elements), `out` overlapping an
 * input (byte spans of 2-byte elements) -- nothing is touched or enqueued;
 * -1 a failed descriptor check (before the device is touched: a dtype other than MEMC_F16 / MEMC_BF16, a null descriptor or
 * data pointer, sizes or strides negative or beyond int32, channel counts other than 3 / 3 / 2 / 8, mismatched batch or
 * sizes, H or W below 2 or not 2h / 2h + 1, 2w / 2w + 1) or a launch error.  Work is enqueued asynchronously on `stream`;
 * nothing is allocated or kept, so a call can be captured in a graph.
 */
#ifndef MEMC_SPYNET_LP_H
#define MEMC_SPYNET_LP_H

#include "memc_warp_lp.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Library / build identification: "memc_hip_spynet_lp 0.1 gfx950". */
const char *memc_spynet_lp_version(void);

/* Kernel family of the most recent enqueued call made BY THE CALLING THREAD: "spynet_level_lp:quad" or
 * "spynet_level_lp:direct"; "" before the first enqueued call (a declined or rejected call does not change it). */
const char *memc_spynet_lp_last_kernel_path(void);

int SpyNetLevelLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype dtype, const memc_tensor4 *first,
                                    const memc_tensor4 *second, const memc_tensor4 *coarse, const memc_tensor4 *out,
                                    int align_upsample, int align_sample);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_SPYNET_LP_H */
