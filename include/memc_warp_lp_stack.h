/*
 * memc_warp_lp_stack.h -- C ABI of libmemc_hip_lp_stack.so: the STACKED adaptive warp (FilterInterpolation) forward on
 * fp16 / bf16 tensors -- several neighbours' warps written straight into channel slices of one wider tensor -- hand-written
 * HIP kernels for gfx950 (MI355X).
 *
 * This is the call a MEMC_Net_VE cast to fp16 / bf16 makes: include/memc_warp_stack.h's, on half storage.  A library of
 * its own: libmemc_hip_stack.so (fp32) and libmemc_hip_lp.so (the half warp) are untouched by it, and each keeps its own
 * last kernel path.
 *
 * Tensors (NCHW, element strides, w-stride 1; memc_tensor4 of include/memc_warp.h; T = payload_dtype, MEMC_F16 or MEMC_BF16):
 *   input1 [N*B, C, H, W] of T, flow [N*B, 2, H, W] of flow_dtype (MEMC_F32 or T), taps [N*B, 16, H, W] of T:
 *   neighbour-major, row n * B + b is neighbour n of batch element b, N = n_neighbours;
 *   out [B, Ctot, H, W] of T: its OWN b / c / h strides.
 * Neighbour n of batch b, channel c, goes to out[b, c_base + slot(n) * C + c], slot(n) = n + (skip >= 0 && n >= skip): one
 * slot of C channels is left untouched for the unwarped centre; skip == -1 leaves none.  With flow_base >= 0 the two flow
 * planes are stored to out[b, flow_base + 2 * n + {0, 1}], with tap_base >= 0 the sixteen tap planes to
 * out[b, tap_base + 16 * n + k] (no slot is skipped there); -1: no such pass-through.
 *
 * Numerics contract: all arithmetic is fp32 on exactly widened inputs, in libmemc_hip.so's order, and every stored element
 * is rounded to T once (round-to-nearest-even, overflow to +-inf, as torch's `tensor.to(T)`) -- every warped element equals
 * FilterInterpolationLayer_gpu_forward_lp's (include/memc_warp_lp.h) on that neighbour's rows bit for bit; pass-through
 * values of type T are the values as read, bit for bit, and an fp32 flow is stored rounded to T once (`flow.to(T)`); sites
 * whose target is outside the image copy the input pixel; no atomics; every element of a written slice is assigned and
 * nothing else of `out` is touched.
 *
 * Coverage (return 1 outside it): C == 3, or C >= 4 with C % 4 == 0; 16 taps (fs == 4); a width that is a multiple of
 * four from 8 on; 8-byte aligned bases and strides that are multiples of four elements in every walked dimension (the
 * flow, fp32 or T, on the same test); every plane within 31-bit element offsets; every written slice inside [0, Ctot) and
 * the written slices pairwise disjoint.  There is no kernel for other calls: the caller composes them from
 * FilterInterpolationLayer_gpu_forward_lp.
 *
 * Return: 0 enqueued (an empty tensor launches nothing and returns 0); 1 a well-formed call outside the coverage above --
 * nothing is touched or enqueued; -1 a failed descriptor check (before the device is touched: a payload_dtype that is
 * neither MEMC_F16 nor MEMC_BF16, a flow_dtype that is neither MEMC_F32 nor the payload's, null data, a w-stride other than
 * 1, strides beyond int32, mismatched shapes, a tap count that is not a square, n_neighbours < 1 or not a divisor of
 * input1's rows, out's batch other than rows / n_neighbours, skip outside [-1, n_neighbours], a base below -1) or a launch
 * error.  Work is enqueued asynchronously on `stream`; nothing is allocated or kept, so a call can be captured in a graph.
 */
#ifndef MEMC_WARP_LP_STACK_H
#define MEMC_WARP_LP_STACK_H

#include "memc_warp_lp.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Library / build identification: "memc_hip_lp_stack 0.1 gfx950". */
const char *memc_lp_stack_version(void);

/* Kernel family of the most recent enqueued call made BY THE CALLING THREAD: "fi_fwd_stack_lp:tiled_c3" or
 * "fi_fwd_stack_lp:tiled_c4n"; "" before the first enqueued call (a declined or rejected call does not change it). */
const char *memc_lp_stack_last_kernel_path(void);

int FilterInterpolationStackLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype payload_dtype, memc_dtype flow_dtype,
                                                 const memc_tensor4 *input1, const memc_tensor4 *flow,
                                                 const memc_tensor4 *taps, const memc_tensor4 *out, int n_neighbours,
                                                 int c_base, int skip, int flow_base, int tap_base);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_WARP_LP_STACK_H */
