/*
 * memc_spynet.h -- C ABI of libmemc_hip_spynet.so: the input of one SPyNet pyramid level in fp32 -- the coarser flow
 * upsampled x2 and doubled, the second frame warped with it, and both concatenated behind the first frame -- as one
 * hand-written HIP kernel for gfx950 (MI355X).
 *
 * This is the step MEMC_Net_s's flow estimator (SPyNet) runs at each of up to six pyramid levels and in both directions.
 * Composed from F.interpolate, F.pad, the grid arithmetic, F.grid_sample and torch.cat it is nine or ten launches and
 * about 170 B moved per site; here every element of the level's 8-channel input is written once by one launch.  A library
 * of its own: libmemc_hip.so (include/memc_warp.h) is untouched by it.
 *
 * Tensors (fp32, NCHW, element strides; memc_tensor4 of include/memc_warp.h):
 *   first [B, 3, H, W], second [B, 3, H, W], coarse [B, 2, h, w], out [B, 8, H, W], each with its OWN b / c / h strides;
 *   H is 2h or 2h + 1, W is 2w or 2w + 1, H and W are at least 2.
 *
 *   out[:, 0:3] = first
 *   out[:, 6:8] = up = 2 * bilinear_x2(coarse): index and weights by ATen's area_pixel_compute_source_index with the scale
 *                 0.5, or (h - 1) / (2h - 1) under align_upsample, of the UNPADDED size 2h x 2w; where H == 2h + 1 row H - 1
 *                 repeats row 2h - 1, where W == 2w + 1 column W - 1 repeats column 2w - 1 (replicate padding)
 *   out[:, 3:6] = second sampled bilinearly (four corners, zero padding: a corner contributes only while it lies inside the
 *                 image) at the pixel position
 *                   align_sample != 0:  px = x + up_x,                      py = y + up_y
 *                   align_sample == 0:  px = (x + up_x) * W / (W - 1) - 0.5, py likewise with H
 *                 which is what linspace(-1, 1, W) + up / ((W - 1) / 2) means to grid_sample with and without align_corners.
 *
 * Numerics contract: fp32 throughout, every element of `out` assigned exactly once, no atomics, no workspace.  The position
 * is clamped into [-2, W + 1] x [-2, H + 1] before any conversion to int and a NaN position counts as outside: no flow
 * value, however large or non-finite, makes the kernel read outside `second`; the warped value for a non-finite flow is
 * otherwise unspecified (up and first are still exact).
 *
 * Kernel families: "spynet_level:quad", four consecutive sites per lane with 16-byte stores, for widths that are a multiple
 * of four from 8 on and dword-aligned bases; "spynet_level:direct", one lane per site, for every other call.
 *
 * Return: 0 enqueued (B == 0 launches nothing and returns 0); 1 a well-formed call that is declined -- a plane beyond
 * 32-bit in-plane offsets ((h - 1) * row stride + w above INT32_MAX elements), a w-stride other than 1, `out` overlapping
 * an input -- nothing is touched or enqueued;
 * -1 a failed descriptor check (before the device is touched: a null descriptor or data pointer, sizes or strides negative
 * or beyond int32, channel counts other than 3 / 3 / 2 / 8, mismatched batch or sizes, H or W below 2 or not 2h / 2h + 1,
 * 2w / 2w + 1) or a launch error.  Work is enqueued asynchronously on `stream`; nothing is allocated or kept, so a call can
 * be captured in a graph.
 */
#ifndef MEMC_SPYNET_H
#define MEMC_SPYNET_H

#include "memc_warp_lp.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Library / build identification: "memc_hip_spynet 0.1 gfx950". */
const char *memc_spynet_version(void);

/* Kernel family of the most recent enqueued call made BY THE CALLING THREAD: "spynet_level:quad" or "spynet_level:direct";
 * "" before the first enqueued call (a declined or rejected call does not change it). */
const char *memc_spynet_last_kernel_path(void);

int SpyNetLevelLayer_gpu_forward(memc_stream_t stream, const memc_tensor4 *first, const memc_tensor4 *second,
                                 const memc_tensor4 *coarse, const memc_tensor4 *out, int align_upsample, int align_sample);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_SPYNET_H */
