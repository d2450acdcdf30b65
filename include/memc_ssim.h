/*
 * memc_ssim.h -- C ABI of libmemc_hip_ssim.so: the third score of the HD demo loop (networks/yuv_io.py), the structural
 * similarity (SSIM) of two 8-bit planes -- hand-written HIP kernels for gfx950 (MI355X).
 *
 * A library of its own: it shares no object and no symbol with libmemc_hip.so, libmemc_hip_video.so or the satellite warp
 * libraries, takes plain pointers and ints and includes no other header of this directory.
 *
 * The number is skimage's compare_ssim at its defaults for two uint8 planes X, Y of h x w: 7 x 7 uniform window (n = 49),
 * sample covariance (n / (n - 1)), K1 = 0.01, K2 = 0.03, data range 255, the mean of the SSIM map over the interior
 * (cropped by 3 on every side: N = (h - 6)(w - 6) windows, so no border rule enters).  On bytes the five window sums are
 * exact integers, and the map is a quotient of small exact integers (csrc/memc_ssim_math.hpp):
 *   Vxx = 49 sxx - sx^2,  Vyy = 49 syy - sy^2,  Vxy = 49 sxy - sx sy
 *   S = ((2 sx sy + c1) (2 Vxy + c2)) / ((sx^2 + sy^2 + c1) (Vxx + Vyy + c2))
 *   c1 = (0.01 * 255)^2 * 49^2,  c2 = (0.03 * 255)^2 * 49 * 48
 * evaluated in float64 from int32 terms.  SSIM = (sum of S) / N in float64, summed in a fixed order: per-wave partials go
 * to the workspace and a final pass adds them, no atomics -- the same bits from run to run.  Equal planes give every
 * S = 1.0 and SSIM == 1.0 exactly.
 *
 * No pointer needs more than its element's alignment (bytes: none; the results and the workspace: 8); rows and frames of
 * the planes may start at any byte.  Odd h and w are allowed.
 *
 * Every entry point takes the stream first, allocates nothing, synchronises nothing and keeps nothing between calls: work
 * is enqueued asynchronously on `stream`.  Return: 0 enqueued; -1 a failed check or a launch error, nothing enqueued.
 * The checks, in this order and before the device is touched: frames < 0, h or w below 7 or beyond 32768, frames > 65535
 * (or a grid beyond 2^31 lanes), a stride that cannot hold the extent (or beyond 2^46), a workspace smaller than
 * memc_ssim_workspace_bytes -> -1; frames == 0 -> 0, a no-op; a null pointer, or an `ssim` or workspace pointer that is
 * not 8-byte aligned -> -1.
 */
#ifndef MEMC_SSIM_H
#define MEMC_SSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* a hipStream_t; NULL: the default stream */
typedef void *memc_ssim_stream_t;

/* Library / build identification, e.g. "memc_hip_ssim 0.1 gfx950". */
const char *memc_ssim_version(void);

/* Bytes of workspace either entry point needs for these arguments: positive, a multiple of 8 and monotone in each of
 * them; 0 where a check of the header's list fails. */
size_t memc_ssim_workspace_bytes(int frames, int h, int w);

/* Per frame f of two uint8 planes [frames, h, w] at the given BYTE strides (w-stride 1; the frame stride is ignored for
 * one frame): ssim[f] = their SSIM.  The workspace is scratch: uninitialised going in, meaningless coming out. */
int memc_ssim_u8(memc_ssim_stream_t stream, const uint8_t *a, const uint8_t *b, int64_t stride_frame, int64_t stride_row,
                 int frames, int h, int w, double *ssim, void *workspace, size_t workspace_bytes);

/* Per frame f of two contiguous uint8 RGB [frames, h, w, 3]: ssim[f] = the SSIM of their truncated 8-bit luma planes (the
 * Y of memc_i420_encode and memc_luma_score in memc_video.h), which are formed in the workspace first. */
int memc_ssim_luma_rgb(memc_ssim_stream_t stream, const uint8_t *rgb_a, const uint8_t *rgb_b, int frames, int h, int w,
                       double *ssim, void *workspace, size_t workspace_bytes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_SSIM_H */
