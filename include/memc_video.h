/*
 * memc_video.h -- C ABI of libmemc_hip_video.so: the frame I/O of the HD demo loop (networks/yuv_io.py) on the GPU --
 * planar YUV 4:2:0 (I420) decode into the network's padded input, quantisation of its output, I420 encode and the luma
 * scores -- hand-written HIP kernels for gfx950 (MI355X).
 *
 * A library of its own: it shares no object and no symbol with libmemc_hip.so or the satellite warp libraries, takes
 * plain pointers and ints (no tensor descriptors) and includes no other header of this directory.
 *
 * Arithmetic: yuv_io.py's, in float64 on the device (csrc/memc_video_math.hpp):
 *   decode   y/255, u/255 - 0.5, v/255 - 0.5 (chroma taken at [row / 2, col / 2]) through RGB_FROM_YUV, clipped to
 *            [0, 1], times 255, truncated;
 *   encode   r/255, g/255, b/255 through YUV_FROM_RGB; Y = 255 y truncated; U and V = 255 clip(c + 0.5, 0, 1)
 *            truncated, sampled at even rows and even columns;
 *   a matrix row times the triple is  fma(m2, c, fma(m1, b, m0 * a)),  numpy's matmul chain: decode, U and V give the
 *   same bytes under every summation order, Y differs by one level at 0.034 % of the RGB triples between orders.
 *   Divisions by 255 are correctly rounded divisions.
 *
 * An I420 frame of h x w (both even) is h*w bytes of Y, then (h/2)*(w/2) of U, then of V: h*w*3/2 bytes; frames follow
 * each other without padding.  No pointer needs more than its element's alignment (bytes: none; float32: 4; the sums and
 * the workspace: 8); widths need not be multiples of 4.
 *
 * Every entry point takes the stream first, allocates nothing, synchronises nothing and keeps nothing between calls: work
 * is enqueued asynchronously on `stream`.  Return: 0 enqueued; -1 a failed check or a launch error, nothing enqueued.
 * The checks, in this order and before the device is touched: frames < 0, odd or non-positive h or w (or beyond 32768),
 * negative pads, non-positive strides, a workspace smaller than memc_luma_score_workspace_bytes -> -1;
 * frames == 0 -> 0, a no-op; a null pointer (or, for the sums and the workspace, one not 8-byte aligned) -> -1.
 */
#ifndef MEMC_VIDEO_H
#define MEMC_VIDEO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* a hipStream_t; NULL: the default stream */
typedef void *memc_video_stream_t;

/* Library / build identification, e.g. "memc_hip_video 0.1 gfx950". */
const char *memc_video_version(void);

/* `frames` consecutive I420 frames -> either or both of (both NULL: -1)
 *   rgb_u8  uint8 [frames, h, w, 3], contiguous;
 *   planes  float32 [frames, 3, h + pad_top + pad_bottom, w + pad_left + pad_right] at the given ELEMENT strides (w-stride
 *           1): float32(byte) / 255, replicate-padded.  Every element of that extent is assigned, by exactly one lane (a
 *           gather over the padded extent); nothing else is written.  The strides and pads are ignored when planes is NULL. */
int memc_i420_decode(memc_video_stream_t stream, const uint8_t *i420, int frames, int h, int w, uint8_t *rgb_u8,
                     float *planes, int64_t stride_frame, int64_t stride_c, int64_t stride_row, int pad_left, int pad_right,
                     int pad_top, int pad_bottom);

/* float32 planes [frames, 3, h, w] at the given element strides (w-stride 1; `planes` points at the window's first
 * element) -> uint8 [frames, h, w, 3]: rintf(255.0f * clamp(x, 0, 1)), ties to even.  NaN maps to 0. */
int memc_rgb_quantise(memc_video_stream_t stream, const float *planes, int64_t stride_frame, int64_t stride_c,
                      int64_t stride_row, int frames, int h, int w, uint8_t *rgb_u8);

/* uint8 RGB [frames, h, w, 3] -> `frames` consecutive I420 frames. */
int memc_i420_encode(memc_video_stream_t stream, const uint8_t *rgb_u8, int frames, int h, int w, uint8_t *i420);

/* Bytes of workspace memc_luma_score needs for these arguments: positive and monotone in each of them; 0 where a check
 * of the header's list fails. */
size_t memc_luma_score_workspace_bytes(int frames, int h, int w);

/* Per frame f of two uint8 RGB [frames, h, w, 3]: sums[2 f] = sum |Ya - Yb|, sums[2 f + 1] = sum (Ya - Yb)^2 over the
 * truncated 8-bit luma planes (the encode's Y), uint64.  Integer sums of per-wave partials and a final pass: no atomics,
 * the same bits from run to run.  The workspace is scratch: uninitialised going in, meaningless coming out. */
int memc_luma_score(memc_video_stream_t stream, const uint8_t *rgb_a, const uint8_t *rgb_b, int frames, int h, int w,
                    uint64_t *sums, void *workspace, size_t workspace_bytes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_VIDEO_H */
