/*
 * memc_video_lp.h -- C ABI of libmemc_hip_video_lp.so: the frame I/O of the HD demo loop (networks/yuv_io.py) for a network
 * that runs in float16 or bfloat16 -- planar YUV 4:2:0 (I420) decode into a padded input of that storage and quantisation of
 * an output of that storage -- hand-written HIP kernels for gfx950 (MI355X).  Encode and the scores work on bytes: they
 * are libmemc_hip_video.so's (memc_video.h) whatever the network's precision.
 *
 * A library of its own: it shares no object and no symbol with libmemc_hip_video.so or any other library, takes plain
 * pointers and ints (no tensor descriptors) and includes no other header of this directory.
 *
 * dtype: a plain int, the values of memc_warp.h's memc_dtype -- 1 float16, 2 bfloat16; anything else -> -1.
 *
 * Arithmetic (T the storage type):
 *   decode   the RGB bytes are memc_video.h's (float64, csrc/memc_video_math.hpp); a plane element is
 *            T(float32(byte) / 255.0f): the correctly rounded float32 division, then ONE round-to-nearest-even to T --
 *            torch's (byte.float() / 255).to(T);
 *   quantise rintf(255.0f * clamp(float32(x), 0, 1)), ties to even, NaN -> 0, on the exactly widened value.
 *   quantise(decode(b)) = b for all 256 bytes in both types.
 *
 * An I420 frame of h x w (both even) is h*w bytes of Y, then (h/2)*(w/2) of U, then of V: h*w*3/2 bytes; frames follow
 * each other without padding.  No pointer needs more than its element's alignment (bytes: none; planes: 2); rows may start
 * on an odd element; widths and pads need not be multiples of 4.
 *
 * Every entry point takes the stream first, allocates nothing, synchronises nothing and keeps nothing between calls: work
 * is enqueued asynchronously on `stream`.  Return: 0 enqueued; -1 a failed check or a launch error, nothing enqueued.
 * The checks, in this order and before the device is touched (memc_video.h's for the same arguments, the dtype second):
 * frames < 0, odd or non-positive h or w (or beyond 32768), a dtype that is neither 1 nor 2, negative pads, non-positive
 * strides -> -1; frames == 0 -> 0, a no-op; a null pointer -> -1.
 */
#ifndef MEMC_VIDEO_LP_H
#define MEMC_VIDEO_LP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* a hipStream_t; NULL: the default stream */
typedef void *memc_video_lp_stream_t;

/* Library / build identification, e.g. "memc_hip_video_lp 0.1 gfx950". */
const char *memc_video_lp_version(void);

/* `frames` consecutive I420 frames -> either or both of (both NULL: -1)
 *   rgb_u8  uint8 [frames, h, w, 3], contiguous: the bytes memc_i420_decode gives;
 *   planes  T [frames, 3, h + pad_top + pad_bottom, w + pad_left + pad_right] at the given ELEMENT strides (w-stride 1):
 *           T(float32(byte) / 255), replicate-padded.  Every element of that extent is assigned, by exactly one lane (a
 *           gather over the padded extent); nothing else is written.  The strides and pads are ignored when planes is NULL. */
int memc_i420_decode_lp(memc_video_lp_stream_t stream, const uint8_t *i420, int frames, int h, int w, uint8_t *rgb_u8,
                        void *planes, int dtype, int64_t stride_frame, int64_t stride_c, int64_t stride_row, int pad_left,
                        int pad_right, int pad_top, int pad_bottom);

/* T planes [frames, 3, h, w] at the given element strides (w-stride 1; `planes` points at the window's first element)
 * -> uint8 [frames, h, w, 3]: rintf(255.0f * clamp(float32(x), 0, 1)), ties to even.  NaN maps to 0. */
int memc_rgb_quantise_lp(memc_video_lp_stream_t stream, const void *planes, int dtype, int64_t stride_frame,
                         int64_t stride_c, int64_t stride_row, int frames, int h, int w, uint8_t *rgb_u8);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_VIDEO_LP_H */
