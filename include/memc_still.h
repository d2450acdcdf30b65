/*
 * memc_still.h -- C ABI of libmemc_hip_still.so: the frame I/O and the scores of the still-image demo loop
 * (networks/png_io.py: interpolate_png_tree) on the GPU -- interleaved 8-bit RGB pictures of ANY height and width (odd ones
 * included) into the network's padded planar input, quantisation of its output back to such bytes, and the integer sums
 * behind the loop's mean absolute error and PSNR together with its difference picture -- hand-written HIP kernels for
 * gfx950 (MI355X).
 *
 * A library of its own: it shares no object and no symbol with libmemc_hip_video.so or any other library, takes plain
 * pointers and ints (no tensor descriptors) and includes no other header of this directory.
 *
 * dtype: a plain int, the values of memc_warp.h's memc_dtype -- 0 float32, 1 float16, 2 bfloat16; anything else -> -1.
 * T below is the storage type of `planes` that it names.
 *
 * Arithmetic: each rule is the host loop's, so that both routes give the same bytes and the same floats.
 *   decode   T(float32(byte) / 255.0f): the correctly rounded float32 division, then, for the 16-bit types, ONE
 *            round-to-nearest-even -- torch's (byte.float() / 255).to(T).  A padded element takes the value of the nearest
 *            pixel of the frame (clamped coordinates: replicate padding).
 *   quantise rintf(255.0f * clamp(float32(x), 0, 1)), ties to even, NaN -> 0, on the exactly widened value (the rule of
 *            memc_rgb_quantise / memc_rgb_quantise_lp).  quantise(decode(b)) = b for all 256 bytes in all three types.
 *   score    exact integers: per frame the sums of |a - b| and (a - b)^2 over its 3 h w samples, uint64, and the
 *            difference picture (128 + a - b) mod 256 per sample (png_io.rgb_scores').  No atomics: one partial pair per
 *            wave goes to the workspace and a final pass adds them, so the same bits come out from run to run.  Every
 *            accumulator that outlives one 16-sample trip is 64 bits wide: the sums are exact for every admitted frame,
 *            32768 x 32768 of 255 against 0 included.
 *
 * No pointer needs more than its element's alignment (bytes: none; float32 planes: 4; float16 / bfloat16 planes: 2; the
 * sums and the workspace: 8).  Rows and frames of the planes may start at any element; 3 h w may be odd, so the frames of
 * the byte tensors start on any byte; widths and pads need not be multiples of 4.
 *
 * The score's grid: at most MEMC_STILL_SCORE_MAX_BLOCKS workgroups of 256 lanes per frame (a lane takes 16 samples per
 * trip and strides over its frame), the frame is the grid's second dimension: at most MEMC_STILL_SCORE_MAX_FRAMES frames
 * per call.
 *
 * Every entry point takes the stream first, allocates nothing, synchronises nothing and keeps nothing between calls: work
 * is enqueued asynchronously on `stream`.  Return: 0 enqueued; -1 a failed check or a launch error, nothing enqueued.
 * The checks, in this order and before the device is touched (each entry point runs those that concern its arguments):
 *    1. frames < 0 -> -1;
 *    2. h or w non-positive or beyond 32768 -> -1;
 *    3. a dtype outside 0..2 -> -1;
 *    4. a negative pad, or one beyond 32768 -> -1;
 *    5. stride_frame or stride_c non-positive, or stride_row below the extent's width -> -1;
 *    6. for the score, frames beyond MEMC_STILL_SCORE_MAX_FRAMES -> -1;
 *    7. a workspace smaller than memc_rgb8_score_workspace_bytes' answer -> -1;
 *    8. frames == 0 -> 0, a no-op;
 *    9. a null pointer (diff_u8 excepted) -> -1;
 *   10. a `sums` or workspace pointer that is not 8-byte aligned -> -1.
 */
#ifndef MEMC_STILL_H
#define MEMC_STILL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* the score's grid: workgroups per frame, frames per call */
#define MEMC_STILL_SCORE_MAX_BLOCKS 1024
#define MEMC_STILL_SCORE_MAX_FRAMES 65535

/* a hipStream_t; NULL: the default stream */
typedef void *memc_still_stream_t;

/* Library / build identification, e.g. "memc_hip_still 0.1 gfx950". */
const char *memc_still_version(void);

/* uint8 RGB [frames, h, w, 3], contiguous -> planes: T [frames, 3, h + pad_top + pad_bottom, w + pad_left + pad_right] at
 * the given ELEMENT strides (w-stride 1): T(float32(byte) / 255), replicate-padded.  Every element of that extent is
 * assigned, by exactly one lane (a gather over the padded extent); nothing else is written. */
int memc_rgb8_decode(memc_still_stream_t stream, const uint8_t *rgb_u8, int frames, int h, int w, void *planes, int dtype,
                     int64_t stride_frame, int64_t stride_c, int64_t stride_row, int pad_left, int pad_right, int pad_top,
                     int pad_bottom);

/* T planes [frames, 3, h, w] at the given element strides (w-stride 1; `planes` points at the window's first element)
 * -> uint8 [frames, h, w, 3]: rintf(255.0f * clamp(float32(x), 0, 1)), ties to even.  NaN maps to 0. */
int memc_rgb8_quantise(memc_still_stream_t stream, const void *planes, int dtype, int64_t stride_frame, int64_t stride_c,
                       int64_t stride_row, int frames, int h, int w, uint8_t *rgb_u8);

/* Bytes of workspace memc_rgb8_score needs for these arguments: positive, a multiple of 8 and monotone in each of them
 * (frames == 0 answers as frames == 1); 0 where one of the checks 1, 2 and 6 fails. */
size_t memc_rgb8_score_workspace_bytes(int frames, int h, int w);

/* Per frame f of two uint8 RGB [frames, h, w, 3]: sums[2 f] = sum |a - b|, sums[2 f + 1] = sum (a - b)^2 over all 3 h w
 * samples, uint64.  diff_u8, where not NULL, receives the difference picture [frames, h, w, 3]: (128 + a - b) mod 256.
 * The workspace is scratch: uninitialised going in, meaningless coming out. */
int memc_rgb8_score(memc_still_stream_t stream, const uint8_t *rgb_a, const uint8_t *rgb_b, int frames, int h, int w,
                    uint64_t *sums, uint8_t *diff_u8, void *workspace, size_t workspace_bytes);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_STILL_H */
