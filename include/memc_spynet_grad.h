/*
 * memc_spynet_grad.h -- C ABI of libmemc_hip_spynet_grad.so: the gradient of one SPyNet pyramid level's 8-channel input
 * (include/memc_spynet.h) with respect to the COARSE FLOW, in fp32, as one hand-written HIP kernel for gfx950 (MI355X).
 *
 * SPyNet's frames are data: in a training step only the coarse flow, which comes out of the previous level's convolutions,
 * wants a gradient.  A gradient for `first` is gradoutput[:, 0:3] (the caller slices it); `second` gets none here -- a caller
 * that needs one keeps torch's autograd.  So there is no image gradient, no scatter and no atomics.  A library of its own:
 * libmemc_hip_spynet.so is untouched by it.
 *
 * Tensors (fp32, NCHW, element strides; memc_tensor4 of include/memc_warp.h):
 *   second [B, 3, H, W], coarse [B, 2, h, w], gradoutput [B, 8, H, W] (channels 3..7 are read), gradcoarse [B, 2, h, w],
 *   each with its OWN b / c / h strides; H is 2h or 2h + 1, W is 2w or 2w + 1, H and W are at least 2.
 *
 * The rule, in the notation of memc_spynet.h, G = gradoutput.  Per fine site (x, y): up = (ux, uy) is recomputed from
 * `coarse` exactly as the forward computes it, and so are the position (px, py) with its clamp, the corners floor(p),
 * floor(p) + 1, their in-range tests and the weights ax = px - floor(px), bx = (floor(px) + 1) - px, ay, by.  X' is the
 * corner value of `second` where the corner lies inside the image, else 0:
 *
 *   dWc/dpx = by (NE' - NW') + ay (SE' - SW')          dWc/dpy = bx (SW' - NW') + ax (SE' - NE')
 *   gux = G[6] + kx' * sum_c G[3 + c] dWc/dpx           guy = G[7] + ky' * sum_c G[3 + c] dWc/dpy
 *   kx' = 1 under align_sample, else W / (W - 1); ky' likewise with H
 *
 * which is grid_sample's backward under zero padding (the one-sided derivative of floor) times the un-normalise / normalise
 * factors of the composed route.  A clamped position has no corner inside, so its warp term is 0.  Per coarse cell (i, j)
 * and channel c:
 *
 *   gradcoarse[c, i, j] = 2 * sum_y sum_x wy(y, i) wx(x, j) gu_c(y, x)
 *   wy(y, i) = (y0(y') == i ? l0 : 0) + (y1(y') == i ? l1 : 0),  y' = min(y, 2h - 1)
 *
 * with the forward's index rule (ATen's area_pixel_compute_source_index): a padded row or column adds its sites to the cells
 * of row 2h - 1 or column 2w - 1, an edge cell with y0 == y1 gets l0 + l1.
 *
 * Numerics contract: fp32 throughout; every element of gradcoarse ASSIGNED exactly once (it need not be zeroed); no atomics,
 * no workspace, owner-computes in a fixed summation order (rows outer, columns inner), so two calls on the same inputs give
 * the same bits.  The position is clamped into [-2, W + 1] x [-2, H + 1] before any conversion to int and a NaN position
 * counts as outside: no flow value, however large or non-finite, makes the kernel read outside `second`; the gradient a
 * non-finite flow yields is otherwise unspecified -- in the cells whose candidate sites (tests/_spynet_grad_spec.footprint)
 * it reaches; every other cell has the bits it has without it.
 *
 * Kernel family: "spynet_level_bwd:tiled" -- 256 lanes per workgroup, a tile of 16 x 16 coarse cells, the per-site gradients
 * of the tile's footprint (at most 39 x 39 fine sites, either upsampling mode) staged in 12 KiB of LDS.
 *
 * Return: 0 enqueued (B == 0 launches nothing and returns 0); 1 a well-formed call that is declined -- a plane beyond
 * 32-bit in-plane offsets ((h - 1) * row stride + w above INT32_MAX elements), a w-stride other than 1, `gradcoarse`
 * overlapping an input -- nothing is touched or enqueued;
 * -1 a failed descriptor check (before the device is touched: a null descriptor or data pointer, sizes or strides negative
 * or beyond int32, channel counts other than 3 / 2 / 8 / 2, mismatched batch or sizes, H or W below 2 or not 2h / 2h + 1,
 * 2w / 2w + 1), a tile whose footprint would exceed the staged box (no size does) or a launch error.  The classes are
 * checked in this order: malformed, empty, declined.  Work is enqueued asynchronously on `stream`; nothing is allocated or
 * kept, so a call can be captured in a graph.
 */
#ifndef MEMC_SPYNET_GRAD_H
#define MEMC_SPYNET_GRAD_H

#include "memc_warp_lp.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Library / build identification: "memc_hip_spynet_grad 0.1 gfx950". */
const char *memc_spynet_grad_version(void);

/* Kernel family of the most recent enqueued call made BY THE CALLING THREAD: "spynet_level_bwd:tiled"; "" before the first
 * enqueued call (a declined or rejected call does not change it). */
const char *memc_spynet_grad_last_kernel_path(void);

int SpyNetLevelLayer_gpu_backward(memc_stream_t stream, const memc_tensor4 *second, const memc_tensor4 *coarse,
                                  const memc_tensor4 *gradoutput, const memc_tensor4 *gradcoarse, int align_upsample,
                                  int align_sample);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif

#endif /* MEMC_SPYNET_GRAD_H */
