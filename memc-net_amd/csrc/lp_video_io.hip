// lp_video_io.hip -- the frame I/O of the HD demo loop (networks/yuv_io.py) for a network in float16 / bfloat16, for gfx950:
// the kernels and the C ABI of libmemc_hip_video_lp.so (include/memc_video_lp.h).  One translation unit; no object and no
// symbol shared with the other libraries.  The lane scheme, the storage tags and the host checks are memc_frame_io.hpp's,
// shared as text with video_io.hip and still_io.hip; the quad's bytes and the kernels' bodies are memc_frame_io_i420.hpp's,
// with video_io.hip (of libmemc_hip_video.so it includes memc_video_math.hpp, the arithmetic, as it is).
//
// Two streaming kernels in video_io.hip's lane scheme; a lane takes four horizontally adjacent pixels of one row, no LDS:
//   i420_decode_lp<T>   i420_decode_body.inc on planes of T: a gather over the PADDED extent that stores
//                       T(float32(byte) / 255) into the three planes and, for the pixels inside the frame, the RGB bytes.
//   rgb_quantise_lp<T>  rgb_quantise_body.inc on planes of T: three quads of T in, twelve bytes out.
// T is a storage tag (F16, BF16): 16 bits in memory, converted in registers.  float32 -> T is ONE round-to-nearest-even of the
// correctly rounded float32 quotient (torch's (byte.float() / 255).to(T)); T -> float32 is exact.
// Memory: a row of a plane may start on an odd element, so four T move through u16x4u, a vector type of alignment 2 (the
// queues run in unaligned-access mode, as for video_io.hip's f32x4u); bytes through vector types of alignment 1.
#include "memc_frame_io_i420.hpp"
#include "memc_video_lp.h"

#pragma clang fp contract(off)

namespace memc {

template <typename T>
__global__ __launch_bounds__(kThreads) void i420_decode_lp(const uint8_t *__restrict__ i420, int frames, int h, int w,
                                                           uint8_t *__restrict__ rgb, uint16_t *__restrict__ planes,
                                                           int64_t sf, int64_t sc, int64_t sr, int pl, int pt, int hp, int wp)
{
#include "i420_decode_body.inc"
}

template <typename T>
__global__ __launch_bounds__(kThreads) void rgb_quantise_lp(const uint16_t *__restrict__ planes, int64_t sf, int64_t sc,
                                                            int64_t sr, int frames, int h, int w, uint8_t *__restrict__ rgb)
{
#include "rgb_quantise_body.inc"
}

// ---- host side -------------------------------------------------------------------------------------------------------

static bool dtype_ok(int dtype) { return dtype == kFloat16 || dtype == kBFloat16; }

}  // namespace memc

using namespace memc;

extern "C" {

const char *memc_video_lp_version(void) { return "memc_hip_video_lp 0.1 gfx950"; }

int memc_i420_decode_lp(memc_video_lp_stream_t stream, const uint8_t *i420, int frames, int h, int w, uint8_t *rgb_u8,
                        void *planes, int dtype, int64_t stride_frame, int64_t stride_c, int64_t stride_row, int pad_left,
                        int pad_right, int pad_top, int pad_bottom)
{
    if (!dims_ok(frames, h, w)) return -1;
    if (!dtype_ok(dtype)) return -1;
    if (!planes) pad_left = pad_right = pad_top = pad_bottom = 0;
    int hp, wp;
    if (!padded_extent_ok(h, w, pad_left, pad_right, pad_top, pad_bottom, planes != nullptr, stride_frame, stride_c, stride_row,
                          hp, wp))
        return -1;
    if (frames == 0) return 0;
    if (!i420 || (!rgb_u8 && !planes)) return -1;
    const unsigned grid = quad_grid(frames, hp, wp);
    if (!grid) return -1;
    auto kernel = dtype == kFloat16 ? i420_decode_lp<F16> : i420_decode_lp<BF16>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, i420, frames, h, w, rgb_u8,
                       static_cast<uint16_t *>(planes), stride_frame, stride_c, stride_row, pad_left, pad_top, hp, wp);
    return launched();
}

int memc_rgb_quantise_lp(memc_video_lp_stream_t stream, const void *planes, int dtype, int64_t stride_frame,
                         int64_t stride_c, int64_t stride_row, int frames, int h, int w, uint8_t *rgb_u8)
{
    if (!dims_ok(frames, h, w)) return -1;
    if (!dtype_ok(dtype)) return -1;
    if (!strides_ok(stride_frame, stride_c, stride_row, w)) return -1;
    if (frames == 0) return 0;
    if (!planes || !rgb_u8) return -1;
    const unsigned grid = quad_grid(frames, h, w);
    if (!grid) return -1;
    auto kernel = dtype == kFloat16 ? rgb_quantise_lp<F16> : rgb_quantise_lp<BF16>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, static_cast<const uint16_t *>(planes),
                       stride_frame, stride_c, stride_row, frames, h, w, rgb_u8);
    return launched();
}

}  // extern "C"
