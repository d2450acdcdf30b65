// memc_frame_io_i420.hpp -- what the two I420 units (video_io.hip, lp_video_io.hip) share beyond memc_frame_io.hpp: the
// twelve bytes of a quad, the dimension rule of an I420 frame, and (i420_decode_body.inc, rgb_quantise_body.inc) the bodies of
// their decode and quantise kernels.  The arithmetic is memc_video_math.hpp's (float64, explicit fma chain, contraction
// off).  still_io.hip does not include this: it uses none of the I420 arithmetic.
#pragma once
#include "memc_frame_io.hpp"
#include "memc_video_math.hpp"

namespace memc {

namespace mv = memc_video;

// twelve RGB bytes of four pixels, indexed by byte (still_io.hip's Rgb4 keeps them in dwords)
union Rgb4Bytes {
    u32x3 v;
    uint8_t b[12];
};

__device__ __forceinline__ void load_rgb4(const uint8_t *p, int count, Rgb4Bytes &q)
{
    if (count == 4) {
        q.v = *reinterpret_cast<const u32x3u *>(p);
    } else {
        q.v = u32x3{0u, 0u, 0u};
        for (int i = 0; i < 3 * count; i++) q.b[i] = p[i];
    }
}

__device__ __forceinline__ void store_rgb4(uint8_t *p, int count, const Rgb4Bytes &q)
{
    if (count == 4) {
        *reinterpret_cast<u32x3u *>(p) = q.v;
    } else {
        for (int i = 0; i < 3 * count; i++) p[i] = q.b[i];
    }
}

static inline bool dims_ok(int frames, int h, int w)
{
    return frames >= 0 && h > 0 && w > 0 && !(h & 1) && !(w & 1) && h <= kMaxDim && w <= kMaxDim;
}

}  // namespace memc
