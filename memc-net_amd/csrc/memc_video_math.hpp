// memc_video_math.hpp -- the per-pixel arithmetic of video_io.hip (libmemc_hip_video.so): networks/yuv_io.py's float64 rule,
// plain C++ that a host compiler takes as well (tests/test_video_abi.py runs it beside numpy on the host; the kernels are
// held to numpy's bytes over all 2^24 triples by tests/test_gpu_video_io.py).
//
// The rule (yuv_io.py: Yuv420Reader.read, Yuv420Writer.write, luma_scores):
//   decode   y/255, u/255 - 0.5, v/255 - 0.5 through RGB_FROM_YUV, clipped to [0, 1], times 255, truncated;
//   encode   r/255, g/255, b/255 through YUV_FROM_RGB; Y = 255 y truncated, U and V = 255 clip(c + 0.5, 0, 1) truncated.
// A row of either matrix times the triple is numpy's matmul chain  fma(m2, c, fma(m1, b, m0 * a)).  Decode, U and V give
// the same bytes under every summation order; Y does not (5704 of the 2^24 RGB triples move by one level between orders),
// so the chain is written with explicit fma and nothing else here may be contracted or re-associated:
// FP contraction is off for the whole file (a compiler that fused 255 * y into the chain would change bytes).
// Division by 255 is the correctly rounded IEEE division of both compilers' defaults, never a multiplication by a reciprocal.
#ifndef MEMC_VIDEO_MATH_HPP
#define MEMC_VIDEO_MATH_HPP

#include <cmath>
#include <cstdint>

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif

#if defined(__HIPCC__)
#define MEMC_VIDEO_FN __host__ __device__ __forceinline__
#else
#define MEMC_VIDEO_FN inline
#endif

namespace memc_video {

// yuv_io.YUV_FROM_RGB (skimage.color's yuv_from_rgb) and its numpy.linalg.inv, bit for bit (row-major)
constexpr double kYuvFromRgb[9] = {
    0x1.322d0e5604189p-2, 0x1.2c8b439581062p-1, 0x1.d2f1a9fbe76c9p-4,      //  0.299       0.587       0.114
    -0x1.2d585c378e61bp-3, -0x1.27cd512c178b1p-2, 0x1.be797f47debbep-2,    // -0.14714119 -0.28886916  0.43601035
    0x1.3ade0d91e3edap-1, -0x1.07a98219f6206p-1, -0x1.99a45bbf6e6a7p-4};   //  0.61497538 -0.51496512 -0.10001026
constexpr double kRgbFromYuv[9] = {
    0x1.0000000000001p+0, -0x1.1f703ccd284c1p-28, 0x1.23cf5fce19d41p+0,
    0x1.0000000000000p+0, -0x1.941d1eb7a0ea5p-2, -0x1.2947445f678e0p-1,
    0x1.0000000000001p+0, 0x1.041a9a51ae08ap+1, -0x1.503fad3171755p-30};

MEMC_VIDEO_FN double row3(const double *m, double a, double b, double c)
{
    return fma(m[2], c, fma(m[1], b, m[0] * a));
}

MEMC_VIDEO_FN double clip01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

// 255 x for x in [0, 1 + a few ulp], truncated (numpy's astype(uint8) of such a value)
MEMC_VIDEO_FN uint8_t level(double x) { return (uint8_t)(int)(255.0 * x); }

MEMC_VIDEO_FN void decode_pixel(uint8_t y, uint8_t u, uint8_t v, uint8_t (&rgb)[3])
{
    const double yd = (double)y / 255.0, ud = (double)u / 255.0 - 0.5, vd = (double)v / 255.0 - 0.5;
    for (int c = 0; c < 3; c++) rgb[c] = level(clip01(row3(kRgbFromYuv + 3 * c, yd, ud, vd)));
}

MEMC_VIDEO_FN uint8_t luma_of(uint8_t r, uint8_t g, uint8_t b)
{
    return level(row3(kYuvFromRgb, (double)r / 255.0, (double)g / 255.0, (double)b / 255.0));
}

MEMC_VIDEO_FN void chroma_of(uint8_t r, uint8_t g, uint8_t b, uint8_t &u, uint8_t &v)
{
    const double rd = (double)r / 255.0, gd = (double)g / 255.0, bd = (double)b / 255.0;
    u = level(clip01(row3(kYuvFromRgb + 3, rd, gd, bd) + 0.5));
    v = level(clip01(row3(kYuvFromRgb + 6, rd, gd, bd) + 0.5));
}

// rintf(255 clamp(x, 0, 1)): numpy's round (ties to even) of the float32 product; NaN -> 0
MEMC_VIDEO_FN uint8_t quantise(float x) { return (uint8_t)(int)rintf(255.0f * fminf(fmaxf(x, 0.0f), 1.0f)); }

}  // namespace memc_video

#endif  // MEMC_VIDEO_MATH_HPP
