// lp_video_io.hip -- the frame I/O of the HD demo loop (networks/yuv_io.py) for a network in float16 / bfloat16, for gfx950:
// the kernels and the C ABI of libmemc_hip_video_lp.so (include/memc_video_lp.h).  One translation unit, nothing shared with
// the other libraries (of libmemc_hip_video.so it includes memc_video_math.hpp, the arithmetic, as it is).
//
// Two streaming kernels in video_io.hip's lane scheme; a lane takes four horizontally adjacent pixels of one row, no LDS:
//   i420_decode_lp<T>   a gather over the PADDED extent: lane (frame, padded row, quad of padded columns) clamps its source
//                       coordinates (replicate padding), decodes, stores T(float32(byte) / 255) into the three planes and, for
//                       the pixels inside the frame, the RGB bytes.  Every element has one writer.
//   rgb_quantise_lp<T>  three quads of T in, twelve bytes out, mv::quantise on the exactly widened value.
// T is a storage tag (F16, BF16): 16 bits in memory, converted in registers.  float32 -> T is ONE round-to-nearest-even of the
// correctly rounded float32 quotient (torch's (byte.float() / 255).to(T)); T -> float32 is exact.
// Memory: a row of a plane may start on an odd element, so four T move through u16x4u, a vector type of alignment 2 (the
// queues run in unaligned-access mode, as for video_io.hip's f32x4u); bytes through vector types of alignment 1.
#include <hip/hip_runtime.h>

#include "memc_video_math.hpp"
#include "memc_video_lp.h"

#pragma clang fp contract(off)

namespace memc {

namespace mv = memc_video;

typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
typedef u16x4 u16x4u __attribute__((aligned(2)));
typedef uint8_t u8x4 __attribute__((ext_vector_type(4)));
typedef u8x4 u8x4u __attribute__((aligned(1)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef u32x3 u32x3u __attribute__((aligned(1)));

constexpr int kThreads = 256;
constexpr int kMaxDim = 32768;
constexpr int kFloat16 = 1, kBFloat16 = 2;         // memc_dtype's values

// IEEE binary16: the compiler's conversions (v_cvt_f16_f32 rounds to nearest even; widening is exact)
struct F16 {
    static __device__ __forceinline__ uint16_t narrow(float x) { return __builtin_bit_cast(uint16_t, (_Float16)x); }
    static __device__ __forceinline__ float widen(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
};

// bfloat16: the upper half of a float32; round to nearest even on the 16 bits dropped, NaN kept quiet
struct BF16 {
    static __device__ __forceinline__ uint16_t narrow(float x)
    {
        const uint32_t u = __builtin_bit_cast(uint32_t, x);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
        return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
    static __device__ __forceinline__ float widen(uint16_t b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }
};

// twelve RGB bytes of four pixels
union Rgb4 {
    u32x3 v;
    uint8_t b[12];
};

__device__ __forceinline__ void store_rgb4(uint8_t *p, int count, const Rgb4 &q)
{
    if (count == 4) {
        *reinterpret_cast<u32x3u *>(p) = q.v;
    } else {
        for (int i = 0; i < 3 * count; i++) p[i] = q.b[i];
    }
}

// lane -> (frame, row, first column of the quad) of an extent of `rows` x `qpr` quads per frame; false past the end
__device__ __forceinline__ bool quad_of_lane(int frames, int rows, int qpr, int &f, int &y, int &x0)
{
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)frames * rows * qpr) return false;
    const int64_t row = idx / qpr;
    x0 = 4 * (int)(idx - row * qpr);
    f = (int)(row / rows);
    y = (int)(row - (int64_t)f * rows);
    return true;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void i420_decode_lp(const uint8_t *__restrict__ i420, int frames, int h, int w,
                                                           uint8_t *__restrict__ rgb, uint16_t *__restrict__ planes,
                                                           int64_t sf, int64_t sc, int64_t sr, int pl, int pt, int hp, int wp)
{
    int f, yp, xp0;
    if (!quad_of_lane(frames, hp, (wp + 3) / 4, f, yp, xp0)) return;
    const int count = min(4, wp - xp0);
    const int64_t ny = (int64_t)h * w, nc = (int64_t)(h / 2) * (w / 2);
    const uint8_t *Y = i420 + (int64_t)f * (ny + 2 * nc), *U = Y + ny, *V = U + nc;
    const int oy = yp - pt, sy = min(max(oy, 0), h - 1);
    const int ox0 = xp0 - pl;
    const uint8_t *yrow = Y + (int64_t)sy * w;
    const int64_t crow = (int64_t)(sy / 2) * (w / 2);
    const bool inside = ox0 >= 0 && ox0 + 3 < w && count == 4;     // four source columns, none clamped

    uint8_t yb[4];
    if (inside) {
        const u8x4 y4 = *reinterpret_cast<const u8x4u *>(yrow + ox0);
        for (int j = 0; j < 4; j++) yb[j] = y4[j];
    } else {
        for (int j = 0; j < 4; j++) yb[j] = yrow[min(max(ox0 + j, 0), w - 1)];     // j >= count: a valid address, unused
    }
    Rgb4 q;
    for (int j = 0; j < 4; j++) {
        const int sx = min(max(ox0 + j, 0), w - 1);
        uint8_t px[3];
        mv::decode_pixel(yb[j], U[crow + sx / 2], V[crow + sx / 2], px);
        for (int c = 0; c < 3; c++) q.b[3 * j + c] = px[c];
    }
    if (planes) {
        uint16_t *o = planes + f * sf + yp * sr + xp0;
        for (int c = 0; c < 3; c++, o += sc) {
            if (count == 4) {
                u16x4 v;
                for (int j = 0; j < 4; j++) v[j] = T::narrow((float)q.b[3 * j + c] / 255.0f);
                *reinterpret_cast<u16x4u *>(o) = v;
            } else {
                for (int j = 0; j < count; j++) o[j] = T::narrow((float)q.b[3 * j + c] / 255.0f);
            }
        }
    }
    if (rgb && oy >= 0 && oy < h) {
        uint8_t *o = rgb + (((int64_t)f * h + oy) * w + ox0) * 3;
        if (inside) {
            store_rgb4(o, 4, q);
        } else {
            for (int j = 0; j < count; j++) {
                if (ox0 + j < 0 || ox0 + j >= w) continue;
                for (int c = 0; c < 3; c++) o[3 * j + c] = q.b[3 * j + c];
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void rgb_quantise_lp(const uint16_t *__restrict__ planes, int64_t sf, int64_t sc,
                                                            int64_t sr, int frames, int h, int w, uint8_t *__restrict__ rgb)
{
    int f, y, x0;
    if (!quad_of_lane(frames, h, (w + 3) / 4, f, y, x0)) return;
    const int count = min(4, w - x0);
    const uint16_t *p = planes + f * sf + y * sr + x0;
    Rgb4 q;
    q.v = u32x3{0u, 0u, 0u};
    for (int c = 0; c < 3; c++, p += sc) {
        if (count == 4) {
            const u16x4 v = *reinterpret_cast<const u16x4u *>(p);
            for (int j = 0; j < 4; j++) q.b[3 * j + c] = mv::quantise(T::widen(v[j]));
        } else {
            for (int j = 0; j < count; j++) q.b[3 * j + c] = mv::quantise(T::widen(p[j]));
        }
    }
    store_rgb4(rgb + (((int64_t)f * h + y) * w + x0) * 3, count, q);
}

// ---- host side -------------------------------------------------------------------------------------------------------

static bool dims_ok(int frames, int h, int w)
{
    return frames >= 0 && h > 0 && w > 0 && !(h & 1) && !(w & 1) && h <= kMaxDim && w <= kMaxDim;
}

static bool dtype_ok(int dtype) { return dtype == kFloat16 || dtype == kBFloat16; }

// blocks of kThreads lanes for `lanes` lanes; 0 where the grid would not fit
static unsigned grid_for(int64_t lanes)
{
    const int64_t blocks = (lanes + kThreads - 1) / kThreads;
    return blocks > 0x7fffffffLL ? 0u : (unsigned)blocks;
}

static int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }

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
    if (pad_left < 0 || pad_right < 0 || pad_top < 0 || pad_bottom < 0) return -1;
    if (pad_left > kMaxDim || pad_right > kMaxDim || pad_top > kMaxDim || pad_bottom > kMaxDim) return -1;
    const int hp = h + pad_top + pad_bottom, wp = w + pad_left + pad_right;
    if (planes && (stride_frame <= 0 || stride_c <= 0 || stride_row < wp)) return -1;
    if (frames == 0) return 0;
    if (!i420 || (!rgb_u8 && !planes)) return -1;
    const unsigned grid = grid_for((int64_t)frames * hp * ((wp + 3) / 4));
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
    if (stride_frame <= 0 || stride_c <= 0 || stride_row < w) return -1;
    if (frames == 0) return 0;
    if (!planes || !rgb_u8) return -1;
    const unsigned grid = grid_for((int64_t)frames * h * ((w + 3) / 4));
    if (!grid) return -1;
    auto kernel = dtype == kFloat16 ? rgb_quantise_lp<F16> : rgb_quantise_lp<BF16>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, static_cast<const uint16_t *>(planes),
                       stride_frame, stride_c, stride_row, frames, h, w, rgb_u8);
    return launched();
}

}  // extern "C"
