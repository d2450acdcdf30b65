// memc_frame_io.hpp -- what the three frame I/O units (video_io.hip, lp_video_io.hip, still_io.hip) share, as text: vector
// types, storage tags, the lane scheme, the integer wave sum with the per-frame final pass, and the host checks of a launch
// over quads.  Internal to csrc: everything here is a type, a constant, a __forceinline__ device function or a static inline
// host function, so each library still holds its own copy of what it uses and exports no symbol of another
// (no __global__ function, nothing with external linkage).  Nothing of the I420 arithmetic: that is memc_frame_io_i420.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace memc {

// Rows, frames and plane offsets start on any byte / element, so vectors move through types of the element's alignment
// (the queues run in unaligned-access mode, as for memc_tile.hpp's f32x4u).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef f32x4 f32x4u __attribute__((aligned(4)));
typedef uint16_t u16x4 __attribute__((ext_vector_type(4)));
typedef u16x4 u16x4u __attribute__((aligned(2)));
typedef uint8_t u8x2 __attribute__((ext_vector_type(2)));
typedef uint8_t u8x4 __attribute__((ext_vector_type(4)));
typedef u8x2 u8x2u __attribute__((aligned(1)));
typedef u8x4 u8x4u __attribute__((aligned(1)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef u32x3 u32x3u __attribute__((aligned(1)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4u __attribute__((aligned(1)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxDim = 32768;
constexpr int kFloat32 = 0, kFloat16 = 1, kBFloat16 = 2;          // memc_dtype's values

// Storage tags: how a plane element lies in memory (elem; four of them, vec, and that vector at elem's alignment, vecu) and
// its conversions in registers.  float32 -> a 16-bit T is ONE round-to-nearest-even; T -> float32 is exact.
struct F32 {
    typedef float elem;
    typedef f32x4 vec;
    typedef f32x4u vecu;
    static __device__ __forceinline__ float narrow(float x) { return x; }
    static __device__ __forceinline__ float widen(float b) { return b; }
};

// IEEE binary16: the compiler's conversions (v_cvt_f16_f32 rounds to nearest even; widening is exact)
struct F16 {
    typedef uint16_t elem;
    typedef u16x4 vec;
    typedef u16x4u vecu;
    static __device__ __forceinline__ uint16_t narrow(float x) { return __builtin_bit_cast(uint16_t, (_Float16)x); }
    static __device__ __forceinline__ float widen(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }
};

// bfloat16: the upper half of a float32; round to nearest even on the 16 bits dropped, NaN kept quiet
struct BF16 {
    typedef uint16_t elem;
    typedef u16x4 vec;
    typedef u16x4u vecu;
    static __device__ __forceinline__ uint16_t narrow(float x)
    {
        const uint32_t u = __builtin_bit_cast(uint32_t, x);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
        return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
    static __device__ __forceinline__ float widen(uint16_t b) { return __builtin_bit_cast(float, (uint32_t)b << 16); }
};

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

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;                                      // lane 0 holds the wave's sum
}

// The body of a score's final pass: one wave (the workgroup) per frame adds its frame's `n` partial pairs.
__device__ __forceinline__ void add_partials(const unsigned long long *__restrict__ partial, int n,
                                             unsigned long long *__restrict__ sums)
{
    const unsigned long long *p = partial + (int64_t)blockIdx.x * n * 2;
    unsigned long long sabs = 0, ssq = 0;
    for (int i = threadIdx.x; i < n; i += 64) {
        sabs += p[2 * i];
        ssq += p[2 * i + 1];
    }
    sabs = wave_sum(sabs);
    ssq = wave_sum(ssq);
    if (threadIdx.x == 0) {
        sums[2 * blockIdx.x] = sabs;
        sums[2 * blockIdx.x + 1] = ssq;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------

// blocks of kThreads lanes for `lanes` lanes; 0 where the grid would not fit
static inline unsigned grid_for(int64_t lanes)
{
    const int64_t blocks = (lanes + kThreads - 1) / kThreads;
    return blocks > 0x7fffffffLL ? 0u : (unsigned)blocks;
}

// the grid of one lane per quad of `frames` extents of rows x cols
static inline unsigned quad_grid(int frames, int rows, int cols) { return grid_for((int64_t)frames * rows * ((cols + 3) / 4)); }

static inline int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }

static inline bool pad_ok(int p) { return p >= 0 && p <= kMaxDim; }

// (frame, channel, row) element strides of planes whose rows hold `cols` elements
static inline bool strides_ok(int64_t sf, int64_t sc, int64_t sr, int cols) { return sf > 0 && sc > 0 && sr >= cols; }

// The checks of a padded decode between its dimensions and its pointers: the four pads, then (where there are planes) that
// the strides hold the padded extent hp x wp, which it hands back.
static inline bool padded_extent_ok(int h, int w, int pl, int pr, int pt, int pb, bool planes, int64_t sf, int64_t sc,
                                    int64_t sr, int &hp, int &wp)
{
    if (!pad_ok(pl) || !pad_ok(pr) || !pad_ok(pt) || !pad_ok(pb)) return false;
    hp = h + pt + pb;
    wp = w + pl + pr;
    return !planes || strides_ok(sf, sc, sr, wp);
}

}  // namespace memc
