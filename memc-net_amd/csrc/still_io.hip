// still_io.hip -- the frame I/O and the scores of the still-image demo loop (networks/png_io.py) for gfx950: the kernels and
// the C ABI of libmemc_hip_still.so (include/memc_still.h).  One translation unit; no object and no symbol shared with the
// other libraries.  The storage tags, the lane scheme, the wave sum, the final pass's body and the host checks are
// memc_frame_io.hpp's, shared as text with video_io.hip and lp_video_io.hip; nothing of the I420 arithmetic comes with them.
//
// Three streaming kernels and a final pass, no LDS anywhere in this file:
//   rgb8_decode<T>    a gather over the PADDED extent: lane (frame, padded row, quad of padded columns) clamps its source
//                     coordinates (replicate padding), reads the twelve bytes of its four pixels and stores
//                     T(float32(byte) / 255) into the three planes.  Every element has one writer.
//   rgb8_quantise<T>  three quads of T in, twelve bytes out, quantise() on the exactly widened value.
//   rgb8_partial      a frame is a flat run of 3 h w samples; a lane takes 16 of them per trip and strides over its frame
//                     with its workgroup's grid; per lane uint64 sums of |a - b| and (a - b)^2, reduced over the wave by
//                     shuffles; one partial pair per WAVE goes to the workspace; the difference picture on the way.
//   rgb8_final        one wave per frame adds the partials.  Integer sums: no atomics, no order dependence.
// T is a storage tag (F32, F16, BF16).  float32 -> a 16-bit T is ONE round-to-nearest-even of the correctly rounded float32
// quotient (torch's (byte.float() / 255).to(T)); T -> float32 is exact.
// Memory: heights and widths are odd as often as not, so a row of the bytes and a frame of them start on any byte and a row
// of a plane on any element: bytes move through vector types of alignment 1, four T through a vector type of T's alignment
// (the queues run in unaligned-access mode, as for video_io.hip's f32x4u).
#include "memc_frame_io.hpp"
#include "memc_still.h"

#pragma clang fp contract(off)

namespace memc {

constexpr int kMaxScoreBlocks = MEMC_STILL_SCORE_MAX_BLOCKS;      // workgroups per frame of rgb8_partial
constexpr int kMaxScoreFrames = MEMC_STILL_SCORE_MAX_FRAMES;      // the frame is the grid's y
constexpr int kTrip = 16;                                         // samples of one lane's trip

// rintf(255 clamp(x, 0, 1)): numpy's round (ties to even) of the float32 product; NaN -> 0 (fmaxf returns the other operand)
__device__ __forceinline__ uint8_t quantise(float x) { return (uint8_t)(int)rintf(255.0f * fminf(fmaxf(x, 0.0f), 1.0f)); }

// N dwords of bytes in registers.  Every index below is a constant once its loop is unrolled, so the dwords stay in VGPRs:
// a byte array indexed by a run-time count would be placed in LDS or scratch by the compiler.
template <int N>
struct Bytes {
    uint32_t w[N];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int i = 0; i < N; i++) w[i] = 0u;
    }
    __device__ __forceinline__ uint32_t get(int i) const { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }
    __device__ __forceinline__ void put(int i, uint32_t b) { w[i >> 2] |= b << (8 * (i & 3)); }      // onto a cleared byte
    // `count` bytes from / to p, one by one (count <= 4 N)
    __device__ __forceinline__ void load_bytes(const uint8_t *p, int count)
    {
        clear();
#pragma unroll
        for (int i = 0; i < 4 * N; i++)
            if (i < count) put(i, p[i]);
    }
    __device__ __forceinline__ void store_bytes(uint8_t *p, int count) const
    {
#pragma unroll
        for (int i = 0; i < 4 * N; i++)
            if (i < count) p[i] = (uint8_t)get(i);
    }
};

// twelve RGB bytes of four pixels; sixteen samples of one trip
struct Rgb4 : Bytes<3> {
    __device__ __forceinline__ void load(const uint8_t *p)
    {
        const u32x3 v = *reinterpret_cast<const u32x3u *>(p);
        w[0] = v[0], w[1] = v[1], w[2] = v[2];
    }
    __device__ __forceinline__ void store(uint8_t *p) const { *reinterpret_cast<u32x3u *>(p) = u32x3{w[0], w[1], w[2]}; }
};

struct Run16 : Bytes<4> {
    __device__ __forceinline__ void load(const uint8_t *p)
    {
        const u32x4 v = *reinterpret_cast<const u32x4u *>(p);
        w[0] = v[0], w[1] = v[1], w[2] = v[2], w[3] = v[3];
    }
    __device__ __forceinline__ void store(uint8_t *p) const { *reinterpret_cast<u32x4u *>(p) = u32x4{w[0], w[1], w[2], w[3]}; }
};

template <typename T>
__global__ __launch_bounds__(kThreads) void rgb8_decode(const uint8_t *__restrict__ rgb, int frames, int h, int w,
                                                        typename T::elem *__restrict__ planes, int64_t sf, int64_t sc,
                                                        int64_t sr, int pl, int pt, int hp, int wp)
{
    int f, yp, xp0;
    if (!quad_of_lane(frames, hp, (wp + 3) / 4, f, yp, xp0)) return;
    const int count = min(4, wp - xp0);
    const int sy = min(max(yp - pt, 0), h - 1), ox0 = xp0 - pl;
    const uint8_t *row = rgb + ((int64_t)f * h + sy) * w * 3;
    Rgb4 q;
    if (ox0 >= 0 && ox0 + 3 < w) {                                 // four source columns, none clamped
        q.load(row + 3 * ox0);
    } else {
        q.clear();
#pragma unroll
        for (int j = 0; j < 4; j++) {                              // j >= count: a valid address, unused
            const uint8_t *p = row + 3 * min(max(ox0 + j, 0), w - 1);
#pragma unroll
            for (int c = 0; c < 3; c++) q.put(3 * j + c, p[c]);
        }
    }
    typename T::elem *o = planes + f * sf + yp * sr + xp0;
#pragma unroll
    for (int c = 0; c < 3; c++, o += sc) {
        typename T::vec v;
#pragma unroll
        for (int j = 0; j < 4; j++) v[j] = T::narrow((float)q.get(3 * j + c) / 255.0f);
        if (count == 4) {
            *reinterpret_cast<typename T::vecu *>(o) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (j < count) o[j] = v[j];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void rgb8_quantise(const typename T::elem *__restrict__ planes, int64_t sf, int64_t sc,
                                                          int64_t sr, int frames, int h, int w, uint8_t *__restrict__ rgb)
{
    int f, y, x0;
    if (!quad_of_lane(frames, h, (w + 3) / 4, f, y, x0)) return;
    const int count = min(4, w - x0);
    const typename T::elem *p = planes + f * sf + y * sr + x0;
    Rgb4 q;
    q.clear();
#pragma unroll
    for (int c = 0; c < 3; c++, p += sc) {
        typename T::vec v = {};
        if (count == 4) {
            v = *reinterpret_cast<const typename T::vecu *>(p);
        } else {
#pragma unroll
            for (int j = 0; j < 3; j++)
                if (j < count) v[j] = p[j];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) q.put(3 * j + c, quantise(T::widen(v[j])));      // j >= count: of a zero, not stored
    }
    uint8_t *o = rgb + (((int64_t)f * h + y) * w + x0) * 3;
    if (count == 4) q.store(o);
    else q.store_bytes(o, 3 * count);
}

// grid (blocks per frame, frames); partial[((f * gridDim.x + block) * kWaves + wave) * 2 + {0, 1}]; n = 3 h w samples a frame
__global__ __launch_bounds__(kThreads) void rgb8_partial(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                         int64_t n, uint8_t *__restrict__ diff,
                                                         unsigned long long *__restrict__ partial)
{
    const int f = blockIdx.y;
    const int64_t base = (int64_t)f * n, trips = (n + kTrip - 1) / kTrip;
    unsigned long long sabs = 0, ssq = 0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < trips; i += (int64_t)gridDim.x * kThreads) {
        const int64_t o = base + i * kTrip;
        const int count = (int)min((int64_t)kTrip, n - i * kTrip);
        Run16 ra, rb, rd;
        if (count == kTrip) {
            ra.load(a + o);
            rb.load(b + o);
        } else {                                   // the frame's last trip: samples past its end count as equal
            ra.load_bytes(a + o, count);
            rb.load_bytes(b + o, count);
        }
        rd.clear();
        unsigned tabs = 0, tsq = 0;                // of one trip: at most 16 * 255 and 16 * 255^2
#pragma unroll
        for (int j = 0; j < kTrip; j++) {
            const int d = (int)ra.get(j) - (int)rb.get(j);
            tabs += (unsigned)(d < 0 ? -d : d);
            tsq += (unsigned)(d * d);
            rd.put(j, (uint32_t)(128 + d) & 0xffu);
        }
        sabs += tabs;
        ssq += tsq;
        if (diff) {
            if (count == kTrip) rd.store(diff + o);
            else rd.store_bytes(diff + o, count);
        }
    }
    sabs = wave_sum(sabs);
    ssq = wave_sum(ssq);
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *o = partial + (((int64_t)f * gridDim.x + blockIdx.x) * kWaves + threadIdx.x / 64) * 2;
        o[0] = sabs;
        o[1] = ssq;
    }
}

// one wave per frame over its `n` partial pairs
__global__ __launch_bounds__(64) void rgb8_final(const unsigned long long *__restrict__ partial, int n,
                                                 unsigned long long *__restrict__ sums)
{
    add_partials(partial, n, sums);
}

// ---- host side -------------------------------------------------------------------------------------------------------

static bool dims_ok(int h, int w) { return h > 0 && w > 0 && h <= kMaxDim && w <= kMaxDim; }

static bool dtype_ok(int dtype) { return dtype == kFloat32 || dtype == kFloat16 || dtype == kBFloat16; }

static int score_blocks(int h, int w)
{
    const int64_t trips = ((int64_t)h * w * 3 + kTrip - 1) / kTrip;
    const int64_t blocks = (trips + kThreads - 1) / kThreads;
    return (int)(blocks < kMaxScoreBlocks ? blocks : kMaxScoreBlocks);
}

template <typename T>
static int launch_decode(hipStream_t stream, unsigned grid, const uint8_t *rgb, int frames, int h, int w, void *planes,
                         int64_t sf, int64_t sc, int64_t sr, int pl, int pt, int hp, int wp)
{
    hipLaunchKernelGGL(rgb8_decode<T>, dim3(grid), dim3(kThreads), 0, stream, rgb, frames, h, w,
                       static_cast<typename T::elem *>(planes), sf, sc, sr, pl, pt, hp, wp);
    return launched();
}

template <typename T>
static int launch_quantise(hipStream_t stream, unsigned grid, const void *planes, int64_t sf, int64_t sc, int64_t sr,
                           int frames, int h, int w, uint8_t *rgb)
{
    hipLaunchKernelGGL(rgb8_quantise<T>, dim3(grid), dim3(kThreads), 0, stream,
                       static_cast<const typename T::elem *>(planes), sf, sc, sr, frames, h, w, rgb);
    return launched();
}

}  // namespace memc

using namespace memc;

extern "C" {

const char *memc_still_version(void) { return "memc_hip_still 0.1 gfx950"; }

int memc_rgb8_decode(memc_still_stream_t stream, const uint8_t *rgb_u8, int frames, int h, int w, void *planes, int dtype,
                     int64_t stride_frame, int64_t stride_c, int64_t stride_row, int pad_left, int pad_right, int pad_top,
                     int pad_bottom)
{
    if (frames < 0) return -1;
    if (!dims_ok(h, w)) return -1;
    if (!dtype_ok(dtype)) return -1;
    int hp, wp;
    if (!padded_extent_ok(h, w, pad_left, pad_right, pad_top, pad_bottom, true, stride_frame, stride_c, stride_row, hp, wp))
        return -1;
    if (frames == 0) return 0;
    if (!rgb_u8 || !planes) return -1;
    const unsigned grid = quad_grid(frames, hp, wp);
    if (!grid) return -1;
    const hipStream_t s = (hipStream_t)stream;
    if (dtype == kFloat32)
        return launch_decode<F32>(s, grid, rgb_u8, frames, h, w, planes, stride_frame, stride_c, stride_row, pad_left, pad_top, hp, wp);
    if (dtype == kFloat16)
        return launch_decode<F16>(s, grid, rgb_u8, frames, h, w, planes, stride_frame, stride_c, stride_row, pad_left, pad_top, hp, wp);
    return launch_decode<BF16>(s, grid, rgb_u8, frames, h, w, planes, stride_frame, stride_c, stride_row, pad_left, pad_top, hp, wp);
}

int memc_rgb8_quantise(memc_still_stream_t stream, const void *planes, int dtype, int64_t stride_frame, int64_t stride_c,
                       int64_t stride_row, int frames, int h, int w, uint8_t *rgb_u8)
{
    if (frames < 0) return -1;
    if (!dims_ok(h, w)) return -1;
    if (!dtype_ok(dtype)) return -1;
    if (!strides_ok(stride_frame, stride_c, stride_row, w)) return -1;
    if (frames == 0) return 0;
    if (!planes || !rgb_u8) return -1;
    const unsigned grid = quad_grid(frames, h, w);
    if (!grid) return -1;
    const hipStream_t s = (hipStream_t)stream;
    if (dtype == kFloat32) return launch_quantise<F32>(s, grid, planes, stride_frame, stride_c, stride_row, frames, h, w, rgb_u8);
    if (dtype == kFloat16) return launch_quantise<F16>(s, grid, planes, stride_frame, stride_c, stride_row, frames, h, w, rgb_u8);
    return launch_quantise<BF16>(s, grid, planes, stride_frame, stride_c, stride_row, frames, h, w, rgb_u8);
}

size_t memc_rgb8_score_workspace_bytes(int frames, int h, int w)
{
    if (frames < 0 || !dims_ok(h, w) || frames > kMaxScoreFrames) return 0;
    return (size_t)(frames > 0 ? frames : 1) * score_blocks(h, w) * kWaves * 2 * sizeof(unsigned long long);
}

int memc_rgb8_score(memc_still_stream_t stream, const uint8_t *rgb_a, const uint8_t *rgb_b, int frames, int h, int w,
                    uint64_t *sums, uint8_t *diff_u8, void *workspace, size_t workspace_bytes)
{
    if (frames < 0) return -1;
    if (!dims_ok(h, w)) return -1;
    if (frames > kMaxScoreFrames) return -1;
    if (workspace_bytes < memc_rgb8_score_workspace_bytes(frames, h, w)) return -1;
    if (frames == 0) return 0;
    if (!rgb_a || !rgb_b || !sums || !workspace) return -1;
    if (((uintptr_t)sums | (uintptr_t)workspace) & 7u) return -1;
    const int blocks = score_blocks(h, w);
    unsigned long long *partial = static_cast<unsigned long long *>(workspace);
    hipLaunchKernelGGL(rgb8_partial, dim3(blocks, frames), dim3(kThreads), 0, (hipStream_t)stream, rgb_a, rgb_b,
                       (int64_t)h * w * 3, diff_u8, partial);
    if (launched() != 0) return -1;
    hipLaunchKernelGGL(rgb8_final, dim3(frames), dim3(64), 0, (hipStream_t)stream, partial, blocks * kWaves,
                       reinterpret_cast<unsigned long long *>(sums));
    return launched();
}

}  // extern "C"
