// ssim.hip -- the structural similarity of two 8-bit planes for gfx950: the kernels and the C ABI of libmemc_hip_ssim.so
// (include/memc_ssim.h), the third score of the HD demo loop (networks/yuv_io.py).  One translation unit, nothing shared
// with the other libraries but memc_video_math.hpp's luma_of (a header: no object, no symbol).
//
// Three kernels, wave64:
//   ssim_luma_planes  uint8 RGB [frames, h, w, 3] of both inputs -> one uint8 luma plane per frame in the workspace (the
//                     encode's truncated Y, memc_video::luma_of).  A lane takes four adjacent pixels of a row.  Once per
//                     input pixel: the tiles below overlap by 6 rows and columns and would recompute the float64 luma 1.5 x.
//   ssim_tiles        one workgroup (256 lanes, four waves) per tile of 64 x 16 window CENTRES of one frame:
//                       1. the 70 x 22 byte box of each plane goes to LDS (rows of 72 bytes; bytes beyond the plane are 0);
//                       2. each of the 22 rows is reduced to the horizontal 7-sums of x, y, x^2, y^2, xy at its 64 centres
//                          (int32, LDS): a lane takes one (row, centre), three dwords of each plane;
//                       3. wave k takes centre rows 4k .. 4k + 3, a lane one column of them: the vertical 7-sum of the first,
//                          then one row in and one row out per further centre; S per centre (memc_ssim_math.hpp), the lane's
//                          four S added in row order, centres outside the interior as +0.0;
//                       4. a shuffle tree in a fixed pattern; lane 0 stores the wave's partial to the workspace.
//   ssim_final        one wave per frame: lane l adds partials l, l + 64, ... in index order, the same tree, over N.
// Float64 sums in a fixed order, no atomics: the same bits from run to run.  LDS per workgroup: 2 x 22 x 72 bytes of box
// and 5 x 22 x 64 int32 of row sums, 31 328 bytes (five workgroups per CU).  No private scratch.
// Memory: rows and frames of a plane start at any byte, so global bytes move through vector types of alignment 1 (the
// queues run in unaligned-access mode), as in video_io.hip; a quad that crosses the plane's right edge goes byte by byte.
#include <hip/hip_runtime.h>

#include "memc_ssim_math.hpp"
#include "memc_video_math.hpp"
#include "memc_ssim.h"

#pragma clang fp contract(off)

namespace memc {

namespace mv = memc_video;
namespace ms = memc_ssim;

typedef uint8_t u8x4 __attribute__((ext_vector_type(4)));
typedef u8x4 u8x4u __attribute__((aligned(1)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef u32x3 u32x3u __attribute__((aligned(1)));
typedef uint32_t u32u __attribute__((aligned(1)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMinDim = ms::kWindow;
constexpr int kMaxDim = 32768;
constexpr int64_t kMaxStride = (int64_t)1 << 46;        // frames * stride and h * stride stay inside int64
constexpr int kHalo = ms::kWindow - 1;                 // 6: a tile's box exceeds its centres by this much
constexpr int kTileX = 64, kTileY = 16;                // window centres per workgroup
constexpr int kRowsPerWave = kTileY / kWaves;          // 4
constexpr int kBoxRows = kTileY + kHalo;               // 22
constexpr int kBoxDwords = (kTileX + kHalo + 3) / 4;   // 18 dwords: 72 bytes per staged row, 70 of them used
constexpr int kSums = 5;                               // x, y, x^2, y^2, xy

// ---- the luma planes -------------------------------------------------------------------------------------------------

// grid (blocks over frames * h * quads per row, 2): y = 0 takes rgb_a, y = 1 rgb_b; planes[(y * frames + f) * h * w ...]
__global__ __launch_bounds__(kThreads) void ssim_luma_planes(const uint8_t *__restrict__ rgb_a,
                                                             const uint8_t *__restrict__ rgb_b, int frames, int h, int w,
                                                             uint8_t *__restrict__ planes)
{
    const int qpr = (w + 3) / 4;
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (int64_t)frames * h * qpr) return;
    const int64_t row = idx / qpr;                     // frame * h + y
    const int x0 = 4 * (int)(idx - row * qpr), count = min(4, w - x0);
    const uint8_t *src = (blockIdx.y ? rgb_b : rgb_a) + (row * w + x0) * 3;
    uint8_t *dst = planes + ((int64_t)blockIdx.y * frames * h + row) * w + x0;
    u32x3 q = u32x3{0u, 0u, 0u};                       // twelve RGB bytes of four pixels, kept in registers
    if (count == 4) {
        q = *reinterpret_cast<const u32x3u *>(src);
    } else {
#pragma unroll
        for (int i = 0; i < 9; i++)
            if (i < 3 * count) q[i >> 2] |= (uint32_t)src[i] << (8 * (i & 3));
    }
    u8x4 y4;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int k = 3 * j;
        y4[j] = mv::luma_of((uint8_t)(q[k >> 2] >> (8 * (k & 3))), (uint8_t)(q[(k + 1) >> 2] >> (8 * ((k + 1) & 3))),
                            (uint8_t)(q[(k + 2) >> 2] >> (8 * ((k + 2) & 3))));
    }
    if (count == 4) {
        *reinterpret_cast<u8x4u *>(dst) = y4;
    } else {
        for (int j = 0; j < count; j++) dst[j] = y4[j];
    }
}

// ---- the tiles -------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double wave_sum(double v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;                                          // lane 0 holds the wave's sum
}

// seven consecutive bytes starting at byte `c` of a staged row of dwords
__device__ __forceinline__ void seven_bytes(const uint32_t *row, int c, int (&v)[7])
{
    const int d = c >> 2, sh = 8 * (c & 3);
    const uint32_t d0 = row[d], d1 = row[d + 1], d2 = row[d + 2];
    const uint32_t lo = (uint32_t)((((uint64_t)d1 << 32) | d0) >> sh), hi = (uint32_t)((((uint64_t)d2 << 32) | d1) >> sh);
    for (int j = 0; j < 4; j++) v[j] = (int)((lo >> (8 * j)) & 0xffu);
    for (int j = 0; j < 3; j++) v[4 + j] = (int)((hi >> (8 * j)) & 0xffu);
}

// grid (tiles across, tiles down, frames); partial[((f * gridDim.y + tile row) * gridDim.x + tile column) * kWaves + wave]
__global__ __launch_bounds__(kThreads) void ssim_tiles(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
                                                       int64_t sf, int64_t sr, int h, int w, double *__restrict__ partial)
{
    __shared__ uint32_t box[2][kBoxRows][kBoxDwords];
    __shared__ int hsum[kSums][kBoxRows][kTileX];
    const int tid = threadIdx.x, f = blockIdx.z;
    const int x0 = blockIdx.x * kTileX, y0 = blockIdx.y * kTileY;      // the box's first pixel = the tile's first centre

    // 1. stage both boxes: a lane per dword; nothing is read beyond row h - 1 or column w - 1
    for (int q = tid; q < 2 * kBoxRows * kBoxDwords; q += kThreads) {
        const int plane = q / (kBoxRows * kBoxDwords), rem = q - plane * (kBoxRows * kBoxDwords);
        const int r = rem / kBoxDwords, dw = rem - r * kBoxDwords;
        const int y = y0 + r, x = x0 + 4 * dw;
        uint32_t v = 0u;
        if (y < h && x < w) {
            const uint8_t *p = (plane ? b : a) + f * sf + y * sr + x;
            if (x + 4 <= w) {
                v = *reinterpret_cast<const u32u *>(p);
            } else {
                for (int j = 0; j < w - x; j++) v |= (uint32_t)p[j] << (8 * j);
            }
        }
        box[plane][r][dw] = v;
    }
    __syncthreads();

    // 2. horizontal 7-sums of every staged row at the tile's 64 centres
    for (int i = tid; i < kBoxRows * kTileX; i += kThreads) {
        const int r = i / kTileX, c = i - r * kTileX;
        int xs[7], ys[7];
        seven_bytes(box[0][r], c, xs);
        seven_bytes(box[1][r], c, ys);
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
        for (int j = 0; j < 7; j++) {
            sx += xs[j];
            sy += ys[j];
            sxx += xs[j] * xs[j];
            syy += ys[j] * ys[j];
            sxy += xs[j] * ys[j];
        }
        hsum[0][r][c] = sx;
        hsum[1][r][c] = sy;
        hsum[2][r][c] = sxx;
        hsum[3][r][c] = syy;
        hsum[4][r][c] = sxy;
    }
    __syncthreads();

    // 3. vertical 7-sums and S for the lane's four centres (rows r0 .. r0 + 3 of column c), top to bottom
    const int c = tid & 63, wave = tid >> 6, r0 = wave * kRowsPerWave;
    const bool col_in = x0 + c < w - kHalo;
    int v[kSums];
    for (int k = 0; k < kSums; k++) {
        v[k] = 0;
        for (int r = 0; r < ms::kWindow; r++) v[k] += hsum[k][r0 + r][c];
    }
    double acc = 0.0;
    for (int j = 0; j < kRowsPerWave; j++) {
        if (j > 0)
            for (int k = 0; k < kSums; k++) v[k] += hsum[k][r0 + j + kHalo][c] - hsum[k][r0 + j - 1][c];
        const double s = ms::window_ssim(v[0], v[1], v[2], v[3], v[4]);
        acc += (col_in && y0 + r0 + j < h - kHalo) ? s : 0.0;
    }

    // 4. one partial per wave
    acc = wave_sum(acc);
    if (c == 0)
        partial[(((int64_t)f * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kWaves + wave] = acc;
}

// one wave per frame over its `n` partials; `count` = (h - 6)(w - 6)
__global__ __launch_bounds__(64) void ssim_final(const double *__restrict__ partial, int n, double count,
                                                 double *__restrict__ ssim)
{
    const double *p = partial + (int64_t)blockIdx.x * n;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) acc += p[i];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) ssim[blockIdx.x] = acc / count;
}

// ---- host side -------------------------------------------------------------------------------------------------------

static bool dims_ok(int frames, int h, int w)
{
    return frames >= 0 && frames <= 65535 && h >= kMinDim && w >= kMinDim && h <= kMaxDim && w <= kMaxDim;
}

static int tiles_x(int w) { return (w - kHalo + kTileX - 1) / kTileX; }
static int tiles_y(int h) { return (h - kHalo + kTileY - 1) / kTileY; }

static size_t partial_bytes(int frames, int h, int w)
{
    return (size_t)frames * tiles_x(w) * tiles_y(h) * kWaves * sizeof(double);
}

// no launch may exceed 2^31 lanes (the frame is the tiles' grid z, the luma planes' lanes are one grid x)
static bool grids_ok(int frames, int h, int w)
{
    const int64_t limit = 0x7fffffffLL;
    return (int64_t)frames * tiles_x(w) * tiles_y(h) * kThreads <= limit &&
           (int64_t)frames * h * ((w + 3) / 4) + kThreads <= limit;
}

static int launched() { return hipGetLastError() == hipSuccess ? 0 : -1; }

// the tiles and the final pass; every check has passed
static int enqueue(hipStream_t stream, const uint8_t *a, const uint8_t *b, int64_t sf, int64_t sr, int frames, int h, int w,
                   double *ssim, double *partial)
{
    const int tx = tiles_x(w), ty = tiles_y(h);
    hipLaunchKernelGGL(ssim_tiles, dim3(tx, ty, frames), dim3(kThreads), 0, stream, a, b, sf, sr, h, w, partial);
    if (launched() != 0) return -1;
    hipLaunchKernelGGL(ssim_final, dim3(frames), dim3(64), 0, stream, partial, tx * ty * kWaves,
                       (double)((int64_t)(h - kHalo) * (w - kHalo)), ssim);
    return launched();
}

}  // namespace memc

using namespace memc;

extern "C" {

const char *memc_ssim_version(void) { return "memc_hip_ssim 0.1 gfx950"; }

// [partials: frames * tiles * 4 doubles][luma planes: 2 * frames * h * w bytes, rounded up to 8]
size_t memc_ssim_workspace_bytes(int frames, int h, int w)
{
    if (!dims_ok(frames, h, w)) return 0;
    const int n = frames > 0 ? frames : 1;
    return partial_bytes(n, h, w) + (((size_t)2 * n * h * w + 7) & ~(size_t)7);
}

int memc_ssim_u8(memc_ssim_stream_t stream, const uint8_t *a, const uint8_t *b, int64_t stride_frame, int64_t stride_row,
                 int frames, int h, int w, double *ssim, void *workspace, size_t workspace_bytes)
{
    if (!dims_ok(frames, h, w) || !grids_ok(frames, h, w)) return -1;
    if (stride_row < w || stride_row > kMaxStride) return -1;
    if (frames > 1 && (stride_frame < (int64_t)(h - 1) * stride_row + w || stride_frame > kMaxStride)) return -1;
    if (workspace_bytes < memc_ssim_workspace_bytes(frames, h, w)) return -1;
    if (frames == 0) return 0;
    if (!a || !b || !ssim || !workspace) return -1;
    if (((uintptr_t)ssim | (uintptr_t)workspace) & 7u) return -1;
    return enqueue((hipStream_t)stream, a, b, frames > 1 ? stride_frame : 0, stride_row, frames, h, w, ssim,
                   static_cast<double *>(workspace));
}

int memc_ssim_luma_rgb(memc_ssim_stream_t stream, const uint8_t *rgb_a, const uint8_t *rgb_b, int frames, int h, int w,
                       double *ssim, void *workspace, size_t workspace_bytes)
{
    if (!dims_ok(frames, h, w) || !grids_ok(frames, h, w)) return -1;
    if (workspace_bytes < memc_ssim_workspace_bytes(frames, h, w)) return -1;
    if (frames == 0) return 0;
    if (!rgb_a || !rgb_b || !ssim || !workspace) return -1;
    if (((uintptr_t)ssim | (uintptr_t)workspace) & 7u) return -1;
    uint8_t *planes = static_cast<uint8_t *>(workspace) + partial_bytes(frames, h, w);
    const int64_t lanes = (int64_t)frames * h * ((w + 3) / 4), plane = (int64_t)h * w;
    hipLaunchKernelGGL(ssim_luma_planes, dim3((unsigned)((lanes + kThreads - 1) / kThreads), 2), dim3(kThreads), 0,
                       (hipStream_t)stream, rgb_a, rgb_b, frames, h, w, planes);
    if (launched() != 0) return -1;
    return enqueue((hipStream_t)stream, planes, planes + frames * plane, plane, w, frames, h, w, ssim,
                   static_cast<double *>(workspace));
}

}  // extern "C"
