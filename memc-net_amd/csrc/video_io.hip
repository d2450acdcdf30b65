// video_io.hip -- the frame I/O of the HD demo loop (networks/yuv_io.py) for gfx950: the kernels and the C ABI of
// libmemc_hip_video.so (include/memc_video.h).  One translation unit; no object and no symbol shared with the other
// libraries.  The lane scheme, the wave sum and the host checks are memc_frame_io.hpp's, shared as text with lp_video_io.hip
// and still_io.hip; the quad's bytes and the bodies of the first two kernels are memc_frame_io_i420.hpp's, with lp_video_io.hip.
//
// Four streaming byte kernels and a final pass; a lane takes four horizontally adjacent pixels of one row:
//   i420_decode     i420_decode_body.inc on float32 planes: a gather over the PADDED extent that stores float32(byte) / 255
//                   into the three planes and, for the pixels inside the frame, the RGB bytes.
//   rgb_quantise    rgb_quantise_body.inc on float32 planes: three float quads in, twelve bytes out.
//   i420_encode     twelve bytes in, four Y bytes out and, on even rows, two U and two V bytes (even columns).
//   luma_partial    a workgroup strides over its frame's quads; per lane uint64 sums of |dY| and dY^2, reduced over the wave
//                   by shuffles; one partial per WAVE goes to the workspace.  luma_final: one wave per frame adds them.
//                   Integer sums: no atomics, no order dependence.  No LDS anywhere in this file.
// The arithmetic is memc_video_math.hpp's (float64, explicit fma chain, contraction off).
// Memory: plane offsets inside an I420 buffer and RGB rows have any alignment, so bytes move through vector types of
// alignment 1 (the queues run in unaligned-access mode, as for memc_tile.hpp's f32x4u) and floats through f32x4u.
#include "memc_frame_io_i420.hpp"
#include "memc_video.h"

#pragma clang fp contract(off)

namespace memc {

constexpr int kMaxScoreBlocks = 1024;      // workgroups per frame of luma_partial

__global__ __launch_bounds__(kThreads) void i420_decode(const uint8_t *__restrict__ i420, int frames, int h, int w,
                                                        uint8_t *__restrict__ rgb, float *__restrict__ planes, int64_t sf,
                                                        int64_t sc, int64_t sr, int pl, int pt, int hp, int wp)
{
    using T = F32;
#include "i420_decode_body.inc"
}

__global__ __launch_bounds__(kThreads) void rgb_quantise(const float *__restrict__ planes, int64_t sf, int64_t sc, int64_t sr,
                                                         int frames, int h, int w, uint8_t *__restrict__ rgb)
{
    using T = F32;
#include "rgb_quantise_body.inc"
}

__global__ __launch_bounds__(kThreads) void i420_encode(const uint8_t *__restrict__ rgb, int frames, int h, int w,
                                                        uint8_t *__restrict__ i420)
{
    int f, y, x0;
    if (!quad_of_lane(frames, h, (w + 3) / 4, f, y, x0)) return;
    const int count = min(4, w - x0);              // 4 or 2: w is even
    Rgb4Bytes q;
    load_rgb4(rgb + (((int64_t)f * h + y) * w + x0) * 3, count, q);
    const int64_t ny = (int64_t)h * w, nc = (int64_t)(h / 2) * (w / 2);
    uint8_t *Y = i420 + (int64_t)f * (ny + 2 * nc), *U = Y + ny, *V = U + nc;
    u8x4 y4;
    for (int j = 0; j < 4; j++) y4[j] = mv::luma_of(q.b[3 * j], q.b[3 * j + 1], q.b[3 * j + 2]);
    uint8_t *yo = Y + (int64_t)y * w + x0;
    if (count == 4) *reinterpret_cast<u8x4u *>(yo) = y4;
    else *reinterpret_cast<u8x2u *>(yo) = u8x2{y4[0], y4[1]};
    if (y & 1) return;
    u8x2 u2, v2;
    for (int j = 0; j < 2; j++) {
        uint8_t u, v;
        mv::chroma_of(q.b[6 * j], q.b[6 * j + 1], q.b[6 * j + 2], u, v);
        u2[j] = u;
        v2[j] = v;
    }
    const int64_t co = (int64_t)(y / 2) * (w / 2) + x0 / 2;
    if (count == 4) {
        *reinterpret_cast<u8x2u *>(U + co) = u2;
        *reinterpret_cast<u8x2u *>(V + co) = v2;
    } else {
        U[co] = u2[0];
        V[co] = v2[0];
    }
}

// grid (blocks per frame, frames); partial[(f * gridDim.x * kWaves + wave of the frame) * 2 + {0, 1}]
__global__ __launch_bounds__(kThreads) void luma_partial(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int h,
                                                         int w, unsigned long long *__restrict__ partial)
{
    const int f = blockIdx.y, qpr = (w + 3) / 4;
    const int64_t quads = (int64_t)h * qpr, base = (int64_t)f * h * w * 3;
    unsigned long long sabs = 0, ssq = 0;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < quads; i += (int64_t)gridDim.x * kThreads) {
        const int64_t y = i / qpr;
        const int x0 = 4 * (int)(i - y * qpr), count = min(4, w - x0);
        const int64_t o = base + (y * w + x0) * 3;
        Rgb4Bytes qa, qb;
        load_rgb4(a + o, count, qa);
        load_rgb4(b + o, count, qb);
        for (int j = 0; j < count; j++) {
            const int d = (int)mv::luma_of(qa.b[3 * j], qa.b[3 * j + 1], qa.b[3 * j + 2]) -
                          (int)mv::luma_of(qb.b[3 * j], qb.b[3 * j + 1], qb.b[3 * j + 2]);
            sabs += (unsigned)(d < 0 ? -d : d);
            ssq += (unsigned)(d * d);
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

// one wave per frame over its `n` partials
__global__ __launch_bounds__(64) void luma_final(const unsigned long long *__restrict__ partial, int n,
                                                 unsigned long long *__restrict__ sums)
{
    add_partials(partial, n, sums);
}

// ---- host side -------------------------------------------------------------------------------------------------------

static int score_blocks(int h, int w)
{
    const int64_t quads = (int64_t)h * ((w + 3) / 4);
    const int64_t blocks = (quads + kThreads - 1) / kThreads;
    return (int)(blocks < kMaxScoreBlocks ? blocks : kMaxScoreBlocks);
}

}  // namespace memc

using namespace memc;

extern "C" {

const char *memc_video_version(void) { return "memc_hip_video 0.1 gfx950"; }

int memc_i420_decode(memc_video_stream_t stream, const uint8_t *i420, int frames, int h, int w, uint8_t *rgb_u8,
                     float *planes, int64_t stride_frame, int64_t stride_c, int64_t stride_row, int pad_left, int pad_right,
                     int pad_top, int pad_bottom)
{
    if (!dims_ok(frames, h, w)) return -1;
    if (!planes) pad_left = pad_right = pad_top = pad_bottom = 0;
    int hp, wp;
    if (!padded_extent_ok(h, w, pad_left, pad_right, pad_top, pad_bottom, planes != nullptr, stride_frame, stride_c, stride_row,
                          hp, wp))
        return -1;
    if (frames == 0) return 0;
    if (!i420 || (!rgb_u8 && !planes)) return -1;
    const unsigned grid = quad_grid(frames, hp, wp);
    if (!grid) return -1;
    hipLaunchKernelGGL(i420_decode, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, i420, frames, h, w, rgb_u8, planes,
                       stride_frame, stride_c, stride_row, pad_left, pad_top, hp, wp);
    return launched();
}

int memc_rgb_quantise(memc_video_stream_t stream, const float *planes, int64_t stride_frame, int64_t stride_c,
                      int64_t stride_row, int frames, int h, int w, uint8_t *rgb_u8)
{
    if (!dims_ok(frames, h, w)) return -1;
    if (!strides_ok(stride_frame, stride_c, stride_row, w)) return -1;
    if (frames == 0) return 0;
    if (!planes || !rgb_u8) return -1;
    const unsigned grid = quad_grid(frames, h, w);
    if (!grid) return -1;
    hipLaunchKernelGGL(rgb_quantise, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, planes, stride_frame, stride_c,
                       stride_row, frames, h, w, rgb_u8);
    return launched();
}

int memc_i420_encode(memc_video_stream_t stream, const uint8_t *rgb_u8, int frames, int h, int w, uint8_t *i420)
{
    if (!dims_ok(frames, h, w)) return -1;
    if (frames == 0) return 0;
    if (!rgb_u8 || !i420) return -1;
    const unsigned grid = quad_grid(frames, h, w);
    if (!grid) return -1;
    hipLaunchKernelGGL(i420_encode, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, rgb_u8, frames, h, w, i420);
    return launched();
}

size_t memc_luma_score_workspace_bytes(int frames, int h, int w)
{
    if (!dims_ok(frames, h, w)) return 0;
    return (size_t)(frames > 0 ? frames : 1) * score_blocks(h, w) * kWaves * 2 * sizeof(unsigned long long);
}

int memc_luma_score(memc_video_stream_t stream, const uint8_t *rgb_a, const uint8_t *rgb_b, int frames, int h, int w,
                    uint64_t *sums, void *workspace, size_t workspace_bytes)
{
    if (!dims_ok(frames, h, w)) return -1;
    if (frames > 65535) return -1;                 // the frame is the grid's y
    if (workspace_bytes < memc_luma_score_workspace_bytes(frames, h, w)) return -1;
    if (frames == 0) return 0;
    if (!rgb_a || !rgb_b || !sums || !workspace) return -1;
    if (((uintptr_t)sums | (uintptr_t)workspace) & 7u) return -1;
    const int blocks = score_blocks(h, w);
    unsigned long long *partial = static_cast<unsigned long long *>(workspace);
    hipLaunchKernelGGL(luma_partial, dim3(blocks, frames), dim3(kThreads), 0, (hipStream_t)stream, rgb_a, rgb_b, h, w,
                       partial);
    if (launched() != 0) return -1;
    hipLaunchKernelGGL(luma_final, dim3(frames), dim3(64), 0, (hipStream_t)stream, partial, blocks * kWaves,
                       reinterpret_cast<unsigned long long *>(sums));
    return launched();
}

}  // extern "C"
