// lp_filter_interpolation.hip -- the adaptive warp (FilterInterpolation) forward and the fused dual warp + occlusion blend
// on fp16 / bf16 storage, for gfx950: the kernels and the C ABI of libmemc_hip_lp.so (include/memc_warp_lp.h).
//
// The fp32 kernels (filter_interpolation.hip) are HBM-bound gather stencils; half-width storage is what removes bytes.
// RGB forward per site: image 6 + flow 8 (fp32) or 4 (T) + taps 32 + output 6 = 52 / 48 B instead of 96; blend 102 / 94 B
// instead of 188; the 64-channel context warp 296 B instead of 584.  The kernels are the fp32 kernels' structure on
// narrower global accesses (memc_lp.hpp):
//   fi_fwd_lp_tiled<T, FT, true>    RGB: fi_fwd_tiled_fs4<16, 3, ...>'s band loop, results kept until every band has run;
//   fi_fwd_lp_tiled<T, FT, false>   any other channel count: fi_fwd_tiled_c4n's chunk pipeline (the next chunk's rows in
//                                   flight while this one is gathered), a ragged last chunk re-reads the last plane;
//   fi_blend_lp_tiled<T, FT>        fi_fwd_blend_c3: both directions' streams up front, one box -> stage -> gather round each;
//   fi_fwd_lp_direct / fi_blend_lp_direct   one lane per site, any filter size, any width, any alignment.
// The LDS holds fp32 pixel quads (staging widens), so the gather and its arithmetic are the fp32 kernels' own: the site
// geometry, the gather and the one-site paths from global memory are memc_fi.hpp's, the descriptor checks memc_desc.hpp's.
#include "memc_common.hpp"
#include "memc_tile.hpp"
#include "memc_fi.hpp"
#include "memc_lp.hpp"
#include "memc_desc.hpp"
#include "memc_launch.hpp"
#include "memc_warp_lp.h"

#include <math.h>

namespace memc {

thread_local const char *t_lp_path = "";

// MEMC_FI_SITES and MEMC_FI_LAUNDER (memc_fi.hpp) as functions, for fi_blend_lp_tiled alone: expanded in place, as in
// every other kernel, its fp16 instantiation is 2 % slower (profiles/r08_refactor_lowp_ab.txt).
__device__ __forceinline__ FiSite4 fi_sites_fn(int x, int y, int W, int H, bool inb, const f32x4 &fx4, const f32x4 &fy4,
                                               int &cmin_, int &cmax_, int &rmin_, int &rmax_)
{
    MEMC_FI_SITES(g, x, y, W, H, inb, fx4, fy4);
    cmin_ = cmin; cmax_ = cmax; rmin_ = rmin; rmax_ = rmax;
    return g;
}
__device__ __forceinline__ void fi_launder_fn(f32x4 (&tp)[16], FiSite4 &g) { MEMC_FI_LAUNDER(tp, g); }

// --------------------------------------------------------------------------------------------------
// Forward, fs == 4, LDS-tiled: 64 x 16 tiles of 256 lanes, one lane = four consecutive sites of a row, strip walk.
// RGB: one chunk of three channels, bands outside (fi_fwd_tiled_fs4<16, 3, 2, 0>).  Otherwise: bands outside, chunks of
// four channels inside, the next chunk's staging loads issued before this chunk's gathers (fi_fwd_tiled_c4n<0, 256,
// RAGGED>).  RAGGED (a channel count that is not a multiple of four, a separate instantiation): the last chunk re-reads the
// last plane and stores only the channels it has; one workgroup per CU (at two, the bf16 instantiation spills).
// --------------------------------------------------------------------------------------------------
template <class T, class FT, bool RGB, bool RAGGED = false>
__global__ __launch_bounds__(256, RAGGED ? 1 : 2) void fi_fwd_lp_tiled(
    int W, int H, int C, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    const st_t<T> *__restrict__ in1, const st_t<FT> *__restrict__ flow, const st_t<T> *__restrict__ filt,
    st_t<T> *__restrict__ out)
{
    constexpr int LX = 16;
    using G = TileGeom<LX>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem);
    int *bb = reinterpret_cast<int *>(smem + G::kCapPx * 16);

    const TileCoord tc = strip_walk(blockIdx.x, gridDim.x, tiles_x, tiles_y, gridDim.x / (tiles_x * tiles_y));
    const int b = tc.b, tile_x0 = tc.tx * G::kTW, tile_y0 = tc.ty * G::kTH;
    const int x = tile_x0 + 4 * (threadIdx.x % LX), y = tile_y0 + threadIdx.x / LX;
    const bool inb = x < W && y < H;                       // W % 4 == 0: a lane's four sites are in or out together
    // streams first, unconditional (a clamped in-range address for lanes past the edge; see fi_fwd_tiled_fs4)
    const int xs = min(x, W - 4), ys = min(y, H - 1);
    const st_t<FT> *flow_p = flow + b * s2b + (int64_t)ys * s2h + xs;
    const st_t<T> *tap_p = filt + b * s3b + (int64_t)ys * s3h + xs;
    const f32x4 fx4 = ld4_stream<FT>(flow_p), fy4 = ld4_stream<FT>(flow_p + s2c);
    f32x4 tp[16];
#pragma unroll
    for (int k = 0; k < 16; k++) tp[k] = ld4_stream<T>(tap_p + k * s3c);

    MEMC_FI_SITES(g, x, y, W, H, inb, fx4, fy4);
    const BBox box = tile_bbox<LX>(cmin, cmax, rmin, rmax, bb);
    const Bands bands = make_bands<LX>(box);
    const st_t<T> *in_b = in1 + b * s1b;
    st_t<T> *out_p = out + b * s1b + (int64_t)y * s1h + x;
    unsigned done = 0;

    if (RGB) {
        f32x4 res[4];
#pragma unroll
        for (int j = 0; j < 4; j++) res[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int bi = 0; bi < bands.n; bi++) {
            const Region rb = band_region(box, bands, bi);
            const unsigned sel = inb ? fi_covered(rb, g, W, H) & ~done : 0u;
            if (bi > 0 && !__syncthreads_or(sel != 0)) continue;
            done |= sel;
            const StageSlot sl = stage_slots(rb);
            const unsigned short *plane[3] = {in_b, in_b + s1c, in_b + 2 * s1c};
            LpStageRegs<3> sr;
            lp_stage_load<3>(rb, sl, plane, s1h, sr);
            lp_stage_store<T, 3>(rb, sl, sr, tile);
            __syncthreads();
            MEMC_FI_LAUNDER(tp, g);
            fi_gather<LX, 3>(rb, g, tp, sel, W, H, tile, res);
        }
        if (inb) {
            if (g.valid != 0xFu) {                         // out-of-range sites copy the input pixel
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const f32x4 own = ld4_cached<T>(in_b + c * s1c + (int64_t)y * s1h + x);
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (!((g.valid >> j) & 1)) res[j][c] = own[j];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) st4_stream<T>(out_p + c * s1c, f32x4{res[0][c], res[1][c], res[2][c], res[3][c]});
        }
    } else {
#pragma unroll 1
        for (int bi = 0; bi < bands.n; bi++) {
            const Region r = band_region(box, bands, bi);
            const unsigned sel = inb ? fi_covered(r, g, W, H) & ~done : 0u;
            // later bands only run when somebody still needs them; the vote is also the barrier that frees the LDS
            if (bi > 0 && !__syncthreads_or(sel != 0)) continue;
            done |= sel;
            // band 0 also writes the out-of-range sites (they copy the input pixel)
            const unsigned wr = sel | (bi == 0 && inb ? ~g.valid & 0xFu : 0u);
            const StageSlot sl = stage_slots(r);
            LpStageRegs<4> sr;
            auto stage_load = [&](int cb) {                // planes past the last one: the last one again
                const unsigned short *plane[4];
#pragma unroll
                for (int c = 0; c < 4; c++) plane[c] = in_b + (RAGGED ? min(cb + c, C - 1) : cb + c) * s1c;
                lp_stage_load<4>(r, sl, plane, s1h, sr);
            };
            stage_load(0);
#pragma unroll 1
            for (int c0 = 0; c0 < C; c0 += 4) {
                lp_stage_store<T, 4>(r, sl, sr, tile);
                __syncthreads();
                // next chunk's rows: in flight while this chunk is gathered (the last iteration re-reads its own chunk)
                stage_load(c0 + 4 < C ? c0 + 4 : c0);
                MEMC_FI_LAUNDER(tp, g);
                f32x4 res[4];
#pragma unroll
                for (int j = 0; j < 4; j++) res[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                fi_gather<LX, 4>(r, g, tp, sel, W, H, tile, res);
                const st_t<T> *plane0 = in_b + c0 * s1c;
                st_t<T> *o = out_p + c0 * s1c;
                if (wr & ~g.valid) {                       // out-of-range sites copy the input pixel
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        if (RAGGED && c0 + c >= C) continue;
                        const f32x4 own = ld4_cached<T>(plane0 + c * s1c + (int64_t)y * s1h + x);
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            if (!((g.valid >> j) & 1)) res[j][c] = own[j];
                    }
                }
                if (wr == 0xFu) {
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        if (!RAGGED || c0 + c < C) st4_stream<T>(o + c * s1c, f32x4{res[0][c], res[1][c], res[2][c], res[3][c]});
                } else if (wr) {                           // a lane whose sites are split over bands
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if ((wr >> j) & 1) {
#pragma unroll
                            for (int c = 0; c < 4; c++)
                                if (!RAGGED || c0 + c < C) o[c * s1c + j] = narrow<T>(res[j][c]);
                        }
                }
                __syncthreads();
            }
        }
    }
    unsigned slow = inb ? g.valid & ~done : 0u;            // rare: not coverable within kMaxBands bands
    while (slow) {
        const int j = __ffs(slow) - 1;
        slow &= slow - 1;
        fi_site_scalar_lp<T, FT>(x + j, y, W, H, C, 4, in_b, s1c, s1h, flow_p + j, s2c, tap_p + j, s3c, out_p + j);
    }
}

// --------------------------------------------------------------------------------------------------
// Fused dual warp + occlusion blend, RGB, fs == 4 (fi_fwd_blend_c3):
//     out = occ0 * FI(in0, flow0, filt0) + occ1 * FI(in2, flow1, filt1)       (two products, one sum, rounded once)
// Both directions' streams are requested up front -- direction 1's taps stay packed (two registers per quad) until
// direction 0 is done -- then each direction runs its own box -> (bands of) stage -> gather round on the same LDS bytes.
// --------------------------------------------------------------------------------------------------
template <class T, class FT>
__global__ __launch_bounds__(256, 2) void fi_blend_lp_tiled(
    int W, int H, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    int64_t sob, int soh,
    const st_t<T> *__restrict__ in0, const st_t<T> *__restrict__ in2, const st_t<FT> *__restrict__ flow0,
    const st_t<FT> *__restrict__ flow1, const st_t<T> *__restrict__ filt0, const st_t<T> *__restrict__ filt1,
    const st_t<T> *__restrict__ occ0, const st_t<T> *__restrict__ occ1, st_t<T> *__restrict__ out)
{
    constexpr int LX = 16;
    using G = TileGeom<LX>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem);
    int *bb = reinterpret_cast<int *>(smem + G::kCapPx * 16);

    const TileCoord tc = strip_walk(blockIdx.x, gridDim.x, tiles_x, tiles_y, gridDim.x / (tiles_x * tiles_y));
    const int b = tc.b;
    const int x = tc.tx * G::kTW + 4 * (int)(threadIdx.x % LX), y = tc.ty * G::kTH + (int)(threadIdx.x / LX);
    const bool inb = x < W && y < H;
    const int xs = min(x, W - 4), ys = min(y, H - 1);
    const int64_t o2 = (int64_t)ys * s2h + xs, o3 = (int64_t)ys * s3h + xs, oo = (int64_t)ys * soh + xs;
    // all streams of both directions first
    f32x4 fx[2], fy[2], oc[2], tp[16];
    u16x4 tq1[16];
    fx[0] = ld4_stream<FT>(flow0 + b * s2b + o2);  fy[0] = ld4_stream<FT>(flow0 + b * s2b + s2c + o2);
    fx[1] = ld4_stream<FT>(flow1 + b * s2b + o2);  fy[1] = ld4_stream<FT>(flow1 + b * s2b + s2c + o2);
#pragma unroll
    for (int k = 0; k < 16; k++) tp[k] = ld4_stream<T>(filt0 + b * s3b + k * s3c + o3);
#pragma unroll
    for (int k = 0; k < 16; k++) tq1[k] = __builtin_nontemporal_load(reinterpret_cast<const u16x4a *>(filt1 + b * s3b + k * s3c + o3));
    oc[0] = ld4_stream<T>(occ0 + b * sob + oo);
    oc[1] = ld4_stream<T>(occ1 + b * sob + oo);

    // one direction: box -> (bands of) stage -> gather; returns the warped RGB of the lane's four sites
    auto warp = [&](const st_t<T> *in_b, const st_t<FT> *flow_b, const st_t<T> *filt_b, const f32x4 &fx4, const f32x4 &fy4,
                    f32x4 (&res)[4]) {
        int cmin, cmax, rmin, rmax;
        FiSite4 g = fi_sites_fn(x, y, W, H, inb, fx4, fy4, cmin, cmax, rmin, rmax);
        const BBox box = tile_bbox<LX>(cmin, cmax, rmin, rmax, bb);
        const Bands bands = make_bands<LX>(box);
#pragma unroll
        for (int j = 0; j < 4; j++) res[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        unsigned done = 0;
#pragma unroll 1
        for (int bi = 0; bi < bands.n; bi++) {
            const Region rb = band_region(box, bands, bi);
            const unsigned sel = inb ? fi_covered(rb, g, W, H) & ~done : 0u;
            if (bi > 0 && !__syncthreads_or(sel != 0)) continue;
            done |= sel;
            const StageSlot sl = stage_slots(rb);
            const unsigned short *plane[3] = {in_b, in_b + s1c, in_b + 2 * s1c};
            LpStageRegs<3> sr;
            lp_stage_load<3>(rb, sl, plane, s1h, sr);
            lp_stage_store<T, 3>(rb, sl, sr, tile);
            __syncthreads();
            fi_launder_fn(tp, g);
            fi_gather<LX, 3>(rb, g, tp, sel, W, H, tile, res);
        }
        if (!inb) return;
        unsigned slow = g.valid & ~done;                   // rare: not coverable within kMaxBands bands
        while (slow) {
            const int j = __ffs(slow) - 1;
            slow &= slow - 1;
            const st_t<FT> *fp = flow_b + (int64_t)y * s2h + x + j;
            const FiSite s = fi_locate(x + j, y, W, H, widen<FT>(fp[0]), widen<FT>(fp[s2c]));
            const int L = s.ix - 1, Tp = s.iy - 1;               // the site's 4 x 4 window
            f32x4 v;
#pragma unroll 1
            for (int c = 0; c < 3; c++)
                v[c] = fi_site_chan<T, int64_t>(s, 4, L, Tp, L + 4, Tp + 4, W, H, in_b + c * s1c, s1h, filt_b + (int64_t)y * s3h + x + j, s3c);
            v[3] = 0.f;
#pragma unroll
            for (int jj = 0; jj < 4; jj++) res[jj] = jj == j ? v : res[jj];
        }
        if (g.valid != 0xFu) {                             // out-of-range sites copy the input pixel
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const f32x4 own = ld4_cached<T>(in_b + c * s1c + (int64_t)y * s1h + x);
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (!((g.valid >> j) & 1)) res[j][c] = own[j];
            }
        }
    };

    f32x4 w0[4], w2[4];
    warp(in0 + b * s1b, flow0 + b * s2b, filt0 + b * s3b, fx[0], fy[0], w0);
    __syncthreads();                                       // direction 0's gathers are done: the LDS is free again
#pragma unroll
    for (int k = 0; k < 16; k++) tp[k] = widen4<T>(tq1[k]);
    warp(in2 + b * s1b, flow1 + b * s2b, filt1 + b * s3b, fx[1], fy[1], w2);
    if (!inb) return;
    st_t<T> *o = out + b * s1b + (int64_t)y * s1h + x;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float p0 = oc[0][j] * w0[j][c], p2 = oc[1][j] * w2[j][c];     // two products, one sum (fi_fwd_blend_c3)
            v[j] = p0 + p2;
        }
        st4_stream<T>(o + c * s1c, v);
    }
}

// --------------------------------------------------------------------------------------------------
// One lane per site, any filter size, any width / strides / alignment: what the tiled kernels do not take.
// 64 x 4 sites per workgroup.  BLEND: the dual warp + blend of any channel count and filter size.
// --------------------------------------------------------------------------------------------------
template <class T, class FT>
__global__ __launch_bounds__(256) void fi_fwd_lp_direct(
    int W, int H, int C, int fs, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    const st_t<T> *__restrict__ in1, const st_t<FT> *__restrict__ flow, const st_t<T> *__restrict__ filt,
    st_t<T> *__restrict__ out)
{
    const unsigned t = xcd_chunked_id(blockIdx.x, gridDim.x);
    const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y, b = t / (tiles_x * tiles_y);
    const int x = tx * kWave + (threadIdx.x & (kWave - 1)), y = ty * 4 + (threadIdx.x / kWave);
    if (x >= W || y >= H) return;
    fi_site_scalar_lp<T, FT>(x, y, W, H, C, fs, in1 + b * s1b, s1c, s1h, flow + b * s2b + (int64_t)y * s2h + x, s2c,
                          filt + b * s3b + (int64_t)y * s3h + x, s3c, out + b * s1b + (int64_t)y * s1h + x);
}

template <class T, class FT>
__global__ __launch_bounds__(256) void fi_blend_lp_direct(
    int W, int H, int C, int fs, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    int64_t sob, int soh,
    const st_t<T> *__restrict__ in0, const st_t<T> *__restrict__ in2, const st_t<FT> *__restrict__ flow0,
    const st_t<FT> *__restrict__ flow1, const st_t<T> *__restrict__ filt0, const st_t<T> *__restrict__ filt1,
    const st_t<T> *__restrict__ occ0, const st_t<T> *__restrict__ occ1, st_t<T> *__restrict__ out)
{
    const unsigned t = xcd_chunked_id(blockIdx.x, gridDim.x);
    const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y, b = t / (tiles_x * tiles_y);
    const int x = tx * kWave + (threadIdx.x & (kWave - 1)), y = ty * 4 + (threadIdx.x / kWave);
    if (x >= W || y >= H) return;
    const int64_t o1 = b * s1b + (int64_t)y * s1h + x, o2 = b * s2b + (int64_t)y * s2h + x,
                  o3 = b * s3b + (int64_t)y * s3h + x, oo = b * sob + (int64_t)y * soh + x;
    const FiSite s0 = fi_locate(x, y, W, H, widen<FT>(flow0[o2]), widen<FT>(flow0[o2 + s2c]));
    const FiSite s1 = fi_locate(x, y, W, H, widen<FT>(flow1[o2]), widen<FT>(flow1[o2 + s2c]));
    const float oc0 = widen<T>(occ0[oo]), oc1 = widen<T>(occ1[oo]);
    const st_t<T> *i0 = in0 + b * s1b, *i2 = in2 + b * s1b;
    const int L0 = s0.ix + 1 - fs / 2, T0 = s0.iy + 1 - fs / 2, L1 = s1.ix + 1 - fs / 2, T1 = s1.iy + 1 - fs / 2;   // windows
    for (int c = 0; c < C; c++) {
        const float w0 = s0.valid ? fi_site_chan<T, int64_t>(s0, fs, L0, T0, L0 + fs, T0 + fs, W, H, i0 + c * s1c, s1h, filt0 + o3, s3c) : widen<T>(in0[o1 + c * s1c]);
        const float w2 = s1.valid ? fi_site_chan<T, int64_t>(s1, fs, L1, T1, L1 + fs, T1 + fs, W, H, i2 + c * s1c, s1h, filt1 + o3, s3c) : widen<T>(in2[o1 + c * s1c]);
        const float p0 = oc0 * w0, p2 = oc1 * w2;
        out[o1 + c * s1c] = narrow<T>(p0 + p2);
    }
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_lp.h)
// ==================================================================================================
namespace {

using namespace memc;
constexpr int kErr = -1;

template <class T, class FT, bool RGB, bool RAGGED = false>
void launch_fi_fwd_lp_tiled(const FiFwdCall<st_t<T>, st_t<FT>> &k)
{
    using G = TileGeom<16>;
    const int ntx = (k.w + G::kTW - 1) / G::kTW, nty = (k.h + G::kTH - 1) / G::kTH;
    hipLaunchKernelGGL((fi_fwd_lp_tiled<T, FT, RGB, RAGGED>), dim3((unsigned)ntx * nty * k.batch), dim3(256),
                       tile_lds_bytes<16>(), k.stream, k.w, k.h, k.channel, ntx, nty, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c,
                       k.s2.h, k.s3.b, k.s3.c, k.s3.h, k.in1, k.flow, k.filt, k.out);
}

template <class T, class FT>
int fi_fwd_lp_launch(hipStream_t stream, int w, int h, int c, int n, int fs, bool tiled, const memc_tensor4 *in1,
                     const memc_tensor4 *flow, const memc_tensor4 *filt, const memc_tensor4 *out)
{
    const FiFwdCall<st_t<T>, st_t<FT>> k = {
        stream, w, h, c, n, fs, plane(in1), plane(flow), plane(filt),
        reinterpret_cast<const st_t<T> *>(in1->data), reinterpret_cast<const st_t<FT> *>(flow->data),
        reinterpret_cast<const st_t<T> *>(filt->data), reinterpret_cast<st_t<T> *>(out->data)};
    if (tiled) {
        if (c == 3) {
            t_lp_path = "fi_fwd_lp:tiled_c3";
            launch_fi_fwd_lp_tiled<T, FT, true, false>(k);
        } else {
            t_lp_path = "fi_fwd_lp:tiled_c4n";
            if (c % 4 == 0) launch_fi_fwd_lp_tiled<T, FT, false, false>(k);
            else launch_fi_fwd_lp_tiled<T, FT, false, true>(k);
        }
    } else {
        const int tiles_x = (w + kWave - 1) / kWave, tiles_y = (h + 3) / 4;
        t_lp_path = "fi_fwd_lp:direct";
        hipLaunchKernelGGL((fi_fwd_lp_direct<T, FT>), dim3((unsigned)tiles_x * tiles_y * n), dim3(256), 0, stream, w, h, c, fs,
                           tiles_x, tiles_y, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c, k.s2.h, k.s3.b, k.s3.c, k.s3.h, k.in1,
                           k.flow, k.filt, k.out);
    }
    return launch_status();
}

template <class T, class FT>
int fi_blend_lp_launch(hipStream_t stream, int w, int h, int c, int n, int fs, bool tiled, const memc_tensor4 *const (&t)[9])
{
    const auto *i0 = reinterpret_cast<const st_t<T> *>(t[0]->data), *i2 = reinterpret_cast<const st_t<T> *>(t[1]->data);
    const auto *f0 = reinterpret_cast<const st_t<FT> *>(t[2]->data), *f1 = reinterpret_cast<const st_t<FT> *>(t[3]->data);
    const auto *k0 = reinterpret_cast<const st_t<T> *>(t[4]->data), *k1 = reinterpret_cast<const st_t<T> *>(t[5]->data);
    const auto *q0 = reinterpret_cast<const st_t<T> *>(t[6]->data), *q1 = reinterpret_cast<const st_t<T> *>(t[7]->data);
    auto *o = reinterpret_cast<st_t<T> *>(t[8]->data);
    const Plane s1 = plane(t[0]), s2 = plane(t[2]), s3 = plane(t[4]), so = plane(t[6]);      // (so.c is not used)
    if (tiled) {
        using G = TileGeom<16>;
        const int ntx = (w + G::kTW - 1) / G::kTW, nty = (h + G::kTH - 1) / G::kTH;
        t_lp_path = "fi_blend_lp:tiled_c3";
        hipLaunchKernelGGL((fi_blend_lp_tiled<T, FT>), dim3((unsigned)ntx * nty * n), dim3(256), tile_lds_bytes<16>(), stream,
                           w, h, ntx, nty, s1.b, s1.c, s1.h, s2.b, s2.c, s2.h, s3.b, s3.c, s3.h, so.b, so.h, i0, i2, f0, f1, k0,
                           k1, q0, q1, o);
    } else {
        const int tiles_x = (w + kWave - 1) / kWave, tiles_y = (h + 3) / 4;
        t_lp_path = "fi_blend_lp:direct";
        hipLaunchKernelGGL((fi_blend_lp_direct<T, FT>), dim3((unsigned)tiles_x * tiles_y * n), dim3(256), 0, stream, w, h, c,
                           fs, tiles_x, tiles_y, s1.b, s1.c, s1.h, s2.b, s2.c, s2.h, s3.b, s3.c, s3.h, so.b, so.h, i0, i2, f0,
                           f1, k0, k1, q0, q1, o);
    }
    return launch_status();
}

// the four (payload, flow) instantiations of a launcher
#define MEMC_LP_DISPATCH(LAUNCH, ...)                                                                                   \
    (payload == MEMC_F16 ? (flowt == MEMC_F32 ? LAUNCH<F16, F32>(__VA_ARGS__) : LAUNCH<F16, F16>(__VA_ARGS__))         \
                         : (flowt == MEMC_F32 ? LAUNCH<BF16, F32>(__VA_ARGS__) : LAUNCH<BF16, BF16>(__VA_ARGS__)))

}  // namespace

extern "C" {

const char *memc_lp_version(void) { return "memc_hip_lp 0.1 gfx950"; }

const char *memc_lp_last_kernel_path(void) { return memc::t_lp_path; }

int FilterInterpolationLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype payload, memc_dtype flowt,
                                            const memc_tensor4 *input1, const memc_tensor4 *input2,
                                            const memc_tensor4 *input3, const memc_tensor4 *output)
{
    if (!dtypes_ok(payload, flowt)) return kErr;
    if (!ok(input1) || !ok(input2) || !ok(input3) || !ok(output)) return kErr;        // my_lib_cuda.c:641-643
    if (!flow_matches(input1, input2) || !taps_match(input1, input3)) return kErr;    // :611-617
    const int fs = (int)sqrt((float)input3->size[1]);                                 // :619-620
    if (fs < 1) return kErr;
    if (!same_layout(input1, output)) return kErr;                                    // :644-645 (+h)
    const int n = (int)input1->size[0], c = (int)input1->size[1], h = (int)input1->size[2], w = (int)input1->size[3];
    if (n == 0 || c == 0 || h == 0 || w == 0) return 0;
    const bool tiled = fs == 4 && w % 4 == 0 && w >= 8 && quad_ok(input1) && quad_ok(input2) && quad_ok(input3) &&
                       quad_ok(output);
    return MEMC_LP_DISPATCH(fi_fwd_lp_launch, (hipStream_t)stream, w, h, c, n, fs, tiled, input1, input2, input3, output);
}

int FilterInterpolationBlendLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype payload, memc_dtype flowt,
                                                 const memc_tensor4 *input0, const memc_tensor4 *input2,
                                                 const memc_tensor4 *flow0, const memc_tensor4 *flow1,
                                                 const memc_tensor4 *filter0, const memc_tensor4 *filter1,
                                                 const memc_tensor4 *occlusion0, const memc_tensor4 *occlusion1,
                                                 const memc_tensor4 *output)
{
    if (!dtypes_ok(payload, flowt)) return kErr;
    const memc_tensor4 *const all[9] = {input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1, output};
    for (const memc_tensor4 *t : all)
        if (!ok(t)) return kErr;
    if (!flow_matches(input0, flow0) || !taps_match(input0, filter0)) return kErr;
    if (!same_layout(input0, input2) || !same_layout(input0, output) || !same_layout(flow0, flow1) ||
        !same_layout(filter0, filter1) || !same_layout(occlusion0, occlusion1))
        return kErr;
    if (occlusion0->size[0] != input0->size[0] || occlusion0->size[1] != 1 || occlusion0->size[2] != input0->size[2] ||
        occlusion0->size[3] != input0->size[3])
        return kErr;
    const int fs = (int)sqrt((float)filter0->size[1]);
    if (fs < 1) return kErr;
    const int n = (int)input0->size[0], c = (int)input0->size[1], h = (int)input0->size[2], w = (int)input0->size[3];
    if (n == 0 || c == 0 || h == 0 || w == 0) return 0;
    bool tiled = fs == 4 && c == 3 && w % 4 == 0 && w >= 8;
    for (const memc_tensor4 *t : all) tiled = tiled && quad_ok(t);
    return MEMC_LP_DISPATCH(fi_blend_lp_launch, (hipStream_t)stream, w, h, c, n, fs, tiled, all);
}

}  // extern "C"
