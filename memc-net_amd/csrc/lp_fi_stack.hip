// lp_fi_stack.hip -- the STACKED adaptive warp (FilterInterpolation) forward on fp16 / bf16 storage, for gfx950: the kernels
// and the C ABI of libmemc_hip_lp_stack.so (include/memc_warp_lp_stack.h).
//
// A MEMC_Net_VE cast to fp16 / bf16 assembles its rectifier input from twelve libmemc_hip_lp.so launches and a torch.cat.
// Per site and neighbour, from the tensor shapes: 48 B for the RGB warp, 292 B for the 64-channel context warp and 340 B
// again for torch.cat (read and write 6 + 128 + 36 B): about 680 B.  Here the warps write their slices of the rectifier
// input themselves and store the flow and the taps they hold in registers anyway to theirs: about 376 B.
//
// The kernel is fi_fwd_stack_tiled<RGB> (fi_stack.hip) on half storage, exactly as fi_fwd_lp_tiled<T, FT, RGB>
// (lp_fi_fwd_body.inc) is the fp32 tiled forward on half storage: 64 x 16 tiles of 256 lanes, four sites per lane, strip
// walk, band loop, the in-kernel one-site path; the image staged from 8-byte quads of T into the fp32 LDS tile; fp32
// arithmetic on exactly widened inputs in memc_fi.hpp's order; every stored element rounded once.  What differs from
// lp_fi_fwd_body.inc is fi_stack.hip's three things, all in how the output is addressed: the batch index splits into
// (neighbour, batch element), the output has its own three strides and a channel offset, and the flow and tap quads are
// stored to their slices once every band has run.  Restated here rather than shared as text with fi_stack.hip: that unit
// keeps its machine code (tools/isa_diff.py), and a lane addresses `out` differently here (a wave-uniform base and a 32-bit
// in-plane offset: below).
//
// The tile grid is the HALF library's for the same call -- fi_tile_grid<TileGeom<16>>(w, h), unshifted; the 32-site shift
// belongs to the fp32 RGB kernels only -- because the grid decides which sites of a tile that no six bands cover go to the
// one-site path, and that path's last bit can differ from the gather's (fi_stack.hip's header).  So every warped element
// is libmemc_hip_lp.so's bit for bit (tests/test_gpu_lp_stack.py).
#include "memc_common.hpp"
#include "memc_tile.hpp"
#include "memc_fi.hpp"
#include "memc_lp.hpp"
#include "memc_fi_abi.hpp"
#include "memc_warp_lp_stack.h"

namespace memc {

thread_local const char *t_lp_stack_path = "";

// ONE site from global memory, all channels: fi_site_scalar_lp (memc_fi.hpp) with the output's own channel stride.
template <class P, class FT>
__device__ __noinline__ void fi_site_scalar_stack_lp(int x, int y, int W, int H, int nch, int fs, const st_t<P> *plane0,
                                                     int64_t s1c, int s1h, const st_t<FT> *flow_p, int64_t s2c,
                                                     const st_t<P> *tap_p, int64_t s3c, st_t<P> *out_p, int64_t soc)
{
    const float fx = widen<FT>(flow_p[0]), fy = widen<FT>(flow_p[s2c]);
    const FiSite s = fi_locate(x, y, W, H, fx, fy);
    if (s.valid) {
        const int L = s.ix + 1 - fs / 2, T = s.iy + 1 - fs / 2, R = L + fs, Bm = T + fs;
        for (int c = 0; c < nch; c++)
            out_p[c * soc] = narrow<P>(fi_site_chan<P, int64_t, P>(s, fs, L, T, R, Bm, W, H, plane0 + c * s1c, s1h, tap_p, s3c));
    } else {
        const st_t<P> *p = plane0 + (int64_t)y * s1h + x;
        for (int c = 0; c < nch; c++) out_p[c * soc] = p[c * s1c];
    }
}

// input1 / flow / taps row `r` = n * nb + b: neighbour n of batch element b.  sob / soc / soh: the output's strides.
// T: the image, the taps and the output; FT: the flow (T or F32).
template <class T, class FT, bool RGB>
__global__ __launch_bounds__(256, 2) void fi_fwd_stack_lp_tiled(
    int W, int H, int C, int tiles_x, int tiles_y, int nb,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    int64_t sob, int64_t soc, int soh, int c_base, int skip, int flow_base, int tap_base,
    const st_t<T> *__restrict__ in1, const st_t<FT> *__restrict__ flow, const st_t<T> *__restrict__ filt,
    st_t<T> *__restrict__ out)
{
    using I = T;                               // the image and the output in the taps' storage
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
    const st_t<I> *in_b = in1 + b * s1b;
    // the output: batch element b % nb, the neighbour's slot of C channels behind c_base (one slot left for the centre)
    const int nbr = b / nb, slot = nbr + (skip >= 0 && nbr >= skip ? 1 : 0);
    const int64_t c_warp = c_base + (int64_t)slot * C;     // wave-uniform: the warp's first channel of `out`
    // wave-uniform base + the lane's in-plane offset (within int: the host checks), so that no lane carries a second 64-bit
    // site offset beside the image's (with one, the many-channel bf16 instantiations spill)
    st_t<I> *out_b = out + (b - nbr * nb) * sob, *out_u = out_b + c_warp * soc;
    const int osite = ys * soh + xs, isite = ys * s1h + xs;    // used by lanes inside the image only: xs == x, ys == y
    unsigned done = 0;
    if constexpr (RGB) {
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
            const st_t<I> *plane[3] = {in_b, in_b + s1c, in_b + 2 * s1c};
            ImgStageRegs<I, 3> sr;
            img_stage_load<I, 3>(rb, sl, plane, s1h, sr);
            img_stage_store<I, 3>(rb, sl, sr, tile);
            __syncthreads();
            MEMC_FI_LAUNDER(tp, g);
            fi_gather<LX, 3>(rb, g, tp, sel, W, H, tile, res);
        }
        if (inb) {
            if (g.valid != 0xFu) {                         // out-of-range sites copy the input pixel
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const f32x4 own = ld4_cached<I>(in_b + c * s1c + isite);
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (!((g.valid >> j) & 1)) res[j][c] = own[j];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) st4_stream<I>(out_u + c * soc + osite, f32x4{res[0][c], res[1][c], res[2][c], res[3][c]});
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
            ImgStageRegs<I, 4> sr;
            auto stage_load = [&](int cb) {
                const st_t<I> *plane[4];
#pragma unroll
                for (int c = 0; c < 4; c++) plane[c] = in_b + (cb + c) * s1c;
                img_stage_load<I, 4>(r, sl, plane, s1h, sr);
            };
            stage_load(0);
#pragma unroll 1
            for (int c0 = 0; c0 < C; c0 += 4) {
                img_stage_store<I, 4>(r, sl, sr, tile);
                __syncthreads();
                // next chunk's rows: in flight while this chunk is gathered (the last iteration re-reads its own chunk)
                stage_load(c0 + 4 < C ? c0 + 4 : c0);
                MEMC_FI_LAUNDER(tp, g);
                f32x4 res[4];
#pragma unroll
                for (int j = 0; j < 4; j++) res[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                fi_gather<LX, 4>(r, g, tp, sel, W, H, tile, res);
                const st_t<I> *plane0 = in_b + c0 * s1c;
                st_t<I> *o = out_u + c0 * soc + osite;
                if (wr & ~g.valid) {                       // out-of-range sites copy the input pixel
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const f32x4 own = ld4_cached<I>(plane0 + c * s1c + isite);
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            if (!((g.valid >> j) & 1)) res[j][c] = own[j];
                    }
                }
                if (wr == 0xFu) {
#pragma unroll
                    for (int c = 0; c < 4; c++) st4_stream<I>(o + c * soc, f32x4{res[0][c], res[1][c], res[2][c], res[3][c]});
                } else if (wr) {                           // a lane whose sites are split over bands
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if ((wr >> j) & 1) {
#pragma unroll
                            for (int c = 0; c < 4; c++) o[c * soc + j] = narrow<I>(res[j][c]);
                        }
                }
                __syncthreads();
            }
        }
    }
    // pass-through: the flow and tap quads to their slices (every band has run: nothing waits for these loads now).  A T
    // value widened and narrowed again is the value as read; an fp32 flow is rounded to T once, as `.to(T)` rounds it.
    if (inb) {
        if (flow_base >= 0) {
            st_t<T> *o = out_b + (flow_base + 2 * (int64_t)nbr) * soc + osite;
            st4_stream<T>(o, fx4);
            st4_stream<T>(o + soc, fy4);
        }
        if (tap_base >= 0) {
            st_t<T> *o = out_b + (tap_base + 16 * (int64_t)nbr) * soc + osite;
#pragma unroll
            for (int k = 0; k < 16; k++) st4_stream<T>(o + k * soc, tp[k]);
        }
    }
    unsigned slow = inb ? g.valid & ~done : 0u;            // rare: not coverable within kMaxBands bands
    while (slow) {
        const int j = __ffs(slow) - 1;
        slow &= slow - 1;
        fi_site_scalar_stack_lp<T, FT>(x + j, y, W, H, C, 4, in_b, s1c, s1h, flow_p + j, s2c, tap_p + j, s3c, out_u + osite + j, soc);
    }
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_lp_stack.h)
// ==================================================================================================
namespace {

using namespace memc;

// every in-plane element offset (h - 1) * row_stride + w within int (the one-site path's row offsets are int)
inline bool plane_fits_int(int w, int h, std::initializer_list<int64_t> row_strides)
{
    for (int64_t s : row_strides)
        if ((int64_t)(h > 0 ? h - 1 : 0) * s + w > INT32_MAX) return false;
    return true;
}

struct ChanRange {
    int64_t lo, hi;                            // [lo, hi)
};

}  // namespace

extern "C" {

const char *memc_lp_stack_version(void) { return "memc_hip_lp_stack 0.1 gfx950"; }

const char *memc_lp_stack_last_kernel_path(void) { return memc::t_lp_stack_path; }

int FilterInterpolationStackLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype payload, memc_dtype flowt,
                                                 const memc_tensor4 *input1, const memc_tensor4 *flow,
                                                 const memc_tensor4 *taps, const memc_tensor4 *out, int n_neighbours,
                                                 int c_base, int skip, int flow_base, int tap_base)
{
    // malformed
    if (!dtypes_ok(payload, flowt)) return kErr;
    if (!ok(input1) || !ok(flow) || !ok(taps) || !ok(out)) return kErr;
    if (!flow_matches(input1, flow) || !taps_match(input1, taps)) return kErr;
    const int fs = fi_filter_side_exact(taps->size[1]);
    if (fs < 1) return kErr;
    if (n_neighbours < 1 || input1->size[0] % n_neighbours != 0) return kErr;
    if (out->size[0] != input1->size[0] / n_neighbours || out->size[2] != input1->size[2] || out->size[3] != input1->size[3])
        return kErr;
    if (skip < -1 || skip > n_neighbours || flow_base < -1 || tap_base < -1) return kErr;
    // empty
    const FiChecked q = fi_sizes(fs, input1);
    if (q.done) return q.code;
    // not covered
    const int nb = q.n / n_neighbours;
    if (!((q.c == 3 || q.c % 4 == 0) && fs == 4 && q.w % 4 == 0 && q.w >= 8)) return kNotCovered;
    // 8-byte quads of four T; an fp32 flow on the same test, as libmemc_hip_lp.so takes it (its loads need dwords only)
    for (const memc_tensor4 *t : {input1, flow, taps, out})
        if (!quad_ok(t)) return kNotCovered;
    if (!plane_fits_int(q.w, q.h, {input1->stride[2], flow->stride[2], taps->stride[2], out->stride[2]})) return kNotCovered;
    // the written channel ranges of `out`: the warps before and behind the centre's slot, the flows, the taps
    ChanRange wr[4];
    int nwr = 0;
    const int64_t c = q.c, n = n_neighbours;
    if (skip > 0 || skip < 0) wr[nwr++] = {c_base, c_base + (skip < 0 ? n : (int64_t)skip) * c};
    if (skip >= 0 && skip < n) wr[nwr++] = {c_base + (skip + 1) * c, c_base + (n + 1) * c};
    if (flow_base >= 0) wr[nwr++] = {flow_base, flow_base + 2 * n};
    if (tap_base >= 0) wr[nwr++] = {tap_base, tap_base + 16 * n};
    for (int i = 0; i < nwr; i++) {
        if (wr[i].lo < 0 || wr[i].hi > out->size[1]) return kNotCovered;
        for (int j = 0; j < i; j++)
            if (wr[i].lo < wr[j].hi && wr[j].lo < wr[i].hi) return kNotCovered;
    }
    // the half library's grid for the same call: unshifted
    const TileGrid g = fi_tile_grid<TileGeom<16>>(q.w, q.h);
    const Plane s1 = plane(input1), s2 = plane(flow), s3 = plane(taps), so = plane(out);
    return fi_dispatch(payload, flowt, [&](auto t, auto ft) {
        using T = decltype(t);
        using FT = decltype(ft);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)g.ntx * g.nty * q.n), dim3(256), tile_lds_bytes<16>(),
                               (hipStream_t)stream, q.w, q.h, q.c, g.ntx, g.nty, nb, s1.b, s1.c, s1.h, s2.b, s2.c, s2.h,
                               s3.b, s3.c, s3.h, so.b, so.c, so.h, c_base, skip, flow_base, tap_base, data_of<T>(input1),
                               data_of<FT>(flow), data_of<T>(taps), data_of<T>(out));
        };
        if (q.c == 3) {
            t_lp_stack_path = "fi_fwd_stack_lp:tiled_c3";
            launch(fi_fwd_stack_lp_tiled<T, FT, true>);
        } else {
            t_lp_stack_path = "fi_fwd_stack_lp:tiled_c4n";
            launch(fi_fwd_stack_lp_tiled<T, FT, false>);
        }
        return launch_status();
    });
}

}  // extern "C"
