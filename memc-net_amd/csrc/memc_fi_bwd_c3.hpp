// memc_fi_bwd_c3.hpp -- the FilterInterpolation backward, RGB (C == 3), fs == 4, LDS-tiled: the pieces of its kernel body
// (fi_bwd_c3_body.inc), written once over the storage of the tensors (memc_lp.hpp: F32, F16, BF16).
//   fi_bwd_c3.hip       fi_bwd_c3_pk: fp32 (libmemc_hip.so), the description of the algorithm and its measurements;
//   lp_fi_bwd_c3.hip    fi_bwd_c3_lp: fp16 / bf16 image and taps, fp32 or half flow and gradoutput (libmemc_hip_lp_grad.so);
//   mx_fi_bwd_c3.hip    fi_bwd_c3_mx: fp32 image and gradoutput, fp16 / bf16 taps, fp32 or half flow (libmemc_hip_mx_grad.so).
// The LDS image, the packed planes of the image gradient and the arithmetic are the same for every storage: loads widen
// exactly, each stored gradient is rounded once.  The fp32 instantiations compile to the machine code they had before the
// storage was made a parameter (checked by disassembly: profiles/r07_lowp_backward.txt).
#pragma once

#include "memc_common.hpp"
#include "memc_tile.hpp"
#include "memc_fi.hpp"
#include "memc_pk.hpp"
#include "memc_lp.hpp"

#include <type_traits>

namespace memc {

// Per-workgroup phase timestamps (shader clock) for tools/trace_kernel.py: the TR = true instantiation exists in the
// measurement build only.
#ifdef MEMC_MEASURE
__device__ unsigned long long *g_trace_buf = nullptr;
#endif
template <bool ON>
__device__ __forceinline__ void trace_mark(int slot)
{
#ifdef MEMC_MEASURE
    if (ON && threadIdx.x == 0) g_trace_buf[(size_t)blockIdx.x * 16 + slot] = __builtin_readcyclecounter();
#else
    static_assert(!ON, "timestamps: measurement build only");
    (void)slot;
#endif
}

// Phase 1 of one band: tap and flow gradients of the sites in `fast` from the staged image.
// With s = sum_c g_c * in_c(tap cell) (3 FMAs per tap), and q the tap's quadrant:
//     gradinput3[tap] = wq * s,   gradinput2.x = sum_taps cx[q] * s * tap,   gradinput2.y likewise,
// where wq = {(1-a)(1-b), a(1-b), (1-a)b, ab}, cx = {-(1-b), (1-b), -b, b}, cy = {-(1-a), -a, (1-a), a}.
// (The reference sums per channel first -- same value up to fp32 re-association, ~1e-7 relative.)
// Tap rows are the outer loop so that only one row of tap gradients (4 float4) is live at a time.
template <class P, class FT>
__device__ __forceinline__ void fi_bwd_phase1(const Region &r, unsigned fast, FiSite4 &g, f32x4 (&tp)[16],
                                              const f32x4 (&go)[3], const f32x4 *tile, int W, int H,
                                              st_t<FT> *gin2_b, int64_t s2c, unsigned o2, st_t<P> *gin3_b, int64_t s3c,
                                              unsigned o3)
{
    MEMC_FI_LAUNDER(tp, g);                    // inside the caller's band loop
    // Only quads that this band owns completely (the common case) take this path -- ONE exec-masked region
    // without inner control flow, every store unconditional (the buffers are zero-filled by the caller:
    // 0 + g == g); mixed quads are redone per site by fi_bwd_site_taps.  Any load or data-dependent merge inside
    // the nest makes the compiler split it and spill the partial sums.
    if (fast != 0xFu) return;
    f32x4 gx4 = {0.f, 0.f, 0.f, 0.f}, gy4 = gx4;
    // Loop order (tap row, tap column, site): one float4 of tap gradients is live at a time and four image reads
    // are in flight; cell addresses are recomputed per use (the asm keeps them from being CSE'd into a table) --
    // the kernel lives or dies by staying clear of spills (252 of 256 registers with the staged rows parked beside it).
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int ro[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            asm volatile("" : "+v"(g.ix[j]));
            ro[j] = (clampi(g.iy[j] - 1 + k, H - 1) - r.y0) * r.pitch;
        }
#pragma unroll
        for (int m = 0; m < 4; m++) {
            f32x4 gt;                          // gt[j]: gradient of tap (k, m) of site j
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float a = g.a[j], bt = g.b[j];
                const int co = swz_col(clampi(g.ix[j] - 1 + m, W - 1) - r.x0);
                const f32x4 pix = tile[ro[j] + co];
                float sv = 0.0f;
                sv += go[0][j] * pix[0];  sv += go[1][j] * pix[1];  sv += go[2][j] * pix[2];
                const float wa = m < 2 ? (1 - a) : a, wb = k < 2 ? (1 - bt) : bt;
                gt[j] = (wa * wb) * sv;
                const float st = sv * tp[k * 4 + m][j];
                gx4[j] += (m < 2 ? -wb : wb) * st;
                gy4[j] += (k < 2 ? -wa : wa) * st;
            }
            st4_stream_u<P>(gin3_b + (k * 4 + m) * s3c, o3, gt);
        }
    }
    st4_stream_u<FT>(gin2_b, o2, gx4);         // gradinput2 is ASSIGNED
    st4_stream_u<FT>(gin2_b + s2c, o2, gy4);
}

// The 32 ds_add_u64 of the sites in `fast`.  sg = 2^(11 - e_g), st = 2^(11 - e_t): |g * sg| < 2^11, |w * st| <= 2^11.
__device__ __forceinline__ void fi_bwd_adds_pk(const Region &r, unsigned fast, FiSite4 &g, const f32x4 (&tp)[16],
                                               const f32x4 (&go)[3], float sg, float st,
                                               unsigned long long *accA, unsigned long long *accB, int W, int H)
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!((fast >> j) & 1)) continue;
        // keep the cell addresses and weights inside the caller's loops (hoisted, they spill)
        asm volatile("" : "+v"(g.ix[j]), "+v"(g.iy[j]), "+v"(g.a[j]), "+v"(g.b[j]));
        int ro[4], co[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            ro[k] = (clampi(g.iy[j] - 1 + k, H - 1) - r.y0) * r.pitch;
            co[k] = pk_col(clampi(g.ix[j] - 1 + k, W - 1) - r.x0, r.pitch >> 2);
        }
        const float a = g.a[j], bt = g.b[j];
        const float wq[4] = {st * ((1 - a) * (1 - bt)), st * (a * (1 - bt)), st * ((1 - a) * bt), st * (a * bt)};
        const float g0 = sg * go[0][j], g1 = sg * go[1][j], g2 = sg * go[2][j];
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const float w = wq[(k >> 1) * 2 + (m >> 1)] * tp[k * 4 + m][j];
                pk_add3(accA, accB, ro[k] + co[m], g0, g1, g2, w);
            }
    }
}

// the image gradient of ONE site with global atomics (tiles with a non-finite gradoutput or tap)
#define MEMC_FI_BWD_SITE_IMAGE_ATOMICS_BODY(P, FT, GT)                                                                \
    {                                                                                                                 \
        const FiSite s = fi_locate(x, y, W, H, widen_f32<FT>(flow_p[0]), widen_f32<FT>(flow_p[s2c]));                 \
        if (!s.valid) return;                                                                                         \
        for (int c = 0; c < 3; c++) {                                                                                 \
            const float gv = widen_f32<GT>(gout_p[c * s1c]);                                                          \
            float *q = gin1_b + c * s1c;                                                                              \
            for (int k = 0; k < 4; k++) {                                                                             \
                const int jj = clampi(s.iy - 1 + k, H - 1) * s1h;                                                     \
                for (int m = 0; m < 4; m++) {                                                                         \
                    const float wa = m < 2 ? (1 - s.a) : s.a, wb = k < 2 ? (1 - s.b) : s.b;                           \
                    atomic_add_f32(q + jj + clampi(s.ix - 1 + m, W - 1),                                              \
                                   gv * wa * wb * widen_f32<P>(tap_p[(k * 4 + m) * s3c]));                            \
                }                                                                                                     \
            }                                                                                                         \
        }                                                                                                             \
    }
__device__ __noinline__ void fi_bwd_site_image_atomics(int x, int y, int W, int H, float *gin1_b, int64_t s1c, int s1h,
                                                       const float *flow_p, int64_t s2c, const float *tap_p,
                                                       int64_t s3c, const float *gout_p)
MEMC_FI_BWD_SITE_IMAGE_ATOMICS_BODY(F32, F32, F32)
template <class P, class FT, class GT>
__device__ __noinline__ void fi_bwd_site_image_atomics_lp(int x, int y, int W, int H, float *gin1_b, int64_t s1c, int s1h,
                                                          const st_t<FT> *flow_p, int64_t s2c, const st_t<P> *tap_p,
                                                          int64_t s3c, const st_t<GT> *gout_p)
MEMC_FI_BWD_SITE_IMAGE_ATOMICS_BODY(P, FT, GT)
#undef MEMC_FI_BWD_SITE_IMAGE_ATOMICS_BODY

// One 64 x 16 tile of sites per workgroup; 48 KiB of LDS: the two packed planes, then -- the same bytes -- the staged
// image (3072 cells: 96 x 32, 80 x 38 or 64 x 48 by the band's width).  The image gradient comes FIRST: its adds need
// no image, so
//   * the planes are zeroed while the tile's 21 input float4 per lane are still in flight;
//   * the adds start as soon as the box is known; the image rows, requested just before, arrive in registers while
//     the LDS is busy with adds and flush (they are touched once before the flush: vmcnt is in order, and a wait
//     placed behind the flush's conditional atomics could only be vmcnt(0));
//   * the rows go to the LDS behind the flush, and phase 1 (tap and flow gradients from the staged image) ends the
//     tile with its stores.
// Serial chain of a tile: load -> box -> adds -> flush -> (image is already here) -> phase 1: four barriers.
// Measured, 720p batch 32, smooth / i.i.d. flow / 448 x 256 batch 8 (profiles/r03_fi_bwd_c3_arms.txt; one box, one process):
//   rounds 1-2: fp64 plane per colour, three rounds of adds / flush      1777 / 2977 /  98.1 us
//   packed planes, image first, fixed 96 x 32 geometry                   1545 / 2594 /  85.6
//   packed planes, image first, pitch by the band's width                1364 / 1985 /  71.5
//   packed planes, image gradient first (this kernel)                    1312 / 1929 /  71.4
//   planes beside the image (78 KiB; adds straight behind phase 1)       1743 / 3462 /  90.1   (two-band sweeps; no overlap won)
// NT lanes take a tile of 64 x NT / 16 sites.  256 (64 x 16, 48 KiB, two workgroups per CU) is the product.
// 128 (64 x 8, 24 KiB, four workgroups of two waves per CU) was built in round 4 for SMALL grids -- BASELINE config 2
// (8 x 448 x 256) is 896 tiles of 64 x 16 on 512 workgroup slots, 1.75 rounds of one tile's serial chain; as 1792 tiles of
// 64 x 8 on 1024 slots the chain per tile should have been shorter and the tail round half as long -- and LOST in one
// process (profiles/r04_fi_bwd_tile_height_ab.txt): config 2 72.9 -> 102.8 us, 720p 1436 -> 2134 us, i.i.d. flow 2.7x
// slower.  A box of 8 + 3 + motion rows holds 2.3x its tile's cells (64 x 16: 1.7x): the flush's atomics, the staged rows
// and the barriers per site all grow, and nothing in the chain got shorter.  Measurement arm 61 only.
template <int NT>
struct PkGeomT {
    static constexpr int kCap = 12 * NT;                               // pixel quads staged = slots per plane: 3 float4 per lane
    static constexpr int kImageBytes = kCap * 16;
    static constexpr int kLds = kImageBytes + 128;
};
using PkGeom = PkGeomT<256>;

// PART: 0 the whole backward; 1 the image gradient alone (planes, adds, flush); 2 the tap and flow gradients alone (staged
// image, phase 1).
//   * PART 2 is what a caller gets who passes gradinput1 == NULL: it does not want the image gradient (the reference's
//     networks never do: the frames they warp are data, MEMC_Net_star.py:266-277).  720p batch 32: 1037 us against 1432 us
//     for the whole backward on the same box (+ the 70 us zero fill of gradinput1 that the caller no longer needs);
//     BASELINE config 2 (8 x 448 x 256): 46.8 us against 72.9 (profiles/r04_fi_bwd_halves_ab.txt).
//   * PART 1 + PART 2 as two launches were round 4's second attempt at SMALL grids (config 2 is 896 tiles on 512 workgroup
//     slots: 1.75 rounds of a four-barrier chain; two shorter chains, and at 2/3 of the registers three workgroups per CU,
//     were to beat that).  They need 189 / 207 VGPRs: at three per CU (168) both spill inside their hot loops; at two per
//     CU the split reads the inputs twice and LOSES -- config 2 72.9 -> 83.1 us, 720p 1432 -> 1792 us.  Measurement arm 62.
#ifdef MEMC_PART_THREE
constexpr bool kPartThree = true;              // (experiment: the halves at three workgroups per CU -- 168 VGPRs, and they SPILL:
#else                                          //  96 / 160 B per lane, reloaded inside the add loop and phase 1)
constexpr bool kPartThree = false;
#endif

// the staging registers of the image box: fp32 quads, or half quads as two packed dwords (memc_lp.hpp)
template <class P>
using StageRegsOf = std::conditional_t<sizeof(st_t<P>) == 4, StageRegs<3>, LpStageRegs<3>>;

template <class P, bool RAG>
__device__ __forceinline__ void fi_bwd_stage_load(const Region &r, const StageSlot &sl, const st_t<P> *in_b, int64_t s1c,
                                                  int s1h, StageRegsOf<P> &sr)
{
    if constexpr (sizeof(st_t<P>) == 4) {
        tile_stage_load<3, RAG>(r, sl, in_b, s1c, s1h, sr);
    } else {
        const unsigned short *plane[3] = {in_b, in_b + s1c, in_b + 2 * s1c};
        lp_stage_load<3>(r, sl, plane, s1h, sr);
    }
}
// the staged rows' registers, touched: their loads are waited for HERE (see the kernel body)
template <class P>
__device__ __forceinline__ void fi_bwd_stage_touch(StageRegsOf<P> &sr)
{
#pragma unroll
    for (int it = 0; it < kStageIts; it++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if constexpr (sizeof(st_t<P>) == 4)
                asm volatile("" : "+v"(sr.v[it][c][0]), "+v"(sr.v[it][c][1]), "+v"(sr.v[it][c][2]), "+v"(sr.v[it][c][3]));
            else
                asm volatile("" : "+v"(sr.v[it][c].x), "+v"(sr.v[it][c].y));
        }
}
template <class P, bool RAG>
__device__ __forceinline__ void fi_bwd_stage_store(const Region &r, const StageSlot &sl, const StageRegsOf<P> &sr, f32x4 *tile)
{
    if constexpr (sizeof(st_t<P>) == 4) tile_stage_store<3, RAG>(r, sl, sr, tile);
    else lp_stage_store<P, 3>(r, sl, sr, tile);
}

}  // namespace memc
