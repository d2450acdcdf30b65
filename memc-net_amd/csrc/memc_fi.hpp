// memc_fi.hpp -- the per-site device helpers of every FilterInterpolation kernel, forward and backward, fp32 and half
// storage (filter_interpolation.hip, fi_bwd_c3.hip, fi_bwd_cn.hip, fi_blend_bwd_c3.hip, lp_filter_interpolation.hip,
// lp_fi_bwd_c3.hip, lp_fi_blend_bwd_c3.hip, mx_filter_interpolation.hip, mx_fi_bwd_c3.hip, mx_fi_blend_bwd_c3.hip, arms/;
// the satellites' host side: memc_fi_abi.hpp):
// the geometry of a lane's four sites, the LDS gather, the one-site paths from global memory.
//
// What the fp32 kernels and their half twins share is written ONCE here, as a macro wherever a shared always-inline
// function would be the same source but not the same machine code in the fp32 libraries (the inlined call changes the
// compiler's scheduling, vectorisation and contraction choices; tools/isa_diff.py is the check), and as a template over
// the storage (memc_lp.hpp) wherever it is not.
#pragma once

#include "memc_tile.hpp"
#include "memc_lp.hpp"

namespace memc {

struct FiSite4 {          // geometry of a lane's four sites
    int ix[4], iy[4];
    float a[4], b[4];
    unsigned valid;       // bit j
};

// sites of this lane whose (clamped) window lies inside the band
__device__ __forceinline__ unsigned fi_covered(const Region &r, const FiSite4 &g, int W, int H)
{
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (((g.valid >> j) & 1) &&
            r.covers(max(g.ix[j] - 1, 0), min(g.ix[j] + 2, W - 1), max(g.iy[j] - 1, 0), min(g.iy[j] + 2, H - 1)))
            m |= 1u << j;
    return m;
}

// Site geometry of the lane's four sites (x .. x + 3 of row y) and the box of their clamped 4 x 4 windows: declares the
// FiSite4 `g` and cmin, cmax, rmin, rmax (no valid site: INT_MAX / -1) in the enclosing scope.
#define MEMC_FI_SITES(g, x, y, W, H, inb, fx4, fy4)                                                                   \
    FiSite4 g;                                                                                                        \
    g.valid = 0;                                                                                                      \
    int cmin = INT_MAX, cmax = -1, rmin = INT_MAX, rmax = -1;                                                         \
    _Pragma("unroll")                                                                                                 \
    for (int j = 0; j < 4; j++) {                                                                                     \
        const FiSite s = fi_locate((x) + j, (y), (W), (H), (fx4)[j], (fy4)[j]);                                       \
        g.ix[j] = s.ix; g.iy[j] = s.iy; g.a[j] = s.a; g.b[j] = s.b;                                                   \
        if ((inb) && s.valid) {                                                                                       \
            g.valid |= 1u << j;                                                                                       \
            cmin = min(cmin, max(s.ix - 1, 0));  cmax = max(cmax, min(s.ix + 2, (W) - 1));                            \
            rmin = min(rmin, max(s.iy - 1, 0));  rmax = max(rmax, min(s.iy + 2, (H) - 1));                            \
        }                                                                                                             \
    }

// Everything a band or chunk body derives from the taps and the site geometry (tap splats for the packed FMAs, 64 LDS
// addresses, blend weights) is loop-invariant; hoisted out of the loop it needs ~400 more registers than exist and lands
// in scratch (1.5 KB per lane in fi_fwd_tiled_fs4's chunk loop).  Laundering the inputs through empty asm statements once
// per iteration keeps that arithmetic inside the loop.
#define MEMC_FI_LAUNDER(tp, g)                                                                                        \
    do {                                                                                                              \
        _Pragma("unroll")                                                                                             \
        for (int k = 0; k < 16; k++)                                                                                  \
            asm volatile("" : "+v"((tp)[k][0]), "+v"((tp)[k][1]), "+v"((tp)[k][2]), "+v"((tp)[k][3]));                \
        _Pragma("unroll")                                                                                             \
        for (int j = 0; j < 4; j++) asm volatile("" : "+v"((g).ix[j]), "+v"((g).iy[j]), "+v"((g).a[j]), "+v"((g).b[j])); \
    } while (0)

// Gather + blend of the sites selected by `sel` (bit j) from the staged band; other sites keep their `res`.
// Branch-free: unselected sites still issue their 16 LDS reads (at pixel 0, harmless).  The LDS image is fp32 pixel
// quads for every storage (staging widens), so this is the gather of the fp32 and of the half kernels.
template <int LX, int NCH>
__device__ __forceinline__ void fi_gather(const Region &r, const FiSite4 &g, const f32x4 (&tp)[16], unsigned sel,
                                          int W, int H, const f32x4 *tile, f32x4 (&res)[4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool on = (sel >> j) & 1;
        int ro[4], co[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            ro[k] = on ? (clampi(g.iy[j] - 1 + k, H - 1) - r.y0) * r.pitch : 0;
            co[k] = on ? swz_col(clampi(g.ix[j] - 1 + k, W - 1) - r.x0) : 0;
        }
        // quadrant sums, row-major inside each quadrant as in the reference (rows 0,1 top; 2,3 bottom)
        f32x4 TL = {0.f, 0.f, 0.f, 0.f}, TR = TL, BL = TL, BR = TL;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            f32x4 v[4];
#pragma unroll
            for (int m = 0; m < 4; m++) v[m] = tile[ro[k] + co[m]];
            if (k < 2) {
                TL += v[0] * tp[k * 4 + 0][j];  TL += v[1] * tp[k * 4 + 1][j];
                TR += v[2] * tp[k * 4 + 2][j];  TR += v[3] * tp[k * 4 + 3][j];
            } else {
                BL += v[0] * tp[k * 4 + 0][j];  BL += v[1] * tp[k * 4 + 1][j];
                BR += v[2] * tp[k * 4 + 2][j];  BR += v[3] * tp[k * 4 + 3][j];
            }
        }
        const float a = g.a[j], bt = g.b[j];
        const f32x4 val = ((1 - a) * (1 - bt)) * TL + (a * (1 - bt)) * TR + ((1 - a) * bt) * BL + (a * bt) * BR;
        res[j] = on ? val : res[j];
    }
}

// One quadrant sum of one channel of one site, everything read from global memory, any filter size: row-major from 0,
// the reference's order.  P: the storage of the image and the taps (memc_lp.hpp: F32, or F16 / BF16 widened exactly at
// the load).  I: the type of a row offset -- int where the C ABI hands the kernels `int` strides or the launcher has
// checked the plane (every fp32 kernel, the half backward); int64_t in the half forward, whose one-lane-per-site kernel
// takes any plane.  TP: the storage of the taps where it is not the image's (the mixed forward: an fp32 image, half taps).
template <class P = F32, class I = int, class TP = P>
__device__ __forceinline__ float fi_quad_sum(const st_t<P> *p, int s1h, int W, int H, const st_t<TP> *tap_p,
                                             int64_t s3c, int fs, int L, int T, int j0, int j1, int i0, int i1)
{
    float acc = 0.0f;
    for (int j = j0; j <= j1; j++) {
        const I jj = (I)clampi(j, H - 1) * s1h;
        for (int i = i0; i <= i1; i++)
            acc += widen_f32<P>(p[jj + clampi(i, W - 1)]) * widen_f32<TP>(tap_p[((j - T) * fs + (i - L)) * s3c]);
    }
    return acc;
}

// One channel of one valid site from global memory: the four quadrant sums over the site's fs x fs window, columns
// [L, R) and rows [T, Bm) with L = ix + 1 - fs / 2, T = iy + 1 - fs / 2, then the four-term blend.  The window is the
// caller's, computed once for all channels and handed over as four ints: as a struct, or computed in here, the fp32
// callers compile to other machine code.
template <class P = F32, class I = int, class TP = P>
__device__ __forceinline__ float fi_site_chan(const FiSite &s, int fs, int L, int T, int R, int Bm, int W, int H,
                                              const st_t<P> *p, int s1h, const st_t<TP> *tap_p, int64_t s3c)
{
    const float TL = fi_quad_sum<P, I, TP>(p, s1h, W, H, tap_p, s3c, fs, L, T, T, s.iy, L, s.ix);
    const float TR = fi_quad_sum<P, I, TP>(p, s1h, W, H, tap_p, s3c, fs, L, T, T, s.iy, s.ix + 1, R - 1);
    const float BL = fi_quad_sum<P, I, TP>(p, s1h, W, H, tap_p, s3c, fs, L, T, s.iy + 1, Bm - 1, L, s.ix);
    const float BR = fi_quad_sum<P, I, TP>(p, s1h, W, H, tap_p, s3c, fs, L, T, s.iy + 1, Bm - 1, s.ix + 1, R - 1);
    return (1 - s.a) * (1 - s.b) * TL + s.a * (1 - s.b) * TR + (1 - s.a) * s.b * BL + s.a * s.b * BR;
}

// ONE site of the forward for channels [0, nch) of `plane0`, everything read from global memory (flow, taps, image): the
// rare path for sites whose source window no staged LDS band covers, and the body of the half library's one-lane-per-site
// kernel.  Same arithmetic order as the fast path; an out-of-range site copies the input pixel.  FT: the storage of the
// flow; TP: that of the taps.  A macro body, expanded in fi_site_scalar (filter_interpolation.hip: the fp32 library's
// named function) and in fi_site_scalar_lp / fi_site_scalar_mx below: behind a forwarding call the fp32 function compiles
// to other machine code.
#define MEMC_FI_SITE_SCALAR_BODY(P, FT, I, TP)                                                                        \
    {                                                                                                                 \
        const float fx = widen<FT>(flow_p[0]), fy = widen<FT>(flow_p[s2c]);                                           \
        const FiSite s = fi_locate(x, y, W, H, fx, fy);                                                               \
        if (s.valid) {                                                                                                \
            const int L = s.ix + 1 - fs / 2, T = s.iy + 1 - fs / 2, R = L + fs, Bm = T + fs;                          \
            for (int c = 0; c < nch; c++)                                                                             \
                out_p[c * s1c] = narrow<P>(fi_site_chan<P, I, TP>(s, fs, L, T, R, Bm, W, H, plane0 + c * s1c, s1h, tap_p, s3c)); \
        } else {                                                                                                      \
            const st_t<P> *p = plane0 + (int64_t)y * s1h + x;                                                         \
            for (int c = 0; c < nch; c++) out_p[c * s1c] = p[c * s1c];                                                \
        }                                                                                                             \
    }
template <class P, class FT>
__device__ __noinline__ void fi_site_scalar_lp(int x, int y, int W, int H, int nch, int fs, const st_t<P> *plane0,
                                               int64_t s1c, int s1h, const st_t<FT> *flow_p, int64_t s2c,
                                               const st_t<P> *tap_p, int64_t s3c, st_t<P> *out_p)
MEMC_FI_SITE_SCALAR_BODY(P, FT, int64_t, P)
// the same for an image and an output of storage P beside taps of storage TP (the mixed forward, libmemc_hip_mx.so)
template <class P, class FT, class TP>
__device__ __noinline__ void fi_site_scalar_mx(int x, int y, int W, int H, int nch, int fs, const st_t<P> *plane0,
                                               int64_t s1c, int s1h, const st_t<FT> *flow_p, int64_t s2c,
                                               const st_t<TP> *tap_p, int64_t s3c, st_t<P> *out_p)
MEMC_FI_SITE_SCALAR_BODY(P, FT, int64_t, TP)

// The per-site backward helpers below are written once over the storage of their tensors (memc_lp.hpp): P for the taps
// and the tap gradient, IM for the image (P itself in the fp32 functions and the *_lp templates; the *_mx templates of
// libmemc_hip_mx_grad.so take it apart: an fp32 image beside half taps), FT for the flow and its gradient, GT for
// gradoutput; the image gradient is always fp32 (it takes atomics).  Every load widens exactly, every result is rounded once when it is stored: for the same (widened)
// inputs a half instantiation computes the fp32 one's values.  The bodies are macros, expanded in the fp32 functions of
// libmemc_hip.so (fi_bwd_site_scalar, fi_bwd_site_taps) and in the *_lp templates of libmemc_hip_lp_grad.so: a forwarding
// call to a shared always-inline template would be the same source but not the same machine code (the inlined call
// changes the compiler's vectorisation and contraction choices), and the fp32 kernels keep theirs bit for bit.

// One site of the backward, everything from global memory, image gradient with global atomics: the rare path for
// sites that no LDS band covers, and the body of the any-filter-size kernel (my_lib_kernel.cu:1248-1515).
// The tap gradient is a sum over the channels: fp32 taps accumulate it in memory (g3[k] +=, exact in fp32); half taps
// may not (each add would be rounded to T), so their sums are formed in a register from the same terms in the same
// order, behind the channel loop, and stored once.
#define MEMC_FI_BWD_SITE_SCALAR_BODY(P, FT, GT, IM)                                                                   \
    {                                                                                                                 \
        constexpr bool kMem = sizeof(st_t<P>) == 4;                                                                   \
        const float fx = widen_f32<FT>(flow_p[0]), fy = widen_f32<FT>(flow_p[s2c]);                                   \
        const FiSite s = fi_locate(x, y, W, H, fx, fy);                                                               \
        if (!s.valid) return;                                                                                         \
        const int L = s.ix + 1 - fs / 2, T = s.iy + 1 - fs / 2, R = L + fs, Bm = T + fs;                              \
        float botx = 0.0f, boty = 0.0f;                                                                               \
        const float gam_x = 1.0f - s.b, gam_y = 1.0f - s.a;                                                           \
        for (int c = 0; c < C; c++) {                                                                                 \
            const st_t<IM> *p = in_b + c * s1c;                                                                       \
            float *q = gin1_b + c * s1c;                                                                              \
            const float g = widen_f32<GT>(gout_p[c * s1c]);                                                           \
            for (int j = T; j < Bm; j++) {                                                                            \
                const int jj = clampi(j, H - 1) * s1h;                                                                \
                for (int i = L; i < R; i++) {                                                                         \
                    const int ii = clampi(i, W - 1);                                                                  \
                    const float wgt = (j <= s.iy) ? ((i <= s.ix) ? g * (1 - s.a) * (1 - s.b) : g * s.a * (1 - s.b))   \
                                                  : ((i <= s.ix) ? g * (1 - s.a) * s.b : g * s.a * s.b);              \
                    const int64_t k = ((j - T) * fs + (i - L)) * s3c;                                                 \
                    atomic_add_f32(q + jj + ii, wgt * widen_f32<P>(tap_p[k]));                                        \
                    if constexpr (kMem) {                                                                             \
                        if (c == 0) g3[k] = wgt * p[jj + ii]; else g3[k] += wgt * p[jj + ii];                         \
                    }                                                                                                 \
                }                                                                                                     \
            }                                                                                                         \
            const float TL = fi_quad_sum<IM, int, P>(p, s1h, W, H, tap_p, s3c, fs, L, T, T, s.iy, L, s.ix);           \
            const float TR = fi_quad_sum<IM, int, P>(p, s1h, W, H, tap_p, s3c, fs, L, T, T, s.iy, s.ix + 1, R - 1);   \
            const float BL = fi_quad_sum<IM, int, P>(p, s1h, W, H, tap_p, s3c, fs, L, T, s.iy + 1, Bm - 1, L, s.ix);  \
            const float BR = fi_quad_sum<IM, int, P>(p, s1h, W, H, tap_p, s3c, fs, L, T, s.iy + 1, Bm - 1, s.ix + 1, R - 1); \
            float tmp = 0.0f;                                                                                         \
            tmp += gam_x * (TR - TL);                                                                                 \
            tmp += (1.0f - gam_x) * (BR - BL);                                                                        \
            botx += g * tmp;                                                                                          \
            tmp = 0.0f;                                                                                               \
            tmp += gam_y * (BL - TL);                                                                                 \
            tmp += (1.0f - gam_y) * (BR - TR);                                                                        \
            boty += g * tmp;                                                                                          \
        }                                                                                                             \
        if constexpr (!kMem) {   /* half taps: each tap's channel sum above, same terms, same order, in a register */ \
            for (int j = T; j < Bm; j++) {                                                                            \
                const int jj = clampi(j, H - 1) * s1h;                                                                \
                for (int i = L; i < R; i++) {                                                                         \
                    const int ii = clampi(i, W - 1);                                                                  \
                    float a3 = 0.0f;                                                                                  \
                    for (int c = 0; c < C; c++) {                                                                     \
                        const float g = widen_f32<GT>(gout_p[c * s1c]);                                               \
                        const float wgt = (j <= s.iy) ? ((i <= s.ix) ? g * (1 - s.a) * (1 - s.b) : g * s.a * (1 - s.b)) \
                                                      : ((i <= s.ix) ? g * (1 - s.a) * s.b : g * s.a * s.b);          \
                        const st_t<IM> *p = in_b + c * s1c;                                                           \
                        /* the fp32 function's `g3[k] += wgt * p` is a rounded product and an add (v_mul, v_add: its */ \
                        /* store of channel 0 sits between them); here the loop unrolls and the compiler would       */ \
                        /* contract the adds into fmas -- a last-bit difference that flips about one rounding to T   */ \
                        /* in 2^13.  The asm keeps the product a value of its own.                                   */ \
                        float t3 = wgt * widen_f32<IM>(p[jj + ii]);                                                   \
                        asm volatile("" : "+v"(t3));                                                                  \
                        if (c == 0) a3 = t3; else a3 += t3;                                                           \
                    }                                                                                                 \
                    g3[((j - T) * fs + (i - L)) * s3c] = narrow_f32<P>(a3);                                           \
                }                                                                                                     \
            }                                                                                                         \
        }                                                                                                             \
        g2[0] = narrow_f32<FT>(botx);                                                                                 \
        g2[s2c] = narrow_f32<FT>(boty);                                                                               \
    }
__device__ __noinline__ inline void fi_bwd_site_scalar(int x, int y, int W, int H, int C, int fs,
                                                const float *in_b, float *gin1_b, int64_t s1c, int s1h,
                                                const float *flow_p, float *g2, int64_t s2c,
                                                const float *tap_p, float *g3, int64_t s3c, const float *gout_p)
MEMC_FI_BWD_SITE_SCALAR_BODY(F32, F32, F32, F32)
template <class P, class FT, class GT>
__device__ __noinline__ void fi_bwd_site_scalar_lp(int x, int y, int W, int H, int C, int fs, const st_t<P> *in_b,
                                                   float *gin1_b, int64_t s1c, int s1h, const st_t<FT> *flow_p,
                                                   st_t<FT> *g2, int64_t s2c, const st_t<P> *tap_p, st_t<P> *g3,
                                                   int64_t s3c, const st_t<GT> *gout_p)
MEMC_FI_BWD_SITE_SCALAR_BODY(P, FT, GT, P)
// the same with an image of storage IM beside taps of storage P (the mixed backward, libmemc_hip_mx_grad.so)
template <class P, class FT, class GT, class IM>
__device__ __noinline__ void fi_bwd_site_scalar_mx(int x, int y, int W, int H, int C, int fs, const st_t<IM> *in_b,
                                                   float *gin1_b, int64_t s1c, int s1h, const st_t<FT> *flow_p,
                                                   st_t<FT> *g2, int64_t s2c, const st_t<P> *tap_p, st_t<P> *g3,
                                                   int64_t s3c, const st_t<GT> *gout_p)
MEMC_FI_BWD_SITE_SCALAR_BODY(P, FT, GT, IM)
#undef MEMC_FI_BWD_SITE_SCALAR_BODY


// gradinput3 and gradinput2 of ONE site straight from global memory (mixed quads of the tiled RGB backward: some of a
// lane's four sites belong to another band or are invalid).  Assigns both, like the tiled path; the image
// gradient of such a site still goes through the tile's LDS planes.
#define MEMC_FI_BWD_SITE_TAPS_BODY(P, FT, GT, IM)                                                                     \
    {                                                                                                                 \
        const FiSite s = fi_locate(x, y, W, H, widen_f32<FT>(flow_p[0]), widen_f32<FT>(flow_p[s2c]));                 \
        if (!s.valid) return;                                                                                         \
        const float g0 = widen_f32<GT>(gout_p[0]), g1 = widen_f32<GT>(gout_p[s1c]), gc2 = widen_f32<GT>(gout_p[2 * s1c]); \
        float gx = 0.0f, gy = 0.0f;                                                                                   \
        for (int k = 0; k < 4; k++) {                                                                                 \
            const st_t<IM> *row = in_b + (int64_t)clampi(s.iy - 1 + k, H - 1) * s1h;                                  \
            for (int m = 0; m < 4; m++) {                                                                             \
                const st_t<IM> *p = row + clampi(s.ix - 1 + m, W - 1);                                                \
                float sv = 0.0f;                                                                                      \
                sv += g0 * widen_f32<IM>(p[0]);  sv += g1 * widen_f32<IM>(p[s1c]);  sv += gc2 * widen_f32<IM>(p[2 * s1c]); \
                const float wa = m < 2 ? (1 - s.a) : s.a, wb = k < 2 ? (1 - s.b) : s.b;                               \
                g3[(k * 4 + m) * s3c] = narrow_f32<P>((wa * wb) * sv);                                                \
                const float st = sv * widen_f32<P>(tap_p[(k * 4 + m) * s3c]);                                         \
                gx += (m < 2 ? -wb : wb) * st;                                                                        \
                gy += (k < 2 ? -wa : wa) * st;                                                                        \
            }                                                                                                         \
        }                                                                                                             \
        g2[0] = narrow_f32<FT>(gx);                                                                                   \
        g2[s2c] = narrow_f32<FT>(gy);                                                                                 \
    }
__device__ __noinline__ inline void fi_bwd_site_taps(int x, int y, int W, int H, const float *in_b, int64_t s1c, int s1h,
                                              const float *flow_p, float *g2, int64_t s2c, const float *tap_p,
                                              float *g3, int64_t s3c, const float *gout_p)
MEMC_FI_BWD_SITE_TAPS_BODY(F32, F32, F32, F32)
template <class P, class FT, class GT>
__device__ __noinline__ void fi_bwd_site_taps_lp(int x, int y, int W, int H, const st_t<P> *in_b, int64_t s1c, int s1h,
                                                 const st_t<FT> *flow_p, st_t<FT> *g2, int64_t s2c, const st_t<P> *tap_p,
                                                 st_t<P> *g3, int64_t s3c, const st_t<GT> *gout_p)
MEMC_FI_BWD_SITE_TAPS_BODY(P, FT, GT, P)
template <class P, class FT, class GT, class IM>
__device__ __noinline__ void fi_bwd_site_taps_mx(int x, int y, int W, int H, const st_t<IM> *in_b, int64_t s1c, int s1h,
                                                 const st_t<FT> *flow_p, st_t<FT> *g2, int64_t s2c, const st_t<P> *tap_p,
                                                 st_t<P> *g3, int64_t s3c, const st_t<GT> *gout_p)
MEMC_FI_BWD_SITE_TAPS_BODY(P, FT, GT, IM)
#undef MEMC_FI_BWD_SITE_TAPS_BODY

// gradinput2 / gradinput3 are fully DEFINED by the backward kernels (the Python layer hands them over
// uninitialised -- their memsets were 72 B/site, a seventh of the call): a quad that contains an invalid site
// first stores zeros to its 16 + 2 float4; its valid sites are then stored site by site (fi_bwd_site_taps), by the
// same lane and therefore after these.  Quads of four valid sites are stored by phase 1 or by fi_bwd_site_taps.
// (o2 / o3: byte offsets; a half quad is 8 bytes, 8-byte aligned.)
template <class P = F32, class FT = F32>
__device__ __forceinline__ void fi_bwd_zero_invalid(bool inb, unsigned valid, st_t<FT> *gin2_b, int64_t s2c, unsigned o2,
                                                    st_t<P> *gin3_b, int64_t s3c, unsigned o3)
{
    if (!inb || valid == 0xFu) return;         // rare (image borders, |flow| guard): ordinary 64-bit addressing
    st_t<P> *q3 = gin3_b + (o3 / (unsigned)sizeof(st_t<P>));
    st_t<FT> *q2 = gin2_b + (o2 / (unsigned)sizeof(st_t<FT>));
    auto zero4 = [](auto *q) {
        if constexpr (sizeof(*q) == 4) *reinterpret_cast<f32x4u *>(q) = f32x4{0.f, 0.f, 0.f, 0.f};
        else *reinterpret_cast<u16x4a *>(q) = u16x4{0, 0, 0, 0};
    };
#pragma unroll 1
    for (int k = 0; k < 16; k++) zero4(q3 + k * s3c);
    zero4(q2);
    zero4(q2 + s2c);
}

}  // namespace memc
