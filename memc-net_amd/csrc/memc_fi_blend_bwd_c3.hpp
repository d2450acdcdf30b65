// memc_fi_blend_bwd_c3.hpp -- the backward of ONE direction of the dual warp + occlusion blend without the image gradient,
// RGB, fs == 4, LDS-tiled: the pieces of its kernel body (fi_blend_bwd_c3_body.inc), written once over the storage of the
// tensors (memc_lp.hpp: F32, F16, BF16).
//   fi_blend_bwd_c3.hip      fi_blend_bwd_c3: fp32 (libmemc_hip_blend_grad.so), the description of the algorithm;
//   mx_fi_blend_bwd_c3.hip   fi_blend_bwd_c3_mx: fp32 image and gradoutput, fp16 / bf16 taps and occlusion, fp32 or half flow
//                            (libmemc_hip_mx_blend_grad.so);
//   lp_fi_blend_bwd_c3.hip   fi_blend_bwd_c3_lp: fp16 / bf16 image, taps and occlusion, fp32 or half flow and gradoutput
//                            (libmemc_hip_lp_blend_grad.so).
// T: the storage of the taps, the occlusion and their gradients; FT: that of the flow and its gradient; I: the image's;
// GT: gradoutput's (I = GT = F32 in the first two).  Loads widen exactly, each stored gradient is rounded once: the LDS
// image and the arithmetic are the same for every storage, and the fp32 and mixed instantiations are the code their units
// had before the image's and gradoutput's storage were made parameters (tools/isa_diff.py).
#pragma once

#include "memc_common.hpp"
#include "memc_fi_bwd_c3.hpp"

namespace memc {

// fi_bwd_phase1 (memc_fi_bwd_c3.hpp) for the blend: quads whose four sites the band covers.  Same loop order and the same
// laundering -- read the comments there before rearranging anything: the nest lives on staying clear of spills.
// (oc * gt, oc * gx4 and gc4 are fp32 values: st4_stream_u rounds the quad it is given, see narrow_f32 of memc_lp.hpp.)
template <class T = F32, class FT = F32>
__device__ __forceinline__ void fi_blend_bwd_phase1(const Region &r, unsigned fast, FiSite4 &g, f32x4 (&tp)[16],
                                                    const f32x4 (&go)[3], const f32x4 &oc, const f32x4 *tile, int W, int H,
                                                    st_t<FT> *gflow_b, int64_t s2c, unsigned o2, st_t<T> *gfilt_b,
                                                    int64_t s3c, unsigned o3, st_t<T> *gocc_b, unsigned o4)
{
    MEMC_FI_LAUNDER(tp, g);                    // inside the caller's band loop
    if (fast != 0xFu) return;                  // mixed quads: site by site (fi_blend_bwd_site)
    f32x4 gx4 = {0.f, 0.f, 0.f, 0.f}, gy4 = gx4, gc4 = gx4;
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
            f32x4 gt;                          // gt[j]: the warp's gradient of tap (k, m) of site j
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
                gc4[j] += gt[j] * tp[k * 4 + m][j];
            }
            st4_stream_u<T>(gfilt_b + (k * 4 + m) * s3c, o3, oc * gt);
        }
    }
    st4_stream_u<FT>(gflow_b, o2, oc * gx4);
    st4_stream_u<FT>(gflow_b + s2c, o2, oc * gy4);
    st4_stream_u<T>(gocc_b, o4, gc4);
}

// The three gradients of ONE site straight from global memory (fi_bwd_site_taps of memc_fi.hpp with the occlusion): mixed
// quads and sites that no band covers.  An invalid site keeps what fi_blend_bwd_store_invalid stored.  A macro body,
// expanded in the fp32 unit's named function and in the mixed and half templates (see memc_fi.hpp on why not a forwarding
// call); halves are read through widen_f32, so that the compiler sees fp32 operands as in the fp32 function.
#define MEMC_FI_BLEND_BWD_SITE_BODY(T, FT, IM, GT)                                                                          \
    {                                                                                                                 \
        const FiSite s = fi_locate(x, y, W, H, widen_f32<FT>(flow_p[0]), widen_f32<FT>(flow_p[s2c]));                 \
        if (!s.valid) return;                                                                                         \
        const float g0 = widen_f32<GT>(gout_p[0]), g1 = widen_f32<GT>(gout_p[s1c]),                                   \
                    gc2 = widen_f32<GT>(gout_p[2 * s1c]), oc = widen_f32<T>(occ_p[0]);                                \
        float gx = 0.0f, gy = 0.0f, gc = 0.0f;                                                                        \
        for (int k = 0; k < 4; k++) {                                                                                 \
            const st_t<IM> *row = in_b + (int64_t)clampi(s.iy - 1 + k, H - 1) * s1h;                                  \
            for (int m = 0; m < 4; m++) {                                                                             \
                const st_t<IM> *p = row + clampi(s.ix - 1 + m, W - 1);                                                \
                float sv = 0.0f;                                                                                      \
                sv += g0 * widen_f32<IM>(p[0]);  sv += g1 * widen_f32<IM>(p[s1c]);  sv += gc2 * widen_f32<IM>(p[2 * s1c]); \
                const float wa = m < 2 ? (1 - s.a) : s.a, wb = k < 2 ? (1 - s.b) : s.b;                               \
                const float gt = (wa * wb) * sv, tap = widen_f32<T>(tap_p[(k * 4 + m) * s3c]);                        \
                g3[(k * 4 + m) * s3c] = narrow_f32<T>(oc * gt);                                                       \
                const float st = sv * tap;                                                                            \
                gx += (m < 2 ? -wb : wb) * st;                                                                        \
                gy += (k < 2 ? -wa : wa) * st;                                                                        \
                gc += gt * tap;                                                                                       \
            }                                                                                                         \
        }                                                                                                             \
        g2[0] = narrow_f32<FT>(oc * gx);                                                                              \
        g2[s2c] = narrow_f32<FT>(oc * gy);                                                                            \
        gocc_p[0] = narrow_f32<T>(gc);                                                                                \
    }
__device__ __noinline__ inline void fi_blend_bwd_site(int x, int y, int W, int H, const float *in_b, int64_t s1c, int s1h,
                                                      const float *flow_p, float *g2, int64_t s2c, const float *tap_p,
                                                      float *g3, int64_t s3c, const float *gout_p, const float *occ_p,
                                                      float *gocc_p)
MEMC_FI_BLEND_BWD_SITE_BODY(F32, F32, F32, F32)
template <class T, class FT>
__device__ __noinline__ void fi_blend_bwd_site_mx(int x, int y, int W, int H, const float *in_b, int64_t s1c, int s1h,
                                                  const st_t<FT> *flow_p, st_t<FT> *g2, int64_t s2c, const st_t<T> *tap_p,
                                                  st_t<T> *g3, int64_t s3c, const float *gout_p, const st_t<T> *occ_p,
                                                  st_t<T> *gocc_p)
MEMC_FI_BLEND_BWD_SITE_BODY(T, FT, F32, F32)
// the same with the image stored as the taps are and a gradoutput of storage GT (libmemc_hip_lp_blend_grad.so)
template <class T, class FT, class GT>
__device__ __noinline__ void fi_blend_bwd_site_lp(int x, int y, int W, int H, const st_t<T> *in_b, int64_t s1c, int s1h,
                                                  const st_t<FT> *flow_p, st_t<FT> *g2, int64_t s2c, const st_t<T> *tap_p,
                                                  st_t<T> *g3, int64_t s3c, const st_t<GT> *gout_p, const st_t<T> *occ_p,
                                                  st_t<T> *gocc_p)
MEMC_FI_BLEND_BWD_SITE_BODY(T, FT, T, GT)
#undef MEMC_FI_BLEND_BWD_SITE_BODY

// A quad that contains an invalid site first stores its 16 + 2 + 1 quads: zeros to the tap and flow gradients
// (fi_bwd_zero_invalid), and to the occlusion gradient, per site, 0 where the site is valid and sum_c gout_c * in_c(x, y)
// where it is not -- the forward copies the input pixel at a site whose target lies outside the image, so that is what
// the occlusion multiplies there (summed in fp32, narrowed once).  The quad's valid sites are then stored site by site by
// the same lane, and therefore after these.  (oi: the byte offset of the quad in the image's planes, of storage IM.)
template <class T = F32, class FT = F32, class IM = F32>
__device__ __forceinline__ void fi_blend_bwd_store_invalid(bool inb, unsigned valid, const f32x4 (&go)[3],
                                                           const st_t<IM> *in_b, int64_t s1c, unsigned oi,
                                                           st_t<FT> *gflow_b, int64_t s2c,
                                                           unsigned o2, st_t<T> *gfilt_b, int64_t s3c, unsigned o3,
                                                           st_t<T> *gocc_b, unsigned o4)
{
    fi_bwd_zero_invalid<T, FT>(inb, valid, gflow_b, s2c, o2, gfilt_b, s3c, o3);
    if (!inb || valid == 0xFu) return;         // rare (image borders, |flow| guard): ordinary 64-bit addressing
    f32x4 gc = {0.f, 0.f, 0.f, 0.f};
    if constexpr (sizeof(st_t<IM>) == 4) {
        const float *p = in_b + oi / 4u;
#pragma unroll
        for (int c = 0; c < 3; c++) gc += go[c] * *reinterpret_cast<const f32x4u *>(p + c * s1c);
    } else {
        const st_t<IM> *p = in_b + oi / 2u;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            f32x4 px = widen4<IM>(*reinterpret_cast<const u16x4a *>(p + c * s1c));
            asm volatile("" : "+v"(px));       // an fp32 operand, as in the fp32 kernel (widen_f32 of memc_lp.hpp)
            gc += go[c] * px;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) gc[j] = ((valid >> j) & 1u) ? 0.0f : gc[j];
    if constexpr (sizeof(st_t<T>) == 4) {
        *reinterpret_cast<f32x4u *>(gocc_b + o4 / 4u) = gc;
    } else {
        const u16x4 q = {narrow_f32<T>(gc[0]), narrow_f32<T>(gc[1]), narrow_f32<T>(gc[2]), narrow_f32<T>(gc[3])};
        *reinterpret_cast<u16x4a *>(gocc_b + o4 / 2u) = q;
    }
}

}  // namespace memc
