// memc_spynet_level.hpp -- the site arithmetic of one SPyNet pyramid level, shared as text by the forward unit
// (spynet_level.hip, libmemc_hip_spynet.so), the backward unit (spynet_level_bwd.hip, libmemc_hip_spynet_grad.so) and the
// fp16 / bf16 forward unit (lp_spynet_level.hip, libmemc_hip_spynet_lp.so): the x2 upsampling's index rule, the clamped
// sample position, what the sites of a row share, the doubled upsampled flow of a site, the corner set-up of its bilinear
// sample and the site body of the forward.  The backward recomputes `up` and the position by these, so both directions see
// the same corners and weights.  Device code only; no object is shared between the three libraries.
//
// The functions that touch storage (level_flow, level_site) take the storage tag S of memc_lp.hpp -- F32 by default, which is
// what the two fp32 units instantiate: their device code is what it was before the tag existed.  For F16 / BF16 every element
// is widened exactly as it is read and handed on as an opaque fp32 value (widen_f32): from there the compiler sees the fp32
// units' expressions, so it contracts the same products and sums.
#pragma once

#include "memc_common.hpp"
#include "memc_lp.hpp"

namespace memc {

// ATen's area_pixel_compute_source_index (flow_prologue.hip's up_index restates the same rule): source index and weights
// of destination index `dst` among `in` samples.  align_corners: index and weight come from the ROUNDED product -- the
// barrier keeps the compiler from contracting `src - i0` into an fma off the unrounded one.  Without align_corners there is
// nothing to guard, which is why the barrier is on one branch only: the scale is 0.5, so 0.5 * (dst + 0.5) - 0.5 is exact
// however it is contracted.
__device__ __forceinline__ void level_up_index(int dst, int in, float scale, bool align, int &i0, int &i1, float &l0, float &l1)
{
    float src = align ? scale * (float)dst : fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.0f);
    if (align) asm volatile("" : "+v"(src));
    i0 = min((int)src, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.0f - l1;
}

// the sample position along one axis, clamped; a NaN fails the first comparison and becomes -2
__device__ __forceinline__ float level_position(int x, float f, int n, float k, bool align)
{
    float p = (float)x + f;
    if (!align) p = p * k - 0.5f;
    p = p > -2.0f ? p : -2.0f;
    return p < (float)(n + 1) ? p : (float)(n + 1);
}

struct LevelRow {                              // what the sites of one output row share: the coarse rows and their weights
    int o0, o1;                                // element offsets of coarse rows y0, y1
    float l0, l1;
};

// the doubled upsampled flow (ux, uy) of site x in the row `r`, from a coarse flow stored as S
template <class S = F32>
__device__ __forceinline__ void level_flow(int x, int w, float sx, bool align_up, const LevelRow &r,
                                           const st_t<S> *__restrict__ cb, int64_t scc, float &ux, float &uy)
{
    int x0, x1;
    float lx0, lx1;
    level_up_index(min(x, 2 * w - 1), w, sx, align_up, x0, x1, lx0, lx1);      // a padded column repeats column 2w - 1
    const st_t<S> *c0 = cb, *c1 = cb + scc;
    const float a0 = widen_f32<S>(c0[r.o0 + x0]), b0 = widen_f32<S>(c0[r.o0 + x1]);
    const float d0 = widen_f32<S>(c0[r.o1 + x0]), e0 = widen_f32<S>(c0[r.o1 + x1]);
    const float a1 = widen_f32<S>(c1[r.o0 + x0]), b1 = widen_f32<S>(c1[r.o0 + x1]);
    const float d1 = widen_f32<S>(c1[r.o1 + x0]), e1 = widen_f32<S>(c1[r.o1 + x1]);
    ux = 2.0f * (r.l0 * (lx0 * a0 + lx1 * b0) + r.l1 * (lx0 * d0 + lx1 * e0));
    uy = 2.0f * (r.l0 * (lx0 * a1 + lx1 * b1) + r.l1 * (lx0 * d1 + lx1 * e1));
}

// The four corners of the bilinear sample at the clamped position (px, py): the weights' factors, the in-range tests, and
// the column indices and row offsets clamped into the image -- a corner is read at its clamped index and selected, not
// multiplied, by its test.
struct LevelCorners {
    float ax, ay, bx, by;
    bool inx0, inx1, iny0, iny1;
    int cx0, cx1, r0, r1;
};

__device__ __forceinline__ LevelCorners level_corners(float px, float py, int W, int H, int ssh)
{
    LevelCorners k;
    const float fx0 = floorf(px), fy0 = floorf(py);
    const int ix = (int)fx0, iy = (int)fy0;                                    // within [-2, W + 1], [-2, H + 1]
    k.ax = px - fx0, k.ay = py - fy0, k.bx = (fx0 + 1.0f) - px, k.by = (fy0 + 1.0f) - py;
    k.inx0 = ix >= 0 && ix < W, k.inx1 = ix + 1 >= 0 && ix + 1 < W;
    k.iny0 = iy >= 0 && iy < H, k.iny1 = iy + 1 >= 0 && iy + 1 < H;
    k.cx0 = clampi(ix, W - 1), k.cx1 = clampi(ix + 1, W - 1);
    k.r0 = clampi(iy, H - 1) * ssh, k.r1 = clampi(iy + 1, H - 1) * ssh;
    return k;
}

// One site of the forward: the doubled upsampled flow (ux, uy) and the three channels of `second` sampled at (x, y) + it,
// all in fp32 from a coarse flow and a second frame stored as S.  The warp uses (ux, uy) as they are: a unit that stores
// them narrower rounds them where it stores them.
template <class S = F32>
__device__ __forceinline__ void level_site(int x, int y, int W, int H, int w, float sx, float kx, float ky, bool align_up,
                                           bool align_sample, const LevelRow &r, const st_t<S> *__restrict__ cb, int64_t scc,
                                           const st_t<S> *__restrict__ sb, int64_t ssc, int ssh, float &ux, float &uy,
                                           float (&warped)[3])
{
    level_flow<S>(x, w, sx, align_up, r, cb, scc, ux, uy);
    const float px = level_position(x, ux, W, kx, align_sample), py = level_position(y, uy, H, ky, align_sample);
    const LevelCorners k = level_corners(px, py, W, H, ssh);
    const float wnw = k.bx * k.by, wne = k.ax * k.by, wsw = k.bx * k.ay, wse = k.ax * k.ay;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const st_t<S> *p = sb + c * ssc;
        const float nw = widen_f32<S>(p[k.r0 + k.cx0]), ne = widen_f32<S>(p[k.r0 + k.cx1]);
        const float sw = widen_f32<S>(p[k.r1 + k.cx0]), se = widen_f32<S>(p[k.r1 + k.cx1]);
        float v = 0.0f;
        v += k.inx0 && k.iny0 ? nw * wnw : 0.0f;
        v += k.inx1 && k.iny0 ? ne * wne : 0.0f;
        v += k.inx0 && k.iny1 ? sw * wsw : 0.0f;
        v += k.inx1 && k.iny1 ? se * wse : 0.0f;
        warped[c] = v;
    }
}

}  // namespace memc
