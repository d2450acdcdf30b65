// memc_lp_fi.hpp -- what the tiled forward kernels on half-width taps share beside their bodies (lp_fi_fwd_body.inc,
// lp_fi_blend_body.inc): lp_filter_interpolation.hip (libmemc_hip_lp.so) and mx_filter_interpolation.hip (libmemc_hip_mx.so).
#pragma once

#include "memc_common.hpp"
#include "memc_tile.hpp"
#include "memc_fi.hpp"
#include "memc_lp.hpp"

namespace memc {

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

}  // namespace memc
