// fi_bwd_c3.hip -- FilterInterpolation backward, RGB (C == 3), fs == 4: the LDS-tiled kernel.
//
// Replaces my_package/src/my_lib_kernel.cu:1220-1518 (kernel) / :1571-1627 (launcher) of the reference for the only
// channel count its networks back-propagate through (networks/MEMC_Net_star.py:266-277; the context warps are
// detached, :285).  Semantics: SURVEY.md appendix A.2.  Same tile / box machinery as the forward kernel:
//   * streams (flow, 16 tap planes, 3 gradoutput planes) as dwordx4;
//   * the image gradient -- 48 scattered adds per site -- is accumulated in LDS (packed fixed point, below) and
//     flushed once per cell with row-coalesced global atomics (neighbouring tiles' boxes overlap);
//   * the image box is staged into LDS pixel quads for the tap and flow gradients: gradinput3 (each site owns its
//     taps) is stored once per site as dwordx4, gradinput2 is assigned;
//   * sites whose window no band covers are redone by fi_bwd_site_scalar with global atomics.
// The packed planes are described in memc_pk.hpp.  The kernel of rounds 1-2 (one fp64 plane per colour) lives on as a
// measurement arm: arms/fi_bwd_c3_arms.hip.  The kernel's body and its per-site helpers live in memc_fi_bwd_c3.hpp, written
// over the tensors' storage: this file instantiates them for fp32, lp_fi_bwd_c3.hip for fp16 / bf16, mx_fi_bwd_c3.hip for an
// fp32 image beside half taps (those two launch through memc_fi_abi.hpp's fi_bwd_tiled_launch; launch_fi_bwd_c3_pk below
// covers the whole quads of a ragged width, w & ~3, and serves the measurement arms, so it keeps its own grid).
#include "memc_common.hpp"
#include "memc_internal.h"
#include "memc_fi_bwd_c3.hpp"

namespace memc {

// RAG: a ragged width (W % 4 != 0, round 5) -- the whole quads here (sites x < W & ~3; the image's true width in every clamp,
// validity test and box, the box's last quad staged ragged-safely: memc_tile.hpp), the one to three columns behind them in
// fi_bwd_direct_fs4 (launcher); both ADD into gradinput1.  One workgroup per CU: the kernel has no registers left for it.
template <bool TR, int NT = 256, int PART = 0, bool RAG = false>
__global__ __launch_bounds__(NT, RAG ? 1 : (PART == 0 || !kPartThree ? 2 : 3)) void fi_bwd_c3_pk(
    int W, int H, int tiles_x, int tiles_y, int batch,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    const float *__restrict__ in1, const float *__restrict__ flow, const float *__restrict__ filt,
    const float *__restrict__ gout, float *__restrict__ gin1, float *__restrict__ gin2,
    float *__restrict__ gin3)
{
    using P = F32;                             // storage of the taps, the image, the flow, gradoutput (memc_lp.hpp)
    using I = P;
    using FT = F32;
    using GT = F32;
#include "fi_bwd_c3_body.inc"
}

// The tiles cover the whole quads (sites x < w & ~3): 64 x NT / 16 sites each.
template <bool TR, int NT = 256, int PART = 0, bool RAG = false>
static void launch_fi_bwd_c3_pk(const FiBwdCall<> &k)
{
    using G = TileGeom<16, 3072, NT>;
    const int ntx = ((k.w & ~3) + G::kTW - 1) / G::kTW, nty = (k.h + G::kTH - 1) / G::kTH;
    hipLaunchKernelGGL((fi_bwd_c3_pk<TR, NT, PART, RAG>), dim3((unsigned)ntx * nty * k.batch), dim3(NT), PkGeomT<NT>::kLds,
                       k.stream, k.w, k.h, ntx, nty, k.batch, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c, k.s2.h, k.s3.b,
                       k.s3.c, k.s3.h, k.in1, k.flow, k.filt, k.gout, k.gin1, k.gin2, k.gin3);
}

// 1: taken; 2: taken for the whole quads of a ragged width (w % 4 != 0): the caller runs the direct kernel on the columns
// from w & ~3 on; 0: not taken (the caller takes the direct kernel for everything); -1: launch error.  `variant` >= 0
// selects a measurement arm (measurement build only; the product passes -1).
int fi_bwd_c3_launch(const FiBwdCall<> &k, int variant)
{
    const int w = k.w, ws = w & ~3;
    if (!plane_fits_u32(w, k.h, {k.s1.h, k.s2.h, k.s3.h}) || ws < 4) return 0;
    if (ws < w && (k.gin1 == nullptr || variant >= 0)) return 0;   // (the tail's direct kernel needs the buffer; arms: whole widths)
#ifdef MEMC_MEASURE
    if (variant == 28) {                                   // + timestamps
        launch_fi_bwd_c3_pk<true>(k);
        return launch_status() == 0 ? 1 : -1;
    }
    if (variant == 61) {                                   // A/B arm: 64 x 8 tiles on 128 lanes (LOST, see PkGeomT)
        launch_fi_bwd_c3_pk<false, 128>(k);
        return launch_status() == 0 ? 1 : -1;
    }
    if (variant >= 0 && variant != 60) {                   // arms/fi_bwd_c3_arms.hip (60: this kernel, named)
        const int r = fi_bwd_c3_arm_launch(variant, k);
        if (r != 0) return r;
    }
#endif
    if (k.gin1 == nullptr) {                               // the caller does not want the image gradient
        launch_fi_bwd_c3_pk<false, 256, 2>(k);
#ifdef MEMC_MEASURE
    } else if (variant == 62) {                            // arm: the two halves as two launches (LOST, see the kernel)
        launch_fi_bwd_c3_pk<false, 256, 1>(k);
        launch_fi_bwd_c3_pk<false, 256, 2>(k);
#endif
    } else if (ws < w) {                                   // a ragged width: the RAG instantiation (+ the caller's tail launch)
        launch_fi_bwd_c3_pk<false, 256, 0, true>(k);
    } else {
        launch_fi_bwd_c3_pk<false>(k);
    }
    return launch_status() == 0 ? (ws < w ? 2 : 1) : -1;
}

}  // namespace memc

#ifdef MEMC_MEASURE
// device buffer of gridDim.x * 16 uint64 for the timestamp arms (fi_bwd variants 9 and 28); tools/trace_kernel.py
extern "C" int memc_debug_set_trace_buffer(void *p)
{
    unsigned long long *q = (unsigned long long *)p;
    const int a = hipMemcpyToSymbol(HIP_SYMBOL(memc::g_trace_buf), &q, sizeof(q)) == hipSuccess ? 0 : -1;
    return a == 0 ? memc::fi_bwd_c3_arms_set_trace_buffer(q) : a;
}
#endif
