// lp_fi_bwd_c3.hip -- the RGB adaptive-warp (FilterInterpolation) backward on fp16 / bf16 storage, for gfx950: the kernel
// and the C ABI of libmemc_hip_lp_grad.so (include/memc_warp_lp_grad.h).
//
// fi_bwd_c3_lp IS the fp32 kernel fi_bwd_c3_pk (fi_bwd_c3.hip): the same body (fi_bwd_c3_body.inc) on half image, taps
// and tap gradient, with fp32 or half flow / flow gradient and gradoutput (memc_lp.hpp).  Loads widen exactly, the LDS
// image and the packed image-gradient planes are fp32, every stored gradient is rounded once; the image gradient stays
// an fp32 buffer that the tiles' flushes add into.  Per site at 720p (fp32 flow, no image gradient): image 6 (staged) +
// flow 8 + taps 32 + gradoutput 6 read, tap gradient 32 + flow gradient 8 written -- about 92 B against the fp32
// kernel's 168 B, and none of the widening / narrowing copies the host path around the fp32 kernel needs.
// PART 0 (gradinput1 given) and PART 2 (gradinput1 == NULL) are chosen exactly as the fp32 launcher chooses them: the two
// sum gradinput2 of sites that no LDS band covers in different orders (fi_bwd_site_scalar vs fi_bwd_site_taps).
#include "memc_common.hpp"
#include "memc_fi_bwd_c3.hpp"
#include "memc_fi_abi.hpp"
#include "memc_warp_lp_grad.h"

namespace memc {

thread_local const char *t_lp_grad_path = "";

// P: image / taps / tap gradient; FT: flow / flow gradient; GT: gradoutput.  Two workgroups of 256 lanes per CU, as the
// fp32 PART 0 / PART 2 kernels.
template <class P, class FT, class GT, int PART>
__global__ __launch_bounds__(256, 2) void fi_bwd_c3_lp(
    int W, int H, int tiles_x, int tiles_y, int batch,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    const st_t<P> *__restrict__ in1, const st_t<FT> *__restrict__ flow, const st_t<P> *__restrict__ filt,
    const st_t<GT> *__restrict__ gout, float *__restrict__ gin1, st_t<FT> *__restrict__ gin2,
    st_t<P> *__restrict__ gin3)
{
    using I = P;                               // the image is stored as the taps are
    constexpr bool TR = false;                 // (timestamps: the fp32 measurement build only)
    constexpr int NT = 256;
    constexpr bool RAG = false;                // widths that are a multiple of four
#include "fi_bwd_c3_body.inc"
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_lp_grad.h)
// ==================================================================================================
using namespace memc;

extern "C" {

const char *memc_lp_grad_version(void) { return "memc_hip_lp_grad 0.1 gfx950"; }

const char *memc_lp_grad_last_kernel_path(void) { return memc::t_lp_grad_path; }

int FilterInterpolationLayer_gpu_backward_lp(memc_stream_t stream, memc_dtype payload, memc_dtype flowt, memc_dtype goutt,
                                             const memc_tensor4 *input1, const memc_tensor4 *input2,
                                             const memc_tensor4 *input3, const memc_tensor4 *gradoutput,
                                             const memc_tensor4 *gradinput1, const memc_tensor4 *gradinput2,
                                             const memc_tensor4 *gradinput3)
{
    if (!dtypes_ok(payload, flowt) || !dtypes_ok(payload, goutt)) return kErr;
    const FiChecked q = fi_bwd_checked(fi_filter_side_exact, input1, input2, input3, gradoutput, gradinput1, gradinput2,
                                       gradinput3);
    if (q.done) return q.code;
    // coverage: the tiled RGB kernel on 8-byte half quads; anything else is the caller's (widened) business
    bool covered = fi_rgb_tiled_shape(q.c, q.fs, q.w) &&
                   plane_fits_u32(q.w, q.h, {(long)input1->stride[2], (long)input2->stride[2], (long)input3->stride[2]});
    for (const memc_tensor4 *t : {input1, input3, gradinput3}) covered = covered && quad_ok(t);
    if (flowt == payload) covered = covered && quad_ok(input2) && quad_ok(gradinput2);
    if (goutt == payload) covered = covered && quad_ok(gradoutput);
    if (!covered) return kNotCovered;
    // the eight (payload, flow, gradoutput) instantiations
    return fi_dispatch(payload, flowt, goutt, [&](auto p, auto ft, auto gt) {
        using P = decltype(p);
        using FT = decltype(ft);
        using GT = decltype(gt);
        return fi_bwd_launch(fi_bwd_call<P, FT, GT>((hipStream_t)stream, q, input1, input2, input3, gradoutput, gradinput1,
                                                    gradinput2, gradinput3),
                             t_lp_grad_path, "fi_bwd_lp:tiled_c3", "fi_bwd_lp:tiled_c3_noimage",
                             [](const auto &k, auto part) {
                                 fi_bwd_tiled_launch<TileGeom<16>>(fi_bwd_c3_lp<P, FT, GT, decltype(part)::value>,
                                                                   PkGeom::kLds, k);
                             });
    });
}

}  // extern "C"
