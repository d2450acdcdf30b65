// mx_fi_bwd_c3.hip -- the RGB adaptive-warp (FilterInterpolation) backward on MIXED storage, for gfx950: an fp32 image and
// an fp32 gradoutput beside fp16 / bf16 taps and a flow in fp32 or that type.  The kernel and the C ABI of
// libmemc_hip_mx_grad.so (include/memc_warp_mx_grad.h).
//
// This is the backward of the call torch.autocast makes (mx_filter_interpolation.hip is its forward): the frames are the
// network's input and stay fp32, so does the gradient of the fp32 output; the U-Net heads' taps are half.  Promoted to
// fp32 on the host such a call moves about 360 B per site (fp32 flow, no image gradient: 96 to widen the taps, the fp32
// kernel's 168, 96 to narrow the tap gradient); read as they are the tensors are 104 B (image 12 staged + flow 8 + taps 32
// + gradoutput 12 read, tap gradient 32 + flow gradient 8 written).
//
// fi_bwd_c3_mx IS the fp32 kernel fi_bwd_c3_pk (fi_bwd_c3.hip): the same body (fi_bwd_c3_body.inc) with the image staged
// as the fp32 kernel stages it (dword-aligned fp32 quads, memc_tile.hpp) and the taps, the tap gradient and -- where it is
// half -- the flow and its gradient handled as the half kernel fi_bwd_c3_lp handles them (lp_fi_bwd_c3.hip): loads widen
// exactly, every stored gradient is rounded once.  PART 0 (gradinput1 given) and PART 2 (gradinput1 == NULL) are chosen
// exactly as the fp32 launcher chooses them.
#include "memc_common.hpp"
#include "memc_fi_bwd_c3.hpp"
#include "memc_fi_abi.hpp"
#include "memc_warp_mx_grad.h"

namespace memc {

thread_local const char *t_mx_grad_path = "";

// T: taps / tap gradient; FT: flow / flow gradient.  Two workgroups of 256 lanes per CU, as the fp32 and half kernels.
template <class T, class FT, int PART>
__global__ __launch_bounds__(256, 2) void fi_bwd_c3_mx(
    int W, int H, int tiles_x, int tiles_y, int batch,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    const float *__restrict__ in1, const st_t<FT> *__restrict__ flow, const st_t<T> *__restrict__ filt,
    const float *__restrict__ gout, float *__restrict__ gin1, st_t<FT> *__restrict__ gin2,
    st_t<T> *__restrict__ gin3)
{
    using P = T;
    using I = F32;                             // the image
    using GT = F32;                            // gradoutput: the gradient of a mixed forward's fp32 output
    constexpr bool TR = false;                 // (timestamps: the fp32 measurement build only)
    constexpr int NT = 256;
    constexpr bool RAG = false;                // widths that are a multiple of four
#include "fi_bwd_c3_body.inc"
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_mx_grad.h)
// ==================================================================================================
using namespace memc;

extern "C" {

const char *memc_mx_grad_version(void) { return "memc_hip_mx_grad 0.1 gfx950"; }

const char *memc_mx_grad_last_kernel_path(void) { return memc::t_mx_grad_path; }

int FilterInterpolationLayer_gpu_backward_mx(memc_stream_t stream, memc_dtype tapt, memc_dtype flowt,
                                             const memc_tensor4 *input1, const memc_tensor4 *input2,
                                             const memc_tensor4 *input3, const memc_tensor4 *gradoutput,
                                             const memc_tensor4 *gradinput1, const memc_tensor4 *gradinput2,
                                             const memc_tensor4 *gradinput3)
{
    if (!dtypes_ok(tapt, flowt)) return kErr;
    const FiChecked q = fi_bwd_checked(fi_filter_side_exact, input1, input2, input3, gradoutput, gradinput1, gradinput2,
                                       gradinput3);
    if (q.done) return q.code;
    // coverage: the tiled RGB kernel, every tensor aligned for its storage; anything else is the caller's (promoted) business
    if (!(fi_rgb_tiled_shape(q.c, q.fs, q.w) &&
          plane_fits_u32(q.w, q.h, {(long)input1->stride[2], (long)input2->stride[2], (long)input3->stride[2]}) &&
          storage_ok(tapt, {input3, gradinput3}) && storage_ok(MEMC_F32, {input1, gradoutput, gradinput1}) &&
          storage_ok(flowt, {input2, gradinput2})))
        return kNotCovered;
    return fi_dispatch(tapt, flowt, [&](auto t, auto ft) {
        using T = decltype(t);
        using FT = decltype(ft);
        return fi_bwd_launch(fi_bwd_call<T, FT, F32, F32>((hipStream_t)stream, q, input1, input2, input3, gradoutput,
                                                          gradinput1, gradinput2, gradinput3),
                             t_mx_grad_path, "fi_bwd_mx:tiled_c3", "fi_bwd_mx:tiled_c3_noimage",
                             [](const auto &k, auto part) {
                                 fi_bwd_tiled_launch<TileGeom<16>>(fi_bwd_c3_mx<T, FT, decltype(part)::value>,
                                                                   PkGeom::kLds, k);
                             });
    });
}

}  // extern "C"
