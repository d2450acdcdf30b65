// mx_fi_blend_bwd_c3.hip -- the backward of ONE direction of the dual warp + occlusion blend on MIXED storage, for gfx950:
// an fp32 image and an fp32 gradoutput beside fp16 / bf16 taps and occlusion and a flow in fp32 or that type, for callers
// that do not want the image gradient.  The kernel and the C ABI of libmemc_hip_mx_blend_grad.so
// (include/memc_warp_mx_blend_grad.h).
//
// This is the blend's backward of the call torch.autocast makes (mx_filter_interpolation.hip's fi_blend_mx_tiled is its
// forward).  Promoted to fp32 on the host one direction moves about 380 B per site (fp32 flow: 96 + 6 to widen the taps and
// the occlusion, the fp32 kernel's 176, 96 + 6 to narrow the two gradients); read as they are the tensors are 108 B (image
// 12 staged + flow 8 + taps 32 + occlusion 2 + gradoutput 12 read, tap gradient 32 + flow gradient 8 + occlusion gradient 2
// written).
//
// fi_blend_bwd_c3_mx IS the fp32 kernel fi_blend_bwd_c3<256> (fi_blend_bwd_c3.hip): the same body
// (fi_blend_bwd_c3_body.inc) and the same three per-site paths (memc_fi_blend_bwd_c3.hpp), the image staged as the fp32
// kernel stages it; loads of the half tensors widen exactly, every stored gradient is rounded once.  So each output equals,
// bit for bit, the fp32 library's on the widened inputs after one `.to(dtype)`.
#include "memc_common.hpp"
#include "memc_fi_blend_bwd_c3.hpp"
#include "memc_fi_abi.hpp"
#include "memc_warp_mx_blend_grad.h"

namespace memc {

thread_local const char *t_mx_blend_grad_path = "";

// T: taps, occlusion and their gradients; FT: flow / flow gradient.  Two workgroups of 256 lanes per CU, as the fp32 kernel.
template <class T, class FT>
__global__ __launch_bounds__(256, 2) void fi_blend_bwd_c3_mx(
    int W, int H, int tiles_x, int tiles_y, int batch,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    int64_t s4b, int s4h,
    const float *__restrict__ in1, const st_t<FT> *__restrict__ flow, const st_t<T> *__restrict__ filt,
    const st_t<T> *__restrict__ occ, const float *__restrict__ gout, st_t<FT> *__restrict__ gflow,
    st_t<T> *__restrict__ gfilt, st_t<T> *__restrict__ gocc)
{
    using I = F32;                             // the image and gradoutput are fp32
    using GT = F32;
    constexpr int NT = 256;
#include "fi_blend_bwd_c3_body.inc"
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_mx_blend_grad.h)
// ==================================================================================================
using namespace memc;

extern "C" {

const char *memc_mx_blend_grad_version(void) { return "memc_hip_mx_blend_grad 0.1 gfx950"; }

const char *memc_mx_blend_grad_last_kernel_path(void) { return memc::t_mx_blend_grad_path; }

int FilterInterpolationBlendLayer_gpu_backward_mx(memc_stream_t stream, memc_dtype tapt, memc_dtype flowt,
                                                  const memc_tensor4 *input, const memc_tensor4 *flow,
                                                  const memc_tensor4 *filter, const memc_tensor4 *occlusion,
                                                  const memc_tensor4 *gradoutput, const memc_tensor4 *gradflow,
                                                  const memc_tensor4 *gradfilter, const memc_tensor4 *gradocclusion)
{
    if (!dtypes_ok(tapt, flowt)) return kErr;
    const FiChecked q = fi_blend_bwd_checked(fi_filter_side_exact, input, flow, filter, occlusion, gradoutput, gradflow,
                                             gradfilter, gradocclusion);
    if (q.done) return q.code;
    // coverage: the tiled RGB kernel, every tensor aligned for its storage; anything else is the caller's (promoted) business
    if (!(fi_rgb_tiled_shape(q.c, q.fs, q.w) &&
          plane_fits_u32(q.w, q.h, {(long)input->stride[2], (long)flow->stride[2], (long)filter->stride[2],
                                    (long)occlusion->stride[2]}) &&
          storage_ok(tapt, {filter, occlusion, gradfilter, gradocclusion}) && storage_ok(MEMC_F32, {input, gradoutput}) &&
          storage_ok(flowt, {flow, gradflow})))
        return kNotCovered;
    return fi_dispatch(tapt, flowt, [&](auto t, auto ft) {
        using T = decltype(t);
        using FT = decltype(ft);
        t_mx_blend_grad_path = "fi_blend_bwd_mx:tiled_c3";
        fi_blend_bwd_tiled_launch<TileGeom<16>>(
            fi_blend_bwd_c3_mx<T, FT>, PkGeom::kLds,
            fi_blend_bwd_call<T, FT, F32, F32>((hipStream_t)stream, q, input, flow, filter, occlusion, gradoutput, gradflow,
                                               gradfilter, gradocclusion));
        return launch_status();
    });
}

}  // extern "C"
