// lp_fi_blend_bwd_c3.hip -- the backward of ONE direction of the dual warp + occlusion blend on fp16 / bf16 storage, for
// gfx950: a half image, half taps and occlusion, a flow and a gradoutput in fp32 or that type, for callers that do not
// want the image gradient.  The kernel and the C ABI of libmemc_hip_lp_blend_grad.so (include/memc_warp_lp_blend_grad.h).
//
// This is the blend's backward of a model cast to bf16 / fp16 (lp_filter_interpolation.hip's blend is its forward).
// Read as they are the tensors of one direction are about 96 B per site (fp32 flow, half gradoutput: image 6 staged +
// flow 8 + taps 32 + occlusion 2 + gradoutput 6 read, tap gradient 32 + flow gradient 8 + occlusion gradient 2 written;
// 88 B with a half flow).
//
// fi_blend_bwd_c3_lp IS the fp32 kernel fi_blend_bwd_c3<256> (fi_blend_bwd_c3.hip): the same body
// (fi_blend_bwd_c3_body.inc) and the same three per-site paths (memc_fi_blend_bwd_c3.hpp), the image staged from half
// quads into the fp32 LDS tile as fi_bwd_c3_lp stages it (lp_fi_bwd_c3.hip); loads widen exactly, every stored gradient is
// rounded once.  So each output equals, bit for bit, the fp32 library's on the widened inputs after one `.to(dtype)`.
// No atomics, no image gradient, no workspace; every element of the three outputs is assigned.
#include "memc_common.hpp"
#include "memc_fi_blend_bwd_c3.hpp"
#include "memc_fi_abi.hpp"
#include "memc_warp_lp_blend_grad.h"

namespace memc {

thread_local const char *t_lp_blend_grad_path = "";

// T: image, taps, occlusion, tap and occlusion gradients; FT: flow / flow gradient; GT: gradoutput.  Two workgroups of 256
// lanes per CU, as the fp32 kernel.
template <class T, class FT, class GT>
__global__ __launch_bounds__(256, 2) void fi_blend_bwd_c3_lp(
    int W, int H, int tiles_x, int tiles_y, int batch,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    int64_t s4b, int s4h,
    const st_t<T> *__restrict__ in1, const st_t<FT> *__restrict__ flow, const st_t<T> *__restrict__ filt,
    const st_t<T> *__restrict__ occ, const st_t<GT> *__restrict__ gout, st_t<FT> *__restrict__ gflow,
    st_t<T> *__restrict__ gfilt, st_t<T> *__restrict__ gocc)
{
    using I = T;                               // the image is stored as the taps are
    constexpr int NT = 256;
#include "fi_blend_bwd_c3_body.inc"
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_lp_blend_grad.h)
// ==================================================================================================
using namespace memc;

extern "C" {

const char *memc_lp_blend_grad_version(void) { return "memc_hip_lp_blend_grad 0.1 gfx950"; }

const char *memc_lp_blend_grad_last_kernel_path(void) { return memc::t_lp_blend_grad_path; }

int FilterInterpolationBlendLayer_gpu_backward_lp(memc_stream_t stream, memc_dtype payload, memc_dtype flowt,
                                                  memc_dtype goutt, const memc_tensor4 *input, const memc_tensor4 *flow,
                                                  const memc_tensor4 *filter, const memc_tensor4 *occlusion,
                                                  const memc_tensor4 *gradoutput, const memc_tensor4 *gradflow,
                                                  const memc_tensor4 *gradfilter, const memc_tensor4 *gradocclusion)
{
    if (!dtypes_ok(payload, flowt) || !dtypes_ok(payload, goutt)) return kErr;
    const FiChecked q = fi_blend_bwd_checked(fi_filter_side_exact, input, flow, filter, occlusion, gradoutput, gradflow,
                                             gradfilter, gradocclusion);
    if (q.done) return q.code;
    // coverage: the tiled RGB kernel, every tensor aligned for its storage; anything else is the caller's (composed) business
    if (!(fi_rgb_tiled_shape(q.c, q.fs, q.w) &&
          plane_fits_u32(q.w, q.h, {(long)input->stride[2], (long)flow->stride[2], (long)filter->stride[2],
                                    (long)occlusion->stride[2]}) &&
          storage_ok(payload, {input, filter, occlusion, gradfilter, gradocclusion}) &&
          storage_ok(flowt, {flow, gradflow}) && storage_ok(goutt, {gradoutput})))
        return kNotCovered;
    // the eight (payload, flow, gradoutput) instantiations
    return fi_dispatch(payload, flowt, goutt, [&](auto t, auto ft, auto gt) {
        using T = decltype(t);
        using FT = decltype(ft);
        using GT = decltype(gt);
        t_lp_blend_grad_path = "fi_blend_bwd_lp:tiled_c3";
        fi_blend_bwd_tiled_launch<TileGeom<16>>(
            fi_blend_bwd_c3_lp<T, FT, GT>, PkGeom::kLds,
            fi_blend_bwd_call<T, FT, GT>((hipStream_t)stream, q, input, flow, filter, occlusion, gradoutput, gradflow,
                                         gradfilter, gradocclusion));
        return launch_status();
    });
}

}  // extern "C"
