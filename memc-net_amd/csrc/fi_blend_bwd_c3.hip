// fi_blend_bwd_c3.hip -- the backward of ONE direction of the dual warp + occlusion blend
//     out = occ0 * FI(frame0, flow0, taps0) + occ1 * FI(frame2, flow1, taps1)
// for callers that do not want the image gradient (the frames are data: networks/MEMC_Net_star.py:266-277), RGB, fs == 4,
// fp32, for gfx950: the kernel and the C ABI of libmemc_hip_blend_grad.so (include/memc_warp_blend_grad.h).
//
// fi_blend_bwd_c3 is fi_bwd_c3_pk<false, 256, 2> (fi_bwd_c3.hip, fi_bwd_c3_body.inc with PART == 2: no packed planes, the
// staged image and phase 1 only) with the occlusion folded in.  Per tap k of a site that kernel forms
//     s_k = sum_c gout_c * pix_c(k),   t_k = w_k * s_k            (t_k: the warp's tap gradient)
// and the gradients are linear in gradoutput, so on the RAW gradoutput
//     grad_taps[k] = occ * t_k,   grad_flow = occ * (gx, gy),   grad_occ = sum_k tap_k * t_k  (= sum_c gout_c * warped_c).
// A site whose target lies outside the image: zero tap and flow gradients, grad_occ = sum_c gout_c * in_c (the forward
// copies the input pixel there).
// Over PART 2: one more input plane (occ), one more output plane, two more f32x4 per lane, no atomics.  What the host
// composition around the warp's entry points did per direction -- a forward warp written and read back, gout * warped
// summed over the channels, gout * occ written, a zero-filled image gradient, the whole backward -- is this one pass.
// Same tile machinery and geometry as the PART 2 path (64 x 16 sites per workgroup, 3072 staged pixel quads, kMaxBands
// bands): tests/_lowp_paths.py::census describes this kernel's in-kernel paths too.
// Every element of the three outputs is assigned; the results are a pure function of the inputs.
// The kernel's body (fi_blend_bwd_c3_body.inc) and its three per-site paths (memc_fi_blend_bwd_c3.hpp) are written over the
// storage of the tensors: mx_fi_blend_bwd_c3.hip runs them on half taps and occlusions, lp_fi_blend_bwd_c3.hip on a half
// image as well; here every tag is F32.
#include "memc_common.hpp"
#include "memc_fi_blend_bwd_c3.hpp"
#include "memc_fi_abi.hpp"
#include "memc_warp_blend_grad.h"

namespace memc {

thread_local const char *t_blend_grad_path = "";

// One 64 x NT / 16 tile of sites per workgroup, one direction per launch; 48 KiB of LDS: the staged image (3072 pixel
// quads) and the box words.  Serial chain of a tile: load -> box -> stage -> phase 1: two barriers.  W % 4 == 0, W >= 8.
template <int NT = 256>
__global__ __launch_bounds__(NT, 2) void fi_blend_bwd_c3(
    int W, int H, int tiles_x, int tiles_y, int batch,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    int64_t s4b, int s4h,
    const float *__restrict__ in1, const float *__restrict__ flow, const float *__restrict__ filt,
    const float *__restrict__ occ, const float *__restrict__ gout, float *__restrict__ gflow,
    float *__restrict__ gfilt, float *__restrict__ gocc)
{
    using I = F32;
    using T = F32;
    using FT = F32;
    using GT = F32;
#include "fi_blend_bwd_c3_body.inc"
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_blend_grad.h)
// ==================================================================================================
using namespace memc;

extern "C" {

const char *memc_blend_grad_version(void) { return "memc_hip_blend_grad 0.1 gfx950"; }

const char *memc_blend_grad_last_kernel_path(void) { return memc::t_blend_grad_path; }

int FilterInterpolationBlendLayer_gpu_backward(memc_stream_t stream, const memc_tensor4 *input, const memc_tensor4 *flow,
                                               const memc_tensor4 *filter, const memc_tensor4 *occlusion,
                                               const memc_tensor4 *gradoutput, const memc_tensor4 *gradflow,
                                               const memc_tensor4 *gradfilter, const memc_tensor4 *gradocclusion)
{
    const FiChecked q = fi_blend_bwd_checked(fi_filter_side_exact, input, flow, filter, occlusion, gradoutput, gradflow,
                                             gradfilter, gradocclusion);
    if (q.done) return q.code;
    // coverage: the tiled RGB kernel; anything else is the caller's composition of the warp's entry points
    if (!(fi_rgb_tiled_shape(q.c, q.fs, q.w) &&
          plane_fits_u32(q.w, q.h, {(long)input->stride[2], (long)flow->stride[2], (long)filter->stride[2],
                                    (long)occlusion->stride[2]})))
        return kNotCovered;
    constexpr int NT = 256;                    // one 64 x NT / 16 tile of sites per workgroup
    t_blend_grad_path = "fi_blend_bwd:tiled_c3";
    fi_blend_bwd_tiled_launch<TileGeom<16, 3072, NT>>(
        fi_blend_bwd_c3<NT>, PkGeomT<NT>::kLds,
        fi_blend_bwd_call<F32, F32, F32>((hipStream_t)stream, q, input, flow, filter, occlusion, gradoutput, gradflow,
                                         gradfilter, gradocclusion));
    return launch_status();
}

}  // extern "C"
