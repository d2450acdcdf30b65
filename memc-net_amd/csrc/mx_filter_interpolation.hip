// mx_filter_interpolation.hip -- the RGB adaptive warp (FilterInterpolation) forward and the fused dual warp + occlusion
// blend on MIXED storage, for gfx950: an fp32 image and an fp32 output beside fp16 / bf16 taps and occlusions and a flow in
// fp32 or that type.  The kernels and the C ABI of libmemc_hip_mx.so (include/memc_warp_mx.h).
//
// This is what torch.autocast hands the operators: the frames are the network's input and stay fp32, the U-Net heads
// return half taps and occlusions.  Promoted to fp32 on the host, such a call moves 416 B per site (blend, half flows:
// 228 B of casts + the fp32 kernel's 188) or 204 B (warp); read as they are it moves 112 B (images 24 + flows 8 + taps 64 +
// occlusions 4 + output 12) or 60 B (12 + 4 + 32 + 12).
//
// The kernels are libmemc_hip_lp.so's tiled RGB kernels (lp_fi_fwd_body.inc, lp_fi_blend_body.inc: one definition) with
// the image's storage set to
// F32: staged with memc_tile.hpp's dword-aligned fp32 quads, the invalid-site copy and the per-site path read fp32 pixels,
// the output is stored as computed.  fs == 4 and C == 3 only; anything else is declined (return 1).
#include "memc_common.hpp"
#include "memc_tile.hpp"
#include "memc_fi.hpp"
#include "memc_lp.hpp"
#include "memc_lp_fi.hpp"
#include "memc_fi_abi.hpp"
#include "memc_warp_mx.h"

namespace memc {

thread_local const char *t_mx_path = "";

template <class T, class FT>
__global__ __launch_bounds__(256, 2) void fi_fwd_mx_tiled(
    int W, int H, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    const float *__restrict__ in1, const st_t<FT> *__restrict__ flow, const st_t<T> *__restrict__ filt,
    float *__restrict__ out)
{
    using I = F32;                             // the image and the output
    constexpr bool RGB = true, RAGGED = false;
    constexpr int C = 3;
#include "lp_fi_fwd_body.inc"
}

template <class T, class FT>
__global__ __launch_bounds__(256, 2) void fi_blend_mx_tiled(
    int W, int H, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    int64_t sob, int soh,
    const float *__restrict__ in0, const float *__restrict__ in2, const st_t<FT> *__restrict__ flow0,
    const st_t<FT> *__restrict__ flow1, const st_t<T> *__restrict__ filt0, const st_t<T> *__restrict__ filt1,
    const st_t<T> *__restrict__ occ0, const st_t<T> *__restrict__ occ1, float *__restrict__ out)
{
    using I = F32;
#include "lp_fi_blend_body.inc"
}

// The tiles cover the width's quads: 64 x 16 sites each.
template <class T, class FT>
void launch_fi_fwd_mx_tiled(const FiFwdCall<st_t<T>, st_t<FT>, float> &k)
{
    const TileGrid g = fi_tile_grid<TileGeom<16>>(k.w, k.h);
    hipLaunchKernelGGL((fi_fwd_mx_tiled<T, FT>), dim3((unsigned)g.ntx * g.nty * k.batch), dim3(256), tile_lds_bytes<16>(),
                       k.stream, k.w, k.h, g.ntx, g.nty, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c, k.s2.h, k.s3.b, k.s3.c,
                       k.s3.h, k.in1, k.flow, k.filt, k.out);
}

template <class T, class FT>
void launch_fi_blend_mx_tiled(const FiBlendFwdCall<st_t<T>, st_t<FT>, float> &k)
{
    const TileGrid g = fi_tile_grid<TileGeom<16>>(k.w, k.h);
    hipLaunchKernelGGL((fi_blend_mx_tiled<T, FT>), dim3((unsigned)g.ntx * g.nty * k.batch), dim3(256), tile_lds_bytes<16>(),
                       k.stream, k.w, k.h, g.ntx, g.nty, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c, k.s2.h, k.s3.b, k.s3.c,
                       k.s3.h, k.so.b, k.so.h, k.in0, k.in2, k.flow0, k.flow1, k.filt0, k.filt1, k.occ0, k.occ1, k.out);
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_mx.h)
// ==================================================================================================
namespace {

using namespace memc;

// fp32 tensors need dword alignment only (f32x4u); a T tensor -- the taps, the occlusions, a flow in T -- 8-byte quads
inline bool flow_quad_ok(memc_dtype flowt, const memc_tensor4 *flow) { return flowt == MEMC_F32 || quad_ok(flow); }

}  // namespace

extern "C" {

const char *memc_mx_version(void) { return "memc_hip_mx 0.1 gfx950"; }

const char *memc_mx_last_kernel_path(void) { return memc::t_mx_path; }

int FilterInterpolationLayer_gpu_forward_mx(memc_stream_t stream, memc_dtype tapt, memc_dtype flowt,
                                            const memc_tensor4 *input1, const memc_tensor4 *input2,
                                            const memc_tensor4 *input3, const memc_tensor4 *output)
{
    if (!dtypes_ok(tapt, flowt)) return kErr;
    if (!ok(input1) || !ok(input2) || !ok(input3) || !ok(output)) return kErr;
    if (!flow_matches(input1, input2) || !taps_match(input1, input3)) return kErr;
    const int fs = fi_filter_side_exact(input3->size[1]);
    if (fs < 1) return kErr;
    if (!same_layout(input1, output)) return kErr;
    const FiChecked q = fi_sizes(fs, input1);
    if (q.done) return q.code;
    // coverage: the tiled RGB kernel; anything else is the caller's (promoted) business
    if (!(fi_rgb_tiled_shape(q.c, fs, q.w) &&
          plane_fits_u32(q.w, q.h, {(long)input1->stride[2], (long)input2->stride[2], (long)input3->stride[2]}) &&
          quad_ok(input3) && flow_quad_ok(flowt, input2)))
        return kNotCovered;
    return fi_dispatch(tapt, flowt, [&](auto t, auto ft) {
        t_mx_path = "fi_fwd_mx:tiled_c3";
        launch_fi_fwd_mx_tiled<decltype(t), decltype(ft)>(
            fi_fwd_call<decltype(t), decltype(ft), F32>((hipStream_t)stream, q, input1, input2, input3, output));
        return launch_status();
    });
}

int FilterInterpolationBlendLayer_gpu_forward_mx(memc_stream_t stream, memc_dtype tapt, memc_dtype flowt,
                                                 const memc_tensor4 *input0, const memc_tensor4 *input2,
                                                 const memc_tensor4 *flow0, const memc_tensor4 *flow1,
                                                 const memc_tensor4 *filter0, const memc_tensor4 *filter1,
                                                 const memc_tensor4 *occlusion0, const memc_tensor4 *occlusion1,
                                                 const memc_tensor4 *output)
{
    if (!dtypes_ok(tapt, flowt)) return kErr;
    const memc_tensor4 *const all[9] = {input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1, output};
    const FiChecked q = fi_blend_fwd_checked(fi_filter_side_exact, all);
    if (q.done) return q.code;
    bool covered = fi_rgb_tiled_shape(q.c, q.fs, q.w) &&
                   plane_fits_u32(q.w, q.h, {(long)input0->stride[2], (long)flow0->stride[2], (long)filter0->stride[2],
                                             (long)occlusion0->stride[2]});
    for (const memc_tensor4 *t : {filter0, filter1, occlusion0, occlusion1}) covered = covered && quad_ok(t);
    covered = covered && flow_quad_ok(flowt, flow0) && flow_quad_ok(flowt, flow1);
    if (!covered) return kNotCovered;
    return fi_dispatch(tapt, flowt, [&](auto t, auto ft) {
        t_mx_path = "fi_blend_mx:tiled_c3";
        launch_fi_blend_mx_tiled<decltype(t), decltype(ft)>(
            fi_blend_fwd_call<decltype(t), decltype(ft), F32>((hipStream_t)stream, q, all));
        return launch_status();
    });
}

}  // extern "C"
