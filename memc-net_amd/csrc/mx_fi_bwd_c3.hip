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
#include "memc_desc.hpp"
#include "memc_launch.hpp"
#include "memc_warp_mx_grad.h"

#include <math.h>

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
namespace {

using namespace memc;
constexpr int kErr = -1;
constexpr int kNotCovered = 1;

template <class T, class FT>
using MxBwdCall = FiBwdCall<st_t<T>, st_t<FT>, float, float>;

template <class T, class FT, int PART>
void launch_fi_bwd_c3_mx(const MxBwdCall<T, FT> &k)
{
    using G = TileGeom<16>;
    const int ntx = (k.w + G::kTW - 1) / G::kTW, nty = (k.h + G::kTH - 1) / G::kTH;
    hipLaunchKernelGGL((fi_bwd_c3_mx<T, FT, PART>), dim3((unsigned)ntx * nty * k.batch), dim3(256), PkGeom::kLds, k.stream,
                       k.w, k.h, ntx, nty, k.batch, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c, k.s2.h, k.s3.b, k.s3.c, k.s3.h,
                       k.in1, k.flow, k.filt, k.gout, k.gin1, k.gin2, k.gin3);
}

template <class T, class FT>
int fi_bwd_mx_launch(hipStream_t stream, int w, int h, int n, const memc_tensor4 *in1, const memc_tensor4 *flow,
                     const memc_tensor4 *filt, const memc_tensor4 *gout, const memc_tensor4 *gin1, const memc_tensor4 *gin2,
                     const memc_tensor4 *gin3)
{
    const MxBwdCall<T, FT> k = {
        stream, w, h, 3, n, 4, plane(in1), plane(flow), plane(filt),
        reinterpret_cast<const float *>(in1->data), reinterpret_cast<const st_t<FT> *>(flow->data),
        reinterpret_cast<const st_t<T> *>(filt->data), reinterpret_cast<const float *>(gout->data),
        gin1 ? reinterpret_cast<float *>(gin1->data) : nullptr, reinterpret_cast<st_t<FT> *>(gin2->data),
        reinterpret_cast<st_t<T> *>(gin3->data)};
    if (k.gin1) {                              // the whole backward (the fp32 launcher's PART 0)
        t_mx_grad_path = "fi_bwd_mx:tiled_c3";
        launch_fi_bwd_c3_mx<T, FT, 0>(k);
    } else {                                   // no image gradient (its PART 2)
        t_mx_grad_path = "fi_bwd_mx:tiled_c3_noimage";
        launch_fi_bwd_c3_mx<T, FT, 2>(k);
    }
    return launch_status();
}

// fp32 tensors need dword alignment only (f32x4u); a T tensor -- the taps, their gradient, a flow in T -- 8-byte quads
inline bool dword_ok(const memc_tensor4 *t) { return reinterpret_cast<uintptr_t>(t->data) % 4 == 0; }

}  // namespace

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
    if (!ok(input1) || !ok(input2) || !ok(input3) || !ok(gradoutput) || (gradinput1 && !ok(gradinput1)) ||
        !ok(gradinput2) || !ok(gradinput3))
        return kErr;                                                                // my_lib_cuda.c:716-718
    if (!flow_matches(input1, input2) || !taps_match(input1, input3)) return kErr;  // :685-691
    const int64_t taps = input3->size[1];
    const int fs = (int)lround(sqrt((double)taps));                                 // :693-694
    if (fs < 1 || (int64_t)fs * fs != taps) return kErr;
    if ((gradinput1 && !same_layout(input1, gradinput1)) || !same_layout(input2, gradinput2) ||
        !same_layout(input3, gradinput3) || !same_layout(input1, gradoutput))
        return kErr;                                                                // :719-723
    const int n = (int)input1->size[0], c = (int)input1->size[1], h = (int)input1->size[2], w = (int)input1->size[3];
    if (n == 0 || c == 0 || h == 0 || w == 0) return 0;
    // coverage: the tiled RGB kernel on 8-byte half quads; anything else is the caller's (promoted) business
    bool covered = c == 3 && fs == 4 && w % 4 == 0 && w >= 8 &&
                   plane_fits_u32(w, h, {(long)input1->stride[2], (long)input2->stride[2], (long)input3->stride[2]});
    for (const memc_tensor4 *t : {input3, gradinput3}) covered = covered && quad_ok(t);
    for (const memc_tensor4 *t : {input1, gradoutput}) covered = covered && dword_ok(t);
    if (gradinput1) covered = covered && dword_ok(gradinput1);
    if (flowt == tapt) covered = covered && quad_ok(input2) && quad_ok(gradinput2);
    else covered = covered && dword_ok(input2) && dword_ok(gradinput2);
    if (!covered) return kNotCovered;
    const hipStream_t s = (hipStream_t)stream;
#define MEMC_MXG_LAUNCH(T, FT) \
    fi_bwd_mx_launch<T, FT>(s, w, h, n, input1, input2, input3, gradoutput, gradinput1, gradinput2, gradinput3)
    const int r = tapt == MEMC_F16 ? (flowt == MEMC_F32 ? MEMC_MXG_LAUNCH(F16, F32) : MEMC_MXG_LAUNCH(F16, F16))
                                   : (flowt == MEMC_F32 ? MEMC_MXG_LAUNCH(BF16, F32) : MEMC_MXG_LAUNCH(BF16, BF16));
#undef MEMC_MXG_LAUNCH
    return r == 0 ? 0 : kErr;
}

}  // extern "C"
