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
#include "memc_desc.hpp"
#include "memc_launch.hpp"
#include "memc_warp_lp_grad.h"

#include <math.h>

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
namespace {

using namespace memc;
constexpr int kErr = -1;
constexpr int kNotCovered = 1;

template <class P, class FT, class GT, int PART>
void launch_fi_bwd_c3_lp(const FiBwdCall<st_t<P>, st_t<FT>, st_t<GT>> &k)
{
    using G = TileGeom<16>;
    const int ntx = (k.w + G::kTW - 1) / G::kTW, nty = (k.h + G::kTH - 1) / G::kTH;
    hipLaunchKernelGGL((fi_bwd_c3_lp<P, FT, GT, PART>), dim3((unsigned)ntx * nty * k.batch), dim3(256), PkGeom::kLds, k.stream,
                       k.w, k.h, ntx, nty, k.batch, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c, k.s2.h, k.s3.b, k.s3.c, k.s3.h,
                       k.in1, k.flow, k.filt, k.gout, k.gin1, k.gin2, k.gin3);
}

template <class P, class FT, class GT>
int fi_bwd_lp_launch(hipStream_t stream, int w, int h, int n, const memc_tensor4 *in1, const memc_tensor4 *flow,
                     const memc_tensor4 *filt, const memc_tensor4 *gout, const memc_tensor4 *gin1, const memc_tensor4 *gin2,
                     const memc_tensor4 *gin3)
{
    const FiBwdCall<st_t<P>, st_t<FT>, st_t<GT>> k = {
        stream, w, h, 3, n, 4, plane(in1), plane(flow), plane(filt),
        reinterpret_cast<const st_t<P> *>(in1->data), reinterpret_cast<const st_t<FT> *>(flow->data),
        reinterpret_cast<const st_t<P> *>(filt->data), reinterpret_cast<const st_t<GT> *>(gout->data),
        gin1 ? reinterpret_cast<float *>(gin1->data) : nullptr, reinterpret_cast<st_t<FT> *>(gin2->data),
        reinterpret_cast<st_t<P> *>(gin3->data)};
    if (k.gin1) {                              // the whole backward (the fp32 launcher's PART 0)
        t_lp_grad_path = "fi_bwd_lp:tiled_c3";
        launch_fi_bwd_c3_lp<P, FT, GT, 0>(k);
    } else {                                   // no image gradient (its PART 2)
        t_lp_grad_path = "fi_bwd_lp:tiled_c3_noimage";
        launch_fi_bwd_c3_lp<P, FT, GT, 2>(k);
    }
    return launch_status();
}

// the eight (payload, flow, gradoutput) instantiations
template <class P>
int dispatch_lp(memc_dtype flowt, memc_dtype goutt, hipStream_t stream, int w, int h, int n, const memc_tensor4 *in1,
                const memc_tensor4 *flow, const memc_tensor4 *filt, const memc_tensor4 *gout, const memc_tensor4 *gin1,
                const memc_tensor4 *gin2, const memc_tensor4 *gin3)
{
    if (flowt == MEMC_F32)
        return goutt == MEMC_F32 ? fi_bwd_lp_launch<P, F32, F32>(stream, w, h, n, in1, flow, filt, gout, gin1, gin2, gin3)
                                 : fi_bwd_lp_launch<P, F32, P>(stream, w, h, n, in1, flow, filt, gout, gin1, gin2, gin3);
    return goutt == MEMC_F32 ? fi_bwd_lp_launch<P, P, F32>(stream, w, h, n, in1, flow, filt, gout, gin1, gin2, gin3)
                             : fi_bwd_lp_launch<P, P, P>(stream, w, h, n, in1, flow, filt, gout, gin1, gin2, gin3);
}

}  // namespace

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
    // coverage: the tiled RGB kernel on 8-byte half quads; anything else is the caller's (widened) business
    bool covered = c == 3 && fs == 4 && w % 4 == 0 && w >= 8 &&
                   plane_fits_u32(w, h, {(long)input1->stride[2], (long)input2->stride[2], (long)input3->stride[2]});
    for (const memc_tensor4 *t : {input1, input3, gradinput3}) covered = covered && quad_ok(t);
    if (flowt == payload) covered = covered && quad_ok(input2) && quad_ok(gradinput2);
    if (goutt == payload) covered = covered && quad_ok(gradoutput);
    if (!covered) return kNotCovered;
    const hipStream_t s = (hipStream_t)stream;
    const int r = payload == MEMC_F16
                      ? dispatch_lp<F16>(flowt, goutt, s, w, h, n, input1, input2, input3, gradoutput, gradinput1, gradinput2,
                                         gradinput3)
                      : dispatch_lp<BF16>(flowt, goutt, s, w, h, n, input1, input2, input3, gradoutput, gradinput1, gradinput2,
                                          gradinput3);
    return r == 0 ? 0 : kErr;
}

}  // extern "C"
