// memc_launch.hpp -- how the warp launchers hand a call to a kernel (host code only): the strides of a tensor as the
// kernels take them, and one call descriptor per operator family, filled once at the top of an entry point.  The launch
// function of a kernel family -- tile count, grid, LDS bytes and the argument list, spelled once -- is a function template
// beside the kernel (launch_fi_fwd_tiled_fs4 in filter_interpolation.hip, launch_proj_owner5 in flow_projection.hip,
// launch_fi_bwd_image_owner in fi_bwd_cn.hip, ...).  The measurement build's arms are one function per entry point, in
// arms/ (fi_fwd_arm_launch, proj_fwd_arm_launch, ...).  The warps' descriptors are templates over the
// tensors' storage: float in the fp32 library, st_t<...> (memc_lp.hpp) in the half-precision and mixed ones, which fill
// them from the memc_tensor4s with memc_fi_abi.hpp's fi_fwd_call / fi_blend_fwd_call / fi_bwd_call / fi_blend_bwd_call.
#pragma once

#include "memc_warp_lp.h"                      // memc_tensor4

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace memc {

// The three strides a kernel takes per tensor, in elements: batch and channel as int64_t (b * s.b must not wrap), the row
// stride as int.  The w stride is 1 (memc_desc.hpp: ok()).  THE place where a launcher's strides are widened.
struct Plane {
    int64_t b, c;
    int h;
};
inline Plane plane(int sb, int sc, int sh) { return {(int64_t)sb, (int64_t)sc, sh}; }          // the fp32 launcher ABI
inline Plane plane(const memc_tensor4 *t) { return {t->stride[0], t->stride[1], (int)t->stride[2]}; }

// FilterInterpolation forward.  s1: input1 and output; s2: the flow; s3: the filter taps.  IT: the storage of input1 and the
// output where it is not the taps' (the mixed library: float beside half taps).
template <class T = float, class FT = T, class IT = T>
struct FiFwdCall {
    hipStream_t stream;
    int w, h, channel, batch, filter_size;
    Plane s1, s2, s3;
    const IT *in1;  const FT *flow;  const T *filt;  IT *out;
};

// The fused dual warp + occlusion blend forward.  s1: the images and the output; s2: the flows; s3: the taps; so: the
// occlusions (so.c is not used).  IT as above.
template <class T = float, class FT = T, class IT = T>
struct FiBlendFwdCall {
    hipStream_t stream;
    int w, h, channel, batch, filter_size;
    Plane s1, s2, s3, so;
    const IT *in0, *in2;  const FT *flow0, *flow1;  const T *filt0, *filt1, *occ0, *occ1;  IT *out;
};

// FilterInterpolation backward.  s1: input1, gradoutput and gradinput1 (always fp32: the tiles' flushes add into it; NULL:
// not wanted); s2: the flow and gradinput2; s3: the taps and gradinput3.  IT: the storage of input1 where it is not the
// taps' (the mixed backward library: float beside half taps).
template <class T = float, class FT = T, class GT = T, class IT = T>
struct FiBwdCall {
    hipStream_t stream;
    int w, h, channel, batch, filter_size;
    Plane s1, s2, s3;
    const IT *in1;  const FT *flow;  const T *filt;  const GT *gout;
    float *gin1;  FT *gin2;  T *gin3;
};

// One direction of the blend's backward (no image gradient).  s1: the image and gradoutput; s2: the flow and its gradient;
// s3: the taps and their gradient; s4: the occlusion and its gradient (one channel: s4.c is not used).
template <class T = float, class FT = float, class IT = float, class GT = float>
struct FiBlendBwdCall {
    hipStream_t stream;
    int w, h, batch;
    Plane s1, s2, s3, s4;
    const IT *in1;  const FT *flow;  const T *filt, *occ;  const GT *gout;
    FT *gflow;  T *gfilt, *gocc;
};

// The bilinear warp (Interpolation / InterpolationCh).  s1: input1, output / gradoutput, gradinput1; s2: the flow, gradinput2.
struct BlFwdCall {
    hipStream_t stream;
    int w, h, channel, batch;
    Plane s1, s2;
    const float *in1, *flow;
    float *out;
};
struct BlBwdCall {
    hipStream_t stream;
    int w, h, channel, batch;
    Plane s1, s2;
    const float *in1, *flow, *gout;
    float *gin1, *gin2;
};

// FlowProjection / DepthFlowProjection.  s1: the flow, the output / gradoutput, gradinput1; sd: the depth and gradinput2
// (sd.c is not used; zeros without a depth); sc: the count (sc.c is not used).  ws: the caller's workspace (the _ws entry
// points) or nullptr: the library's own scratch block.
struct ProjFwdCall {
    hipStream_t stream;
    int w, h, batch, fillhole;
    Plane s1, sd, sc;
    const float *flow, *depth;
    float *count, *out;
    void *ws;
    size_t ws_bytes;
};
struct ProjBwdCall {
    hipStream_t stream;
    int w, h, batch;
    Plane s1, sd, sc;
    const float *flow, *depth, *count, *fwd_out, *gout;
    float *gin1, *gin2;
};

}  // namespace memc
