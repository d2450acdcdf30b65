// memc_fi_abi.hpp -- what the C ABIs of the eight satellite warp libraries share (host code only): lp_filter_interpolation.hip
// (memc_warp_lp.h), lp_fi_bwd_c3.hip (memc_warp_lp_grad.h), fi_blend_bwd_c3.hip (memc_warp_blend_grad.h),
// mx_filter_interpolation.hip (memc_warp_mx.h), mx_fi_bwd_c3.hip (memc_warp_mx_grad.h), mx_fi_blend_bwd_c3.hip
// (memc_warp_mx_blend_grad.h), lp_fi_blend_bwd_c3.hip (memc_warp_lp_blend_grad.h) and fi_stack.hip (memc_warp_stack.h: the
// filter-side rule, the sizes, the tile grid and the return codes).  The filter-side rules, the
// coverage predicates, the three check sequences that more than one entry point runs, the tile grid, the call descriptors
// filled from the tensors, the launch of the tiled backward kernels, the backward's PART choice and the dtype dispatch.  An
// entry point keeps its dtype check, its filter-side rule, its coverage test and its path strings; the order of every
// sequence is memc_desc.hpp's contract: malformed (-1), then empty (0), then -- the entry point's own -- not covered (1),
// then the launch.
#pragma once

#include "memc_common.hpp"                     // launch_status
#include "memc_desc.hpp"
#include "memc_launch.hpp"
#include "memc_lp.hpp"                         // the storage tags F32 / F16 / BF16; memc_tile.hpp: TileGeom

#include <initializer_list>
#include <math.h>
#include <type_traits>

namespace memc {

constexpr int kErr = -1;
constexpr int kNotCovered = 1;

// The filter's side from the tap count; below 1: malformed.  Exact: only a square count has a side.  Ref: the reference's
// truncation (my_lib_cuda.c:619-620, :693-694), which takes 8 taps for a 2 x 2 filter.  Each entry point names its rule.
inline int fi_filter_side_exact(int64_t taps)
{
    const int fs = (int)lround(sqrt((double)taps));
    return (int64_t)fs * fs == taps ? fs : 0;
}
inline int fi_filter_side_ref(int64_t taps) { return (int)sqrt((float)taps); }

// occlusion [N, 1, H, W] matching input [N, C, H, W]
inline bool occlusion_matches(const memc_tensor4 *in1, const memc_tensor4 *occ)
{
    return occ->size[0] == in1->size[0] && occ->size[1] == 1 && occ->size[2] == in1->size[2] && occ->size[3] == in1->size[3];
}

// Aligned for its storage: an fp32 tensor needs dword alignment only (f32x4u), a half tensor 8-byte quads (quad_ok).
// `ts`: tensors stored as `dt`; a NULL one (an optional gradient) passes.
inline bool dword_ok(const memc_tensor4 *t) { return reinterpret_cast<uintptr_t>(t->data) % 4 == 0; }
inline bool storage_ok(memc_dtype dt, std::initializer_list<const memc_tensor4 *> ts)
{
    for (const memc_tensor4 *t : ts)
        if (t && !(dt == MEMC_F32 ? dword_ok(t) : quad_ok(t))) return false;
    return true;
}

// the shapes the RGB tiled kernels take: whole quads, at least two of them
inline bool fi_rgb_tiled_shape(int c, int fs, int w) { return c == 3 && fs == 4 && w % 4 == 0 && w >= 8; }

// What a shared check sequence found: `done` with the entry point's return code, or go on with the call's sizes.
struct FiChecked {
    bool done;
    int code, fs, n, c, h, w;
};
inline FiChecked fi_sizes(int fs, const memc_tensor4 *in1)
{
    const int n = (int)in1->size[0], c = (int)in1->size[1], h = (int)in1->size[2], w = (int)in1->size[3];
    return {n == 0 || c == 0 || h == 0 || w == 0, 0, fs, n, c, h, w};
}

// The backward warp's seven tensors (gradinput1 may be NULL: no image gradient).
inline FiChecked fi_bwd_checked(int (*side)(int64_t), const memc_tensor4 *input1, const memc_tensor4 *input2,
                                const memc_tensor4 *input3, const memc_tensor4 *gradoutput, const memc_tensor4 *gradinput1,
                                const memc_tensor4 *gradinput2, const memc_tensor4 *gradinput3)
{
    const FiChecked bad = {true, kErr, 0, 0, 0, 0, 0};
    if (!ok(input1) || !ok(input2) || !ok(input3) || !ok(gradoutput) || (gradinput1 && !ok(gradinput1)) ||
        !ok(gradinput2) || !ok(gradinput3))
        return bad;                                                                 // my_lib_cuda.c:716-718
    if (!flow_matches(input1, input2) || !taps_match(input1, input3)) return bad;   // :685-691
    const int fs = side(input3->size[1]);                                           // :693-694
    if (fs < 1) return bad;
    if ((gradinput1 && !same_layout(input1, gradinput1)) || !same_layout(input2, gradinput2) ||
        !same_layout(input3, gradinput3) || !same_layout(input1, gradoutput))
        return bad;                                                                 // :719-723
    return fi_sizes(fs, input1);
}

// One direction of the blend's backward: its eight tensors (no image gradient).
inline FiChecked fi_blend_bwd_checked(int (*side)(int64_t), const memc_tensor4 *input, const memc_tensor4 *flow,
                                      const memc_tensor4 *filter, const memc_tensor4 *occlusion,
                                      const memc_tensor4 *gradoutput, const memc_tensor4 *gradflow,
                                      const memc_tensor4 *gradfilter, const memc_tensor4 *gradocclusion)
{
    const FiChecked bad = {true, kErr, 0, 0, 0, 0, 0};
    for (const memc_tensor4 *t : {input, flow, filter, occlusion, gradoutput, gradflow, gradfilter, gradocclusion})
        if (!ok(t)) return bad;
    if (!flow_matches(input, flow) || !taps_match(input, filter) || !occlusion_matches(input, occlusion)) return bad;
    const int fs = side(filter->size[1]);
    if (fs < 1) return bad;
    if (!same_layout(input, gradoutput) || !same_layout(flow, gradflow) || !same_layout(filter, gradfilter) ||
        !same_layout(occlusion, gradocclusion))
        return bad;
    return fi_sizes(fs, input);
}

// The blend forward's nine tensors: input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1, output.
inline FiChecked fi_blend_fwd_checked(int (*side)(int64_t), const memc_tensor4 *const (&t)[9])
{
    const FiChecked bad = {true, kErr, 0, 0, 0, 0, 0};
    for (const memc_tensor4 *x : t)
        if (!ok(x)) return bad;
    if (!flow_matches(t[0], t[2]) || !taps_match(t[0], t[4])) return bad;
    if (!same_layout(t[0], t[1]) || !same_layout(t[0], t[8]) || !same_layout(t[2], t[3]) || !same_layout(t[4], t[5]) ||
        !same_layout(t[6], t[7]))
        return bad;
    if (!occlusion_matches(t[0], t[6])) return bad;
    const int fs = side(t[4]->size[1]);
    if (fs < 1) return bad;
    return fi_sizes(fs, t[0]);
}

// The tiles of geometry G (memc_tile.hpp: TileGeom) that cover w x h sites, the last column and row ragged.
struct TileGrid {
    int ntx, nty;
};
template <class G>
inline TileGrid fi_tile_grid(int w, int h)
{
    return {(w + G::kTW - 1) / G::kTW, (h + G::kTH - 1) / G::kTH};
}

// The call descriptors (memc_launch.hpp) from the checked tensors.  T, FT, GT, IT: storage tags.
template <class S>
inline st_t<S> *data_of(const memc_tensor4 *t) { return t ? reinterpret_cast<st_t<S> *>(t->data) : nullptr; }

template <class T, class FT, class IT = T>
inline FiFwdCall<st_t<T>, st_t<FT>, st_t<IT>> fi_fwd_call(hipStream_t stream, const FiChecked &q, const memc_tensor4 *in1,
                                                          const memc_tensor4 *flow, const memc_tensor4 *filt,
                                                          const memc_tensor4 *out)
{
    return {stream, q.w, q.h, q.c, q.n, q.fs, plane(in1), plane(flow), plane(filt),
            data_of<IT>(in1), data_of<FT>(flow), data_of<T>(filt), data_of<IT>(out)};
}

template <class T, class FT, class IT = T>
inline FiBlendFwdCall<st_t<T>, st_t<FT>, st_t<IT>> fi_blend_fwd_call(hipStream_t stream, const FiChecked &q,
                                                                     const memc_tensor4 *const (&t)[9])
{
    return {stream, q.w, q.h, q.c, q.n, q.fs, plane(t[0]), plane(t[2]), plane(t[4]), plane(t[6]),
            data_of<IT>(t[0]), data_of<IT>(t[1]), data_of<FT>(t[2]), data_of<FT>(t[3]), data_of<T>(t[4]), data_of<T>(t[5]),
            data_of<T>(t[6]), data_of<T>(t[7]), data_of<IT>(t[8])};
}

template <class T, class FT, class GT, class IT = T>
inline FiBwdCall<st_t<T>, st_t<FT>, st_t<GT>, st_t<IT>> fi_bwd_call(
    hipStream_t stream, const FiChecked &q, const memc_tensor4 *in1, const memc_tensor4 *flow, const memc_tensor4 *filt,
    const memc_tensor4 *gout, const memc_tensor4 *gin1, const memc_tensor4 *gin2, const memc_tensor4 *gin3)
{
    return {stream, q.w, q.h, q.c, q.n, q.fs, plane(in1), plane(flow), plane(filt),
            data_of<IT>(in1), data_of<FT>(flow), data_of<T>(filt), data_of<GT>(gout),
            data_of<F32>(gin1), data_of<FT>(gin2), data_of<T>(gin3)};
}

template <class T, class FT, class GT, class IT = T>
inline FiBlendBwdCall<st_t<T>, st_t<FT>, st_t<IT>, st_t<GT>> fi_blend_bwd_call(
    hipStream_t stream, const FiChecked &q, const memc_tensor4 *in1, const memc_tensor4 *flow, const memc_tensor4 *filt,
    const memc_tensor4 *occ, const memc_tensor4 *gout, const memc_tensor4 *gflow, const memc_tensor4 *gfilt,
    const memc_tensor4 *gocc)
{
    return {stream, q.w, q.h, q.n, plane(in1), plane(flow), plane(filt), plane(occ),
            data_of<IT>(in1), data_of<FT>(flow), data_of<T>(filt), data_of<T>(occ), data_of<GT>(gout),
            data_of<FT>(gflow), data_of<T>(gfilt), data_of<T>(gocc)};
}

// The launch of a tiled RGB backward kernel: one workgroup of G::kThreads lanes and `lds` bytes per tile of geometry G,
// one argument list per family -- the warp's seven tensors, the blend direction's eight.
template <class G, class Kernel, class T, class FT, class GT, class IT>
inline void fi_bwd_tiled_launch(Kernel kernel, int lds, const FiBwdCall<T, FT, GT, IT> &k)
{
    const TileGrid g = fi_tile_grid<G>(k.w, k.h);
    hipLaunchKernelGGL(kernel, dim3((unsigned)g.ntx * g.nty * k.batch), dim3(G::kThreads), lds, k.stream, k.w, k.h, g.ntx,
                       g.nty, k.batch, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c, k.s2.h, k.s3.b, k.s3.c, k.s3.h, k.in1, k.flow,
                       k.filt, k.gout, k.gin1, k.gin2, k.gin3);
}
template <class G, class Kernel, class T, class FT, class IT, class GT>
inline void fi_blend_bwd_tiled_launch(Kernel kernel, int lds, const FiBlendBwdCall<T, FT, IT, GT> &k)
{
    const TileGrid g = fi_tile_grid<G>(k.w, k.h);
    hipLaunchKernelGGL(kernel, dim3((unsigned)g.ntx * g.nty * k.batch), dim3(G::kThreads), lds, k.stream, k.w, k.h, g.ntx,
                       g.nty, k.batch, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c, k.s2.h, k.s3.b, k.s3.c, k.s3.h, k.s4.b, k.s4.h,
                       k.in1, k.flow, k.filt, k.occ, k.gout, k.gflow, k.gfilt, k.gocc);
}

// The RGB backward's launch: the whole backward where the image gradient is wanted (the fp32 launcher's PART 0), else
// the tap and flow gradients alone (its PART 2).  launch(k, std::integral_constant<int, PART>): the kernel's launch function.
template <class Call, class Launch>
inline int fi_bwd_launch(const Call &k, const char *&path, const char *whole, const char *noimage, Launch launch)
{
    if (k.gin1) {
        path = whole;
        launch(k, std::integral_constant<int, 0>());
    } else {
        path = noimage;
        launch(k, std::integral_constant<int, 2>());
    }
    return launch_status();
}

// The dtype dispatch: f(payload tag, flow tag) or f(payload tag, flow tag, gradoutput tag), after dtypes_ok.  The order
// is the order in which the compiler emits the kernels: F16 before BF16, an fp32 flow before a half one, an fp32
// gradoutput before a half one.
template <class F>
inline int fi_dispatch(memc_dtype payload, memc_dtype flowt, F f)
{
    if (payload == MEMC_F16) return flowt == MEMC_F32 ? f(F16(), F32()) : f(F16(), F16());
    return flowt == MEMC_F32 ? f(BF16(), F32()) : f(BF16(), BF16());
}
template <class F>
inline int fi_dispatch(memc_dtype payload, memc_dtype flowt, memc_dtype goutt, F f)
{
    return fi_dispatch(payload, flowt, [&](auto p, auto ft) { return goutt == MEMC_F32 ? f(p, ft, F32()) : f(p, ft, p); });
}

}  // namespace memc
