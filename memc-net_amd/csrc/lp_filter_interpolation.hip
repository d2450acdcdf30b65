// lp_filter_interpolation.hip -- the adaptive warp (FilterInterpolation) forward and the fused dual warp + occlusion blend
// on fp16 / bf16 storage, for gfx950: the kernels and the C ABI of libmemc_hip_lp.so (include/memc_warp_lp.h).
//
// The fp32 kernels (filter_interpolation.hip) are HBM-bound gather stencils; half-width storage is what removes bytes.
// RGB forward per site: image 6 + flow 8 (fp32) or 4 (T) + taps 32 + output 6 = 52 / 48 B instead of 96; blend 102 / 94 B
// instead of 188; the 64-channel context warp 296 B instead of 584.  The kernels are the fp32 kernels' structure on
// narrower global accesses (memc_lp.hpp):
//   fi_fwd_lp_tiled<T, FT, true>    RGB: fi_fwd_tiled_fs4<16, 3, ...>'s band loop, results kept until every band has run;
//   fi_fwd_lp_tiled<T, FT, false>   any other channel count: fi_fwd_tiled_c4n's chunk pipeline (the next chunk's rows in
//                                   flight while this one is gathered), a ragged last chunk re-reads the last plane;
//   fi_blend_lp_tiled<T, FT>        fi_fwd_blend_c3: both directions' streams up front, one box -> stage -> gather round each;
//   fi_fwd_lp_direct / fi_blend_lp_direct   one lane per site, any filter size, any width, any alignment.
// The LDS holds fp32 pixel quads (staging widens), so the gather and its arithmetic are the fp32 kernels' own: the site
// geometry, the gather and the one-site paths from global memory are memc_fi.hpp's, the descriptor checks memc_desc.hpp's,
// what the satellite libraries' C ABIs share memc_fi_abi.hpp's.
// The two tiled kernels' bodies (lp_fi_fwd_body.inc, lp_fi_blend_body.inc) are shared with libmemc_hip_mx.so (an fp32
// image beside half taps).
#include "memc_common.hpp"
#include "memc_tile.hpp"
#include "memc_fi.hpp"
#include "memc_lp.hpp"
#include "memc_lp_fi.hpp"
#include "memc_fi_abi.hpp"
#include "memc_warp_lp.h"

namespace memc {

thread_local const char *t_lp_path = "";

// The tiled kernels: the bodies lp_fi_fwd_body.inc / lp_fi_blend_body.inc with the image in T (libmemc_hip_mx.so runs the
// same bodies on an fp32 image).
template <class T, class FT, bool RGB, bool RAGGED = false>
__global__ __launch_bounds__(256, RAGGED ? 1 : 2) void fi_fwd_lp_tiled(
    int W, int H, int C, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    const st_t<T> *__restrict__ in1, const st_t<FT> *__restrict__ flow, const st_t<T> *__restrict__ filt,
    st_t<T> *__restrict__ out)
{
    using I = T;                               // the image and the output in the taps' storage
#include "lp_fi_fwd_body.inc"
}

template <class T, class FT>
__global__ __launch_bounds__(256, 2) void fi_blend_lp_tiled(
    int W, int H, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    int64_t sob, int soh,
    const st_t<T> *__restrict__ in0, const st_t<T> *__restrict__ in2, const st_t<FT> *__restrict__ flow0,
    const st_t<FT> *__restrict__ flow1, const st_t<T> *__restrict__ filt0, const st_t<T> *__restrict__ filt1,
    const st_t<T> *__restrict__ occ0, const st_t<T> *__restrict__ occ1, st_t<T> *__restrict__ out)
{
    using I = T;
#include "lp_fi_blend_body.inc"
}

// --------------------------------------------------------------------------------------------------
// One lane per site, any filter size, any width / strides / alignment: what the tiled kernels do not take.
// 64 x 4 sites per workgroup.  BLEND: the dual warp + blend of any channel count and filter size.
// --------------------------------------------------------------------------------------------------
template <class T, class FT>
__global__ __launch_bounds__(256) void fi_fwd_lp_direct(
    int W, int H, int C, int fs, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    const st_t<T> *__restrict__ in1, const st_t<FT> *__restrict__ flow, const st_t<T> *__restrict__ filt,
    st_t<T> *__restrict__ out)
{
    const unsigned t = xcd_chunked_id(blockIdx.x, gridDim.x);
    const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y, b = t / (tiles_x * tiles_y);
    const int x = tx * kWave + (threadIdx.x & (kWave - 1)), y = ty * 4 + (threadIdx.x / kWave);
    if (x >= W || y >= H) return;
    fi_site_scalar_lp<T, FT>(x, y, W, H, C, fs, in1 + b * s1b, s1c, s1h, flow + b * s2b + (int64_t)y * s2h + x, s2c,
                          filt + b * s3b + (int64_t)y * s3h + x, s3c, out + b * s1b + (int64_t)y * s1h + x);
}

template <class T, class FT>
__global__ __launch_bounds__(256) void fi_blend_lp_direct(
    int W, int H, int C, int fs, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    int64_t sob, int soh,
    const st_t<T> *__restrict__ in0, const st_t<T> *__restrict__ in2, const st_t<FT> *__restrict__ flow0,
    const st_t<FT> *__restrict__ flow1, const st_t<T> *__restrict__ filt0, const st_t<T> *__restrict__ filt1,
    const st_t<T> *__restrict__ occ0, const st_t<T> *__restrict__ occ1, st_t<T> *__restrict__ out)
{
    const unsigned t = xcd_chunked_id(blockIdx.x, gridDim.x);
    const int tx = t % tiles_x, ty = (t / tiles_x) % tiles_y, b = t / (tiles_x * tiles_y);
    const int x = tx * kWave + (threadIdx.x & (kWave - 1)), y = ty * 4 + (threadIdx.x / kWave);
    if (x >= W || y >= H) return;
    const int64_t o1 = b * s1b + (int64_t)y * s1h + x, o2 = b * s2b + (int64_t)y * s2h + x,
                  o3 = b * s3b + (int64_t)y * s3h + x, oo = b * sob + (int64_t)y * soh + x;
    const FiSite s0 = fi_locate(x, y, W, H, widen<FT>(flow0[o2]), widen<FT>(flow0[o2 + s2c]));
    const FiSite s1 = fi_locate(x, y, W, H, widen<FT>(flow1[o2]), widen<FT>(flow1[o2 + s2c]));
    const float oc0 = widen<T>(occ0[oo]), oc1 = widen<T>(occ1[oo]);
    const st_t<T> *i0 = in0 + b * s1b, *i2 = in2 + b * s1b;
    const int L0 = s0.ix + 1 - fs / 2, T0 = s0.iy + 1 - fs / 2, L1 = s1.ix + 1 - fs / 2, T1 = s1.iy + 1 - fs / 2;   // windows
    for (int c = 0; c < C; c++) {
        const float w0 = s0.valid ? fi_site_chan<T, int64_t>(s0, fs, L0, T0, L0 + fs, T0 + fs, W, H, i0 + c * s1c, s1h, filt0 + o3, s3c) : widen<T>(in0[o1 + c * s1c]);
        const float w2 = s1.valid ? fi_site_chan<T, int64_t>(s1, fs, L1, T1, L1 + fs, T1 + fs, W, H, i2 + c * s1c, s1h, filt1 + o3, s3c) : widen<T>(in2[o1 + c * s1c]);
        const float p0 = oc0 * w0, p2 = oc1 * w2;
        out[o1 + c * s1c] = narrow<T>(p0 + p2);
    }
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_lp.h)
// ==================================================================================================
namespace {

using namespace memc;

template <class T, class FT, bool RGB, bool RAGGED = false>
void launch_fi_fwd_lp_tiled(const FiFwdCall<st_t<T>, st_t<FT>> &k)
{
    const TileGrid g = fi_tile_grid<TileGeom<16>>(k.w, k.h);
    hipLaunchKernelGGL((fi_fwd_lp_tiled<T, FT, RGB, RAGGED>), dim3((unsigned)g.ntx * g.nty * k.batch), dim3(256),
                       tile_lds_bytes<16>(), k.stream, k.w, k.h, k.channel, g.ntx, g.nty, k.s1.b, k.s1.c, k.s1.h, k.s2.b,
                       k.s2.c, k.s2.h, k.s3.b, k.s3.c, k.s3.h, k.in1, k.flow, k.filt, k.out);
}

template <class T, class FT>
int fi_fwd_lp_launch(const FiFwdCall<st_t<T>, st_t<FT>> &k, bool tiled)
{
    if (tiled) {
        if (k.channel == 3) {
            t_lp_path = "fi_fwd_lp:tiled_c3";
            launch_fi_fwd_lp_tiled<T, FT, true, false>(k);
        } else {
            t_lp_path = "fi_fwd_lp:tiled_c4n";
            if (k.channel % 4 == 0) launch_fi_fwd_lp_tiled<T, FT, false, false>(k);
            else launch_fi_fwd_lp_tiled<T, FT, false, true>(k);
        }
    } else {
        const int tiles_x = (k.w + kWave - 1) / kWave, tiles_y = (k.h + 3) / 4;
        t_lp_path = "fi_fwd_lp:direct";
        hipLaunchKernelGGL((fi_fwd_lp_direct<T, FT>), dim3((unsigned)tiles_x * tiles_y * k.batch), dim3(256), 0, k.stream,
                           k.w, k.h, k.channel, k.filter_size, tiles_x, tiles_y, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c,
                           k.s2.h, k.s3.b, k.s3.c, k.s3.h, k.in1, k.flow, k.filt, k.out);
    }
    return launch_status();
}

template <class T, class FT>
int fi_blend_lp_launch(const FiBlendFwdCall<st_t<T>, st_t<FT>> &k, bool tiled)
{
    if (tiled) {
        const TileGrid g = fi_tile_grid<TileGeom<16>>(k.w, k.h);
        t_lp_path = "fi_blend_lp:tiled_c3";
        hipLaunchKernelGGL((fi_blend_lp_tiled<T, FT>), dim3((unsigned)g.ntx * g.nty * k.batch), dim3(256),
                           tile_lds_bytes<16>(), k.stream, k.w, k.h, g.ntx, g.nty, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c,
                           k.s2.h, k.s3.b, k.s3.c, k.s3.h, k.so.b, k.so.h, k.in0, k.in2, k.flow0, k.flow1, k.filt0, k.filt1,
                           k.occ0, k.occ1, k.out);
    } else {
        const int tiles_x = (k.w + kWave - 1) / kWave, tiles_y = (k.h + 3) / 4;
        t_lp_path = "fi_blend_lp:direct";
        hipLaunchKernelGGL((fi_blend_lp_direct<T, FT>), dim3((unsigned)tiles_x * tiles_y * k.batch), dim3(256), 0, k.stream,
                           k.w, k.h, k.channel, k.filter_size, tiles_x, tiles_y, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c,
                           k.s2.h, k.s3.b, k.s3.c, k.s3.h, k.so.b, k.so.h, k.in0, k.in2, k.flow0, k.flow1, k.filt0, k.filt1,
                           k.occ0, k.occ1, k.out);
    }
    return launch_status();
}

}  // namespace

extern "C" {

const char *memc_lp_version(void) { return "memc_hip_lp 0.1 gfx950"; }

const char *memc_lp_last_kernel_path(void) { return memc::t_lp_path; }

int FilterInterpolationLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype payload, memc_dtype flowt,
                                            const memc_tensor4 *input1, const memc_tensor4 *input2,
                                            const memc_tensor4 *input3, const memc_tensor4 *output)
{
    if (!dtypes_ok(payload, flowt)) return kErr;
    if (!ok(input1) || !ok(input2) || !ok(input3) || !ok(output)) return kErr;        // my_lib_cuda.c:641-643
    if (!flow_matches(input1, input2) || !taps_match(input1, input3)) return kErr;    // :611-617
    const int fs = fi_filter_side_ref(input3->size[1]);                               // :619-620
    if (fs < 1) return kErr;
    if (!same_layout(input1, output)) return kErr;                                    // :644-645 (+h)
    const FiChecked q = fi_sizes(fs, input1);
    if (q.done) return q.code;
    const bool tiled = fs == 4 && q.w % 4 == 0 && q.w >= 8 && quad_ok(input1) && quad_ok(input2) && quad_ok(input3) &&
                       quad_ok(output);
    return fi_dispatch(payload, flowt, [&](auto t, auto ft) {
        using T = decltype(t);
        using FT = decltype(ft);
        return fi_fwd_lp_launch<T, FT>(fi_fwd_call<T, FT>((hipStream_t)stream, q, input1, input2, input3, output), tiled);
    });
}

int FilterInterpolationBlendLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype payload, memc_dtype flowt,
                                                 const memc_tensor4 *input0, const memc_tensor4 *input2,
                                                 const memc_tensor4 *flow0, const memc_tensor4 *flow1,
                                                 const memc_tensor4 *filter0, const memc_tensor4 *filter1,
                                                 const memc_tensor4 *occlusion0, const memc_tensor4 *occlusion1,
                                                 const memc_tensor4 *output)
{
    if (!dtypes_ok(payload, flowt)) return kErr;
    const memc_tensor4 *const all[9] = {input0, input2, flow0, flow1, filter0, filter1, occlusion0, occlusion1, output};
    const FiChecked q = fi_blend_fwd_checked(fi_filter_side_ref, all);
    if (q.done) return q.code;
    bool tiled = fi_rgb_tiled_shape(q.c, q.fs, q.w);
    for (const memc_tensor4 *t : all) tiled = tiled && quad_ok(t);
    return fi_dispatch(payload, flowt, [&](auto t, auto ft) {
        using T = decltype(t);
        using FT = decltype(ft);
        return fi_blend_lp_launch<T, FT>(fi_blend_fwd_call<T, FT>((hipStream_t)stream, q, all), tiled);
    });
}

}  // extern "C"
