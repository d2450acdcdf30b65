// lp_spynet_level.hip -- the input of one SPyNet pyramid level on fp16 / bf16 storage, for gfx950: the kernels and the C ABI
// of libmemc_hip_spynet_lp.so (include/memc_spynet_lp.h).
//
// spynet_level_lp<T, QUAD> restates spynet_level<QUAD> (spynet_level.hip) on half storage: `first`, `second`, `coarse` and
// `out` are all of T (F16 or BF16, the storage tags of memc_lp.hpp).  The arithmetic is the fp32 kernel's, in the fp32
// kernel's order, on exactly widened inputs: level_up_index, level_flow, level_position, level_corners and the site body
// level_site are memc_spynet_level.hpp's, instantiated on T -- one text for both units, and every element reaches it as an
// opaque fp32 value, so the compiler is handed the fp32 unit's expressions.  The warp uses the UNROUNDED fp32 `up`.  Every
// stored element is rounded ONCE (narrow<T>: round-to-nearest-even, overflow to +-inf, what `tensor.to(T)` does) where it
// is stored: out[:, 3:6] and out[:, 6:8].  out[:, 0:3] is a copy of `first`'s 16-bit patterns, not widened and narrowed
// again.  Contract: `out` equals, bit for bit, SpyNetLevelLayer_gpu_forward on the widened inputs followed by one .to(T),
// for the same kernel family.
//
// Two kernels of one body.  quad: four consecutive sites per lane, `first` read and `out` written as 8-byte quads of T
// (widths that are a multiple of four from 8 on, 8-byte aligned bases of `first` and `out` and b / c / h strides of theirs
// that are multiples of four elements; `second` and `coarse` are gathered element by element and need no alignment beyond
// their own).  direct: one lane per site, every other width, stride and alignment.
//
// Safety, unchanged from the fp32 kernel: the sample position is clamped into [-2, W + 1] x [-2, H + 1] by comparisons that
// send a NaN to -2 BEFORE any conversion to int, and every corner is read at an index clamped into the image and selected,
// not multiplied, by its in-range test: no flow value, however large or non-finite, forms an address outside `second`.  The
// coarse indices come from level_up_index of a site index, never from data.  No LDS, no atomics, no workspace; every element
// of `out` is assigned once.
#include "memc_common.hpp"
#include "memc_desc.hpp"
#include "memc_lp.hpp"
#include "memc_spynet_level.hpp"
#include "memc_spynet_lp.h"

#include <initializer_list>

namespace memc {

thread_local const char *t_spynet_lp_path = "";

// four fp32 values rounded to T, each once.  The quad as a whole is made opaque first: the compiler then sees one fp32
// vector consumed, as by the fp32 kernel's 16-byte store, and cannot fold the multiply or FMA that produced a value into
// its conversion (v_fma_mixlo_f16 would round the exact result, not the fp32 value).
template <class T>
__device__ __forceinline__ u16x4 narrow4(f32x4 v)
{
    asm volatile("" : "+v"(v));
    return u16x4{narrow<T>(v[0]), narrow<T>(v[1]), narrow<T>(v[2]), narrow<T>(v[3])};
}

// per_row: lanes per output row (QUAD: W / 4, else W).  Strides in elements of T: f first, s second, c coarse, o out.
template <class T, bool QUAD>
__global__ __launch_bounds__(256) void spynet_level_lp(
    int W, int H, int w, int h, int batch, int per_row, float sy, float sx, float kx, float ky, int align_up, int align_sample,
    int64_t sfb, int64_t sfc, int sfh, int64_t ssb, int64_t ssc, int ssh, int64_t scb, int64_t scc, int sch,
    int64_t sob, int64_t soc, int soh, const unsigned short *__restrict__ first, const unsigned short *__restrict__ second,
    const unsigned short *__restrict__ coarse, unsigned short *__restrict__ out)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    const int y = (int)(i / (unsigned)per_row);
    if (y >= H) return;
    const int x = ((int)i - y * per_row) * (QUAD ? 4 : 1);
    LevelRow r;
    {
        int y0, y1;
        level_up_index(min(y, 2 * h - 1), h, sy, align_up != 0, y0, y1, r.l0, r.l1);   // a padded row repeats row 2h - 1
        r.o0 = y0 * sch;
        r.o1 = y1 * sch;
    }
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const unsigned short *fp = first + b * sfb + (int64_t)y * sfh + x;
        const unsigned short *sb = second + b * ssb, *cb = coarse + b * scb;
        unsigned short *op = out + b * sob + (int64_t)y * soh + x;
        if constexpr (QUAD) {
            f32x4 ux, uy, wv[3];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float u, v, t[3];
                level_site<T>(x + j, y, W, H, w, sx, kx, ky, align_up != 0, align_sample != 0, r, cb, scc, sb, ssc, ssh, u, v, t);
                ux[j] = u;
                uy[j] = v;
#pragma unroll
                for (int c = 0; c < 3; c++) wv[c][j] = t[c];
            }
#pragma unroll
            for (int c = 0; c < 3; c++)
                *reinterpret_cast<u16x4a *>(op + c * soc) = *reinterpret_cast<const u16x4a *>(fp + c * sfc);
#pragma unroll
            for (int c = 0; c < 3; c++) *reinterpret_cast<u16x4a *>(op + (3 + c) * soc) = narrow4<T>(wv[c]);
            *reinterpret_cast<u16x4a *>(op + 6 * soc) = narrow4<T>(ux);
            *reinterpret_cast<u16x4a *>(op + 7 * soc) = narrow4<T>(uy);
        } else {
            float u, v, t[3];
            level_site<T>(x, y, W, H, w, sx, kx, ky, align_up != 0, align_sample != 0, r, cb, scc, sb, ssc, ssh, u, v, t);
#pragma unroll
            for (int c = 0; c < 3; c++) op[c * soc] = fp[c * sfc];
#pragma unroll
            for (int c = 0; c < 3; c++) op[(3 + c) * soc] = narrow_f32<T>(t[c]);
            op[6 * soc] = narrow_f32<T>(u);
            op[7 * soc] = narrow_f32<T>(v);
        }
    }
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_spynet_lp.h): memc_spynet.h's checks and return codes, in its order
// ==================================================================================================
namespace {

using namespace memc;

constexpr int kErr = -1;
constexpr int kNotCovered = 1;

// usable descriptor: sizes / strides fit int, non-null data unless empty (the w-stride is a matter of coverage here)
inline bool usable(const memc_tensor4 *t) { return t && fits_int(t) && (t->data || numel(t) == 0); }

inline bool shaped(const memc_tensor4 *t, int64_t n, int64_t c, int64_t h, int64_t w)
{
    return t->size[0] == n && t->size[1] == c && t->size[2] == h && t->size[3] == w;
}

// the bytes [lo, hi) a tensor's elements lie in: 2-byte elements
struct Span {
    uintptr_t lo, hi;
};
inline Span span_of(const memc_tensor4 *t)
{
    int64_t last = 0;
    for (int i = 0; i < 4; i++) last += (t->size[i] - 1) * t->stride[i];
    const uintptr_t lo = reinterpret_cast<uintptr_t>(t->data);
    return {lo, lo + (uintptr_t)(last + 1) * sizeof(unsigned short)};
}

}  // namespace

extern "C" {

const char *memc_spynet_lp_version(void) { return "memc_hip_spynet_lp 0.1 gfx950"; }

const char *memc_spynet_lp_last_kernel_path(void) { return memc::t_spynet_lp_path; }

int SpyNetLevelLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype dtype, const memc_tensor4 *first,
                                    const memc_tensor4 *second, const memc_tensor4 *coarse, const memc_tensor4 *out,
                                    int align_upsample, int align_sample)
{
    // malformed
    if (dtype != MEMC_F16 && dtype != MEMC_BF16) return kErr;
    if (!usable(first) || !usable(second) || !usable(coarse) || !usable(out)) return kErr;
    const int64_t B = first->size[0], H = first->size[2], W = first->size[3], h = coarse->size[2], w = coarse->size[3];
    if (!shaped(first, B, 3, H, W) || !shaped(second, B, 3, H, W) || !shaped(coarse, B, 2, h, w) || !shaped(out, B, 8, H, W))
        return kErr;
    if (H < 2 || W < 2 || (H != 2 * h && H != 2 * h + 1) || (W != 2 * w && W != 2 * w + 1)) return kErr;
    // empty
    if (B == 0) return 0;
    // not covered
    for (const memc_tensor4 *t : {first, second, coarse, out})
        if (t->size[3] > 1 && t->stride[3] != 1) return kNotCovered;
    for (const memc_tensor4 *t : {first, second, coarse, out})
        if ((t->size[2] - 1) * t->stride[2] + t->size[3] > INT32_MAX) return kNotCovered;
    const Span so = span_of(out);
    for (const memc_tensor4 *t : {first, second, coarse}) {
        const Span s = span_of(t);
        if (so.lo < s.hi && s.lo < so.hi) return kNotCovered;
    }
    // quads of four T: `first` is read and `out` written 8 bytes at a time; `second` and `coarse` are gathered by element
    const bool quad = W % 4 == 0 && W >= 8 && quad_ok(first) && quad_ok(out);
    const int per_row = quad ? (int)(W / 4) : (int)W;
    // ATen's scales: 1 / scale_factor, or (in - 1) / (out - 1) under align_corners, of the UNPADDED size 2h x 2w
    const float sy = align_upsample ? (h > 1 ? (float)(h - 1) / (float)(2 * h - 1) : 0.0f) : 0.5f;
    const float sx = align_upsample ? (w > 1 ? (float)(w - 1) / (float)(2 * w - 1) : 0.0f) : 0.5f;
    const float kx = (float)W / (float)(W - 1), ky = (float)H / (float)(H - 1);
    const unsigned blocks = (unsigned)(((int64_t)per_row * H + 255) / 256);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks, (unsigned)(B < 65535 ? B : 65535)), dim3(256), 0, (hipStream_t)stream, (int)W,
                           (int)H, (int)w, (int)h, (int)B, per_row, sy, sx, kx, ky, align_upsample, align_sample,
                           first->stride[0], first->stride[1], (int)first->stride[2], second->stride[0], second->stride[1],
                           (int)second->stride[2], coarse->stride[0], coarse->stride[1], (int)coarse->stride[2],
                           out->stride[0], out->stride[1], (int)out->stride[2], (const unsigned short *)first->data,
                           (const unsigned short *)second->data, (const unsigned short *)coarse->data,
                           (unsigned short *)out->data);
    };
    const bool f16 = dtype == MEMC_F16;
    if (quad) {
        t_spynet_lp_path = "spynet_level_lp:quad";
        if (f16) launch(spynet_level_lp<F16, true>);
        else launch(spynet_level_lp<BF16, true>);
    } else {
        t_spynet_lp_path = "spynet_level_lp:direct";
        if (f16) launch(spynet_level_lp<F16, false>);
        else launch(spynet_level_lp<BF16, false>);
    }
    return launch_status();
}

}  // extern "C"
