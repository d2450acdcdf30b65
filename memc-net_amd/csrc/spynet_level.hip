// spynet_level.hip -- the input of one SPyNet pyramid level in fp32, for gfx950: the kernels and the C ABI of
// libmemc_hip_spynet.so (include/memc_spynet.h).
//
// At each of up to six levels SPyNet upsamples the coarser flow x2 and doubles it, replicate-pads a row or column where the
// level's size is odd, warps the second frame with it (grid_sample, zero padding) and concatenates [first, warped second,
// upsampled flow] into the 8-channel input of the level's convolutions: nine or ten ATen launches, about 170 B moved per
// site.  Here one launch writes all eight channels: 12 B of `first` read, four gathers per channel of `second`, the coarse
// flow's four neighbours per channel, 32 B written.  No atomics, no workspace, no LDS: the coarse flow and the small levels
// are L2-resident and a smooth flow keeps neighbouring lanes on neighbouring lines, so the gathers go straight to global
// memory.
//
// Two kernels of one body.  quad: four consecutive sites per lane, dwordx4 loads of `first` and dwordx4 stores (widths that
// are a multiple of four from 8 on; such a width has no padded column, a padded row it can have).  direct: one lane per
// site, every other width (a 768 x 1344 frame has a 24 x 42 level).
//
// Safety: the sample position is clamped into [-2, W + 1] x [-2, H + 1] by comparisons that send a NaN to -2 BEFORE any
// conversion to int, and every corner is read at an index clamped into the image and selected, not multiplied, by its
// in-range test: no flow value, however large or non-finite, forms an address outside `second`.
#include "memc_common.hpp"
#include "memc_tile.hpp"
#include "memc_desc.hpp"
#include "memc_spynet_level.hpp"
#include "memc_spynet.h"

namespace memc {

thread_local const char *t_spynet_path = "";

// The site body (level_site) and the arithmetic under it (level_up_index, level_position, LevelRow, level_flow,
// level_corners) are memc_spynet_level.hpp's, shared with the backward unit and the fp16 / bf16 forward unit.
// per_row: lanes per output row (QUAD: W / 4, else W).  Strides in elements: f first, s second, c coarse, o out.
template <bool QUAD>
__global__ __launch_bounds__(256) void spynet_level(
    int W, int H, int w, int h, int batch, int per_row, float sy, float sx, float kx, float ky, int align_up, int align_sample,
    int64_t sfb, int64_t sfc, int sfh, int64_t ssb, int64_t ssc, int ssh, int64_t scb, int64_t scc, int sch,
    int64_t sob, int64_t soc, int soh, const float *__restrict__ first, const float *__restrict__ second,
    const float *__restrict__ coarse, float *__restrict__ out)
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
        const float *fp = first + b * sfb + (int64_t)y * sfh + x;
        const float *sb = second + b * ssb, *cb = coarse + b * scb;
        float *op = out + b * sob + (int64_t)y * soh + x;
        if constexpr (QUAD) {
            f32x4 ux, uy, wv[3];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                float u, v, t[3];
                level_site(x + j, y, W, H, w, sx, kx, ky, align_up != 0, align_sample != 0, r, cb, scc, sb, ssc, ssh, u, v, t);
                ux[j] = u;
                uy[j] = v;
#pragma unroll
                for (int c = 0; c < 3; c++) wv[c][j] = t[c];
            }
#pragma unroll
            for (int c = 0; c < 3; c++) st_cached4(op + c * soc, ld_cached4(fp + c * sfc));
#pragma unroll
            for (int c = 0; c < 3; c++) st_cached4(op + (3 + c) * soc, wv[c]);
            st_cached4(op + 6 * soc, ux);
            st_cached4(op + 7 * soc, uy);
        } else {
            float u, v, t[3];
            level_site(x, y, W, H, w, sx, kx, ky, align_up != 0, align_sample != 0, r, cb, scc, sb, ssc, ssh, u, v, t);
#pragma unroll
            for (int c = 0; c < 3; c++) op[c * soc] = fp[c * sfc];
#pragma unroll
            for (int c = 0; c < 3; c++) op[(3 + c) * soc] = t[c];
            op[6 * soc] = u;
            op[7 * soc] = v;
        }
    }
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_spynet.h)
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

// the bytes [lo, hi) a tensor's elements lie in
struct Span {
    uintptr_t lo, hi;
};
inline Span span_of(const memc_tensor4 *t)
{
    int64_t last = 0;
    for (int i = 0; i < 4; i++) last += (t->size[i] - 1) * t->stride[i];
    const uintptr_t lo = reinterpret_cast<uintptr_t>(t->data);
    return {lo, lo + (uintptr_t)(last + 1) * sizeof(float)};
}

}  // namespace

extern "C" {

const char *memc_spynet_version(void) { return "memc_hip_spynet 0.1 gfx950"; }

const char *memc_spynet_last_kernel_path(void) { return memc::t_spynet_path; }

int SpyNetLevelLayer_gpu_forward(memc_stream_t stream, const memc_tensor4 *first, const memc_tensor4 *second,
                                 const memc_tensor4 *coarse, const memc_tensor4 *out, int align_upsample, int align_sample)
{
    // malformed
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
    bool quad = W % 4 == 0 && W >= 8;
    for (const memc_tensor4 *t : {first, second, coarse, out})
        if (reinterpret_cast<uintptr_t>(t->data) % 4 != 0) quad = false;
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
                           out->stride[0], out->stride[1], (int)out->stride[2], (const float *)first->data,
                           (const float *)second->data, (const float *)coarse->data, (float *)out->data);
    };
    if (quad) {
        t_spynet_path = "spynet_level:quad";
        launch(spynet_level<true>);
    } else {
        t_spynet_path = "spynet_level:direct";
        launch(spynet_level<false>);
    }
    return launch_status();
}

}  // extern "C"
