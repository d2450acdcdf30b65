// spynet_level_bwd.hip -- the gradient of one SPyNet pyramid level's input with respect to the coarse flow, in fp32, for
// gfx950: the kernel and the C ABI of libmemc_hip_spynet_grad.so (include/memc_spynet_grad.h).
//
// SPyNet's frames are data: of the level's three inputs only the coarse flow, which comes out of the previous level's
// convolutions, wants a gradient.  (A gradient for `first` is a slice of gradoutput; `second` gets none.)  So there is no
// image gradient, no scatter and no atomics.  Composed from ATen it is about twenty launches per level and direction.
//
// One kernel, spynet_level_bwd_tiled: 256 lanes, a workgroup owns a tile of kTile x kTile coarse cells.
//   Phase 1  the lanes compute, for every fine site of the tile's footprint, the gradient (gux, guy) that reaches the
//            upsampled flow `up` there -- G[6:8] plus the warp's derivative along x and y, the site arithmetic being the
//            forward's own (memc_spynet_level.hpp) -- into LDS.
//   Phase 2  after ONE barrier lane t owns coarse cell (t / kTile, t % kTile) of the tile and sums the adjoint of the x2
//            upsampling over the cell's candidate sites from LDS, rows outer, columns inner: a fixed order, so the result
//            repeats its bits from run to run.  Each weight is level_up_index's, kept only where its index is the cell's.
//
// The footprint.  Coarse cell i has a weight at the unpadded fine index y' (y' = min(y, 2n - 1): a padded row or column
// repeats the last) only where level_up_index(y') yields i0 == i or i1 == i, that is where floor(src(y')) is i - 1 or i.
//   without align_upsample: src = max(y' / 2 - 1 / 4, 0) exactly, so y' lies in [2i - 1, 2i + 2]; the cells [i0, i1) take
//       the fine rows [2 i0 - 1, 2 i1], at most 2 (i1 - i0) + 2 of them;
//   under align_upsample: src = y' (n - 1) / (2n - 1) to within fp32 rounding, so y' lies in [(i - 1) q, (i + 1) q) with
//       q = (2n - 1) / (n - 1); the candidate range of the cells [i0, i1) is [floor((i0 - 1) q), ceil(i1 q)], in integers:
//       up to one site too generous at either end, which also covers the rounding of src (one site moves src by about a
//       half, its rounding error is below n * 2^-22); a site whose index does not match has weight 0.
//   either way the range is clipped to [0, 2n - 1] and, where it reaches 2n - 1, extended to the last fine row N - 1 (the
//   padded one, if there is one).
// The bound of the staged box (level_box_bound below, restated by tests/_spynet_grad_spec.footprint): an axis with at most
// kTile coarse cells has at most 2 kTile + 1 fine sites altogether.  Otherwise n >= kTile + 1 and, both ends being
// multiples of 1 / (n - 1), ceil(i1 q) - floor((i0 - 1) q) + 1 <= (i1 - i0 + 1) q + 2 (n - 2) / (n - 1) + 1
// < 2 (kTile + 1) + (kTile + 1) / (n - 1) + 3, hence at most 2 kTile + 4 + ceil((kTile + 1) / (n - 1)) <= 2 kTile + 6 sites,
// and one more for a padded row: kBox = 2 kTile + 7 bounds both modes.  The LDS array is sized by it and the host refuses to
// launch if a tile could exceed it.
//
// Tile size: 16 x 16.  One coarse cell per lane in phase 2; the footprint of 34 x 34 sites (without align_upsample)
// recomputes 13 % of the sites for its halo against 27 % for 8 x 8 tiles; 2 x 39 x 39 floats are 12 KiB of LDS, so LDS
// never limits the workgroups per CU.  Not measured against other sizes.
//
// Safety: as in the forward, the position is clamped into [-2, W + 1] x [-2, H + 1] by comparisons that send a NaN to -2
// BEFORE any conversion to int, and every corner is read at an index clamped into the image and selected, not multiplied,
// by its in-range test: no flow value, however large or non-finite, forms an address outside `second`.  The coarse indices
// come from level_up_index of a site index, never from data; the LDS offsets from the box, which the host bounds.
#include "memc_common.hpp"
#include "memc_desc.hpp"
#include "memc_spynet_level.hpp"
#include "memc_spynet_grad.h"

#include <initializer_list>

namespace memc {

thread_local const char *t_spynet_grad_path = "";

constexpr int kTile = 16;                      // coarse cells per tile side: kTile * kTile == 256 lanes
constexpr int kBox = 2 * kTile + 7;            // fine sites per side of the staged box, both modes (derived above)
constexpr int kPitch = kBox;                   // odd: the rows of a cell's candidates start in different banks

// The candidate range [lo, hi] of fine indices (of N, N in {2n, 2n + 1}) for the coarse cells [i0, i1) of n.  Host and
// device; tests/_spynet_grad_spec.footprint restates it.
__host__ __device__ inline void level_footprint(int i0, int i1, int n, int N, bool align, int &lo, int &hi)
{
    const int last = 2 * n - 1;
    int a, b;
    if (!align) {
        a = 2 * i0 - 1;
        b = 2 * i1;
    } else if (n == 1) {
        a = 0;
        b = last;
    } else {
        const int64_t num = 2 * (int64_t)n - 1, den = n - 1;
        a = i0 >= 1 ? (int)(((i0 - 1) * num) / den) : 0;
        const int64_t top = (i1 * num + den - 1) / den;
        b = top < last ? (int)top : last;
    }
    lo = a > 0 ? a : 0;
    hi = b >= last ? N - 1 : b;
}

// An upper bound of hi - lo + 1 over every tile of kTile cells (derived above)
inline int level_box_bound(int n, int N, bool align)
{
    if (n <= kTile) return N;
    if (!align) return 2 * kTile + 2;
    return 2 * kTile + 4 + (kTile + 1 + n - 2) / (n - 1) + (N - 2 * n);
}

// the weight of coarse index i at the fine index d (already unpadded): level_up_index's, kept where the index matches
__device__ __forceinline__ float level_adjoint_weight(int d, int i, int n, float scale, bool align)
{
    int i0, i1;
    float l0, l1;
    level_up_index(d, n, scale, align, i0, i1, l0, l1);
    return (i0 == i ? l0 : 0.0f) + (i1 == i ? l1 : 0.0f);
}

// Strides in elements: s second, c coarse, g gradoutput, q gradcoarse.  kxs, kys: kx', ky' (1 under align_sample).
__global__ __launch_bounds__(256) void spynet_level_bwd_tiled(
    int W, int H, int w, int h, int batch, int tiles_x, float sy, float sx, float kx, float ky, float kxs, float kys,
    int align_up, int align_sample, int64_t ssb, int64_t ssc, int ssh, int64_t scb, int64_t scc, int sch, int64_t sgb,
    int64_t sgc, int sgh, int64_t sqb, int64_t sqc, int sqh, const float *__restrict__ second,
    const float *__restrict__ coarse, const float *__restrict__ gout, float *__restrict__ gcoarse)
{
    __shared__ float gu[2][kBox * kPitch];
    const int tid = (int)threadIdx.x;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int i0 = ty * kTile, j0 = tx * kTile;
    const int i1 = min(i0 + kTile, h), j1 = min(j0 + kTile, w);
    const bool au = align_up != 0, as = align_sample != 0;
    int ylo, yhi, xlo, xhi;
    level_footprint(i0, i1, h, H, au, ylo, yhi);
    level_footprint(j0, j1, w, W, au, xlo, xhi);
    const int nby = min(yhi - ylo + 1, kBox), nbx = min(xhi - xlo + 1, kBox);      // the host has refused a larger box
    // phase 2's cell and its candidate range, inside the box
    const int ci = i0 + tid / kTile, cj = j0 + tid % kTile;
    const bool owner = ci < i1 && cj < j1;
    int cy0 = 0, cy1 = -1, cx0 = 0, cx1 = -1;
    if (owner) {
        level_footprint(ci, ci + 1, h, H, au, cy0, cy1);
        level_footprint(cj, cj + 1, w, W, au, cx0, cx1);
        cy0 = max(cy0, ylo), cy1 = min(cy1, ylo + nby - 1);
        cx0 = max(cx0, xlo), cx1 = min(cx1, xlo + nbx - 1);
    }
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const float *sb = second + b * ssb, *cb = coarse + b * scb, *gb = gout + b * sgb;
        // phase 1: (gux, guy) of every site of the box
        for (int s = tid; s < nby * nbx; s += 256) {
            const int yy = s / nbx, xx = s - yy * nbx;
            const int y = ylo + yy, x = xlo + xx;
            LevelRow r;
            {
                int y0, y1;
                level_up_index(min(y, 2 * h - 1), h, sy, au, y0, y1, r.l0, r.l1);      // a padded row repeats row 2h - 1
                r.o0 = y0 * sch;
                r.o1 = y1 * sch;
            }
            float ux, uy;
            level_flow(x, w, sx, au, r, cb, scc, ux, uy);
            const float px = level_position(x, ux, W, kx, as), py = level_position(y, uy, H, ky, as);
            const LevelCorners k = level_corners(px, py, W, H, ssh);
            const float *gp = gb + (int64_t)y * sgh + x;
            float dx = 0.0f, dy = 0.0f;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float *p = sb + c * ssc;
                const float nw = k.inx0 && k.iny0 ? p[k.r0 + k.cx0] : 0.0f, ne = k.inx1 && k.iny0 ? p[k.r0 + k.cx1] : 0.0f;
                const float sw = k.inx0 && k.iny1 ? p[k.r1 + k.cx0] : 0.0f, se = k.inx1 && k.iny1 ? p[k.r1 + k.cx1] : 0.0f;
                const float g = gp[(3 + c) * sgc];
                dx += g * (k.by * (ne - nw) + k.ay * (se - sw));
                dy += g * (k.bx * (sw - nw) + k.ax * (se - ne));
            }
            gu[0][yy * kPitch + xx] = gp[6 * sgc] + kxs * dx;
            gu[1][yy * kPitch + xx] = gp[7 * sgc] + kys * dy;
        }
        __syncthreads();
        // phase 2: the adjoint of the upsampling, rows outer, columns inner
        if (owner) {
            float acc0 = 0.0f, acc1 = 0.0f;
            for (int y = cy0; y <= cy1; y++) {
                const float wy = level_adjoint_weight(min(y, 2 * h - 1), ci, h, sy, au);
                const int o = (y - ylo) * kPitch - xlo;
                float row0 = 0.0f, row1 = 0.0f;
                for (int x = cx0; x <= cx1; x++) {
                    const float wx = level_adjoint_weight(min(x, 2 * w - 1), cj, w, sx, au);
                    row0 += wx * gu[0][o + x];
                    row1 += wx * gu[1][o + x];
                }
                acc0 += wy * row0;
                acc1 += wy * row1;
            }
            float *qp = gcoarse + b * sqb + (int64_t)ci * sqh + cj;
            qp[0] = 2.0f * acc0;
            qp[sqc] = 2.0f * acc1;
        }
        __syncthreads();                       // the next batch element's phase 1 overwrites the box
    }
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_spynet_grad.h)
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

const char *memc_spynet_grad_version(void) { return "memc_hip_spynet_grad 0.1 gfx950"; }

const char *memc_spynet_grad_last_kernel_path(void) { return memc::t_spynet_grad_path; }

int SpyNetLevelLayer_gpu_backward(memc_stream_t stream, const memc_tensor4 *second, const memc_tensor4 *coarse,
                                  const memc_tensor4 *gradoutput, const memc_tensor4 *gradcoarse, int align_upsample,
                                  int align_sample)
{
    // malformed
    if (!usable(second) || !usable(coarse) || !usable(gradoutput) || !usable(gradcoarse)) return kErr;
    const int64_t B = second->size[0], H = second->size[2], W = second->size[3], h = coarse->size[2], w = coarse->size[3];
    if (!shaped(second, B, 3, H, W) || !shaped(coarse, B, 2, h, w) || !shaped(gradoutput, B, 8, H, W) ||
        !shaped(gradcoarse, B, 2, h, w))
        return kErr;
    if (H < 2 || W < 2 || (H != 2 * h && H != 2 * h + 1) || (W != 2 * w && W != 2 * w + 1)) return kErr;
    // empty
    if (B == 0) return 0;
    // not covered
    for (const memc_tensor4 *t : {second, coarse, gradoutput, gradcoarse})
        if (t->size[3] > 1 && t->stride[3] != 1) return kNotCovered;
    for (const memc_tensor4 *t : {second, coarse, gradoutput, gradcoarse})
        if ((t->size[2] - 1) * t->stride[2] + t->size[3] > INT32_MAX) return kNotCovered;
    const Span so = span_of(gradcoarse);
    for (const memc_tensor4 *t : {second, coarse, gradoutput}) {
        const Span s = span_of(t);
        if (so.lo < s.hi && s.lo < so.hi) return kNotCovered;
    }
    // the staged box must hold every tile's footprint (it does for every size: kBox is the derived bound)
    if (level_box_bound((int)h, (int)H, align_upsample != 0) > kBox || level_box_bound((int)w, (int)W, align_upsample != 0) > kBox)
        return kErr;
    // ATen's scales, as the forward has them
    const float sy = align_upsample ? (h > 1 ? (float)(h - 1) / (float)(2 * h - 1) : 0.0f) : 0.5f;
    const float sx = align_upsample ? (w > 1 ? (float)(w - 1) / (float)(2 * w - 1) : 0.0f) : 0.5f;
    const float kx = (float)W / (float)(W - 1), ky = (float)H / (float)(H - 1);
    const float kxs = align_sample ? 1.0f : kx, kys = align_sample ? 1.0f : ky;
    const int64_t tiles_x = (w + kTile - 1) / kTile, tiles_y = (h + kTile - 1) / kTile;
    if (tiles_x * tiles_y > INT32_MAX) return kNotCovered;
    t_spynet_grad_path = "spynet_level_bwd:tiled";
    hipLaunchKernelGGL(spynet_level_bwd_tiled, dim3((unsigned)(tiles_x * tiles_y), (unsigned)(B < 65535 ? B : 65535)), dim3(256),
                       0, (hipStream_t)stream, (int)W, (int)H, (int)w, (int)h, (int)B, (int)tiles_x, sy, sx, kx, ky, kxs, kys,
                       align_upsample, align_sample, second->stride[0], second->stride[1], (int)second->stride[2],
                       coarse->stride[0], coarse->stride[1], (int)coarse->stride[2], gradoutput->stride[0],
                       gradoutput->stride[1], (int)gradoutput->stride[2], gradcoarse->stride[0], gradcoarse->stride[1],
                       (int)gradcoarse->stride[2], (const float *)second->data, (const float *)coarse->data,
                       (const float *)gradoutput->data, (float *)gradcoarse->data);
    return launch_status();
}

}  // extern "C"
