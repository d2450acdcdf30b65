// lp_flow_projection_bwd.hip -- the backward of FlowProjectionLayer on fp16 / bf16 storage, for gfx950: a half flow, a half
// gradoutput and a half gradient beside the float32 count of the (float32) forward.  The kernel and the C ABI of
// libmemc_hip_lp_proj_grad.so (include/memc_warp_lp_proj_grad.h).
//
// This is the projection's backward of a model cast to bf16 / fp16.  Widened on the host the call is a cast pass over
// gradoutput, the fp32 kernel and a cast pass over the gradient (~48 B per site, three launches); read as they are the
// tensors are 16 B per site: flow 4 + gradoutput 4 (staged, once per tile box) + count 4 (staged) read, gradient 4 written.
//
// proj_bwd_lp_tiled RESTATES the fp32 kernel proj_bwd_tiled<false, 2496, false> (flow_projection.hip, "Backward, tiled":
// the whole kernel body -- tile walk, site location, tile_region, the staging of (gx / count, gy / count, 0, 0), the
// covered gather from LDS, the uncovered gather from global memory, the corner sums, the two stores) without the depth
// operator's and the ragged width's branches.  It is written out rather than shared as a body: the fp32 kernel stages its
// three planes through one float loader (tile_stage_load_planes<3, RAG>) where this one stages two half planes and one
// float plane, and what remains in common after DEPTH and RAG are taken out is shorter than the parameters a shared body
// would need.  The arithmetic is the fp32 kernel's in its order: 1.0f / count and gradoutput * that once per staged cell
// (the same two products for a corner gathered from global memory), the corners summed TL, TR, BL, BR as g += -q, all in
// fp32 on exactly widened inputs; each gradient element is rounded once.  So the result equals, bit for bit, the fp32
// library's on the widened inputs after one `.to(dtype)`.  No atomics, no workspace; every element is assigned.
#include "memc_common.hpp"
#include "memc_lp.hpp"
#include "memc_desc.hpp"
#include "memc_warp_lp_proj_grad.h"

namespace memc {

thread_local const char *t_lp_proj_grad_path = "";

constexpr int kProjBwdCap = 2496;          // the fp32 kernel's staging budget: 39 KiB of cells, four workgroups per CU

// T: the flow, gradoutput and the gradient (s1: their common strides); the count is fp32 (sc).
template <class T>
__global__ __launch_bounds__(256) void proj_bwd_lp_tiled(
    int W, int H, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t scb, int sch,
    const st_t<T> *__restrict__ flow, const float *__restrict__ count, const st_t<T> *__restrict__ gout,
    st_t<T> *__restrict__ gin1, int sw)
{
    constexpr int LX = 16;
    using G = TileGeom<LX, kProjBwdCap>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem);
    int *bb = reinterpret_cast<int *>(smem + G::kCapPx * 16);

    const TileCoord tc = tile_walk(blockIdx.x, gridDim.x, tiles_x, tiles_y, sw);
    if (tc.tx >= tiles_x) return;
    const int b = tc.b, tile_x0 = tc.tx * G::kTW, tile_y0 = tc.ty * G::kTH;
    const int x = tile_x0 + 4 * (threadIdx.x % LX), y = tile_y0 + threadIdx.x / LX;
    const bool inb = x < W && y < H;
    const int xs = min(x, W - 4), ys = min(y, H - 1);
    const st_t<T> *flow_p = flow + b * s1b + (int64_t)ys * s1h + xs;
    const f32x4 fx4 = ld4_stream<T>(flow_p), fy4 = ld4_stream<T>(flow_p + s1c);
    // every site owns its two gradient elements: they are STORED once (invalid sites store zero), the buffer needs no fill
    st_t<T> *g1p = gin1 + b * s1b + (int64_t)ys * s1h + xs;
    f32x4 acc_x = {0.f, 0.f, 0.f, 0.f}, acc_y = acc_x;

    BlSite st[4];
    int cmin = INT_MAX, cmax = -1, rmin = INT_MAX, rmax = -1;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        st[j] = bl_locate<false>(x + j, y, W, H, fx4[j], fy4[j]);
        st[j].valid = st[j].valid && inb;
        if (st[j].valid) {
            cmin = min(cmin, st[j].L);  cmax = max(cmax, st[j].R);
            rmin = min(rmin, st[j].T);  rmax = max(rmax, st[j].Bm);
        }
    }
    const Region r = tile_region<LX, true, kProjBwdCap>(cmin, cmax, rmin, rmax, tile_x0, tile_y0, bb);
    const st_t<T> *go = gout + b * s1b;
    const float *cn = count + b * scb;
    // the staged pixel quad is (gout_x / count, gout_y / count, 0, 0), the division done once per staged cell: gradoutput
    // as 8-byte quads of T (lp_stage_load), the count as the fp32 kernel reads it
    {
        const StageSlot sl = stage_slots(r);
        LpStageRegs<2> sg;
        StageRegs<1> sc;
        const st_t<T> *const gplanes[2] = {go, go + s1c};
        const float *const cplanes[1] = {cn};
        const int chs[1] = {sch};
        lp_stage_load<2>(r, sl, gplanes, s1h, sg);
        tile_stage_load_planes<1, false>(r, sl, cplanes, chs, sc);
#pragma unroll
        for (int it = 0; it < kStageIts; it++) {
            if (sl.row[it] < r.h) {
                f32x4 *dst = tile + sl.row[it] * r.pitch;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const float inv = 1.0f / sc.v[it][0][i];       // cells nobody projected to: inf, never read
                    const unsigned wx = i < 2 ? sg.v[it][0].x : sg.v[it][0].y, wy = i < 2 ? sg.v[it][1].x : sg.v[it][1].y;
                    const float gx = (i & 1) ? widen_hi<T>(wx) : widen_lo<T>(wx);
                    const float gy = (i & 1) ? widen_hi<T>(wy) : widen_lo<T>(wy);
                    const f32x4 px = {gx * inv, gy * inv, 0.f, 0.f};
                    dst[swz_col(4 * sl.q[it] + i)] = px;
                }
            }
        }
    }
    __syncthreads();
    if (!inb) return;

#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!st[j].valid) continue;
        const BlSite &s = st[j];
        f32x4 q[4];          // (gx / count, gy / count, 0, 0) at TL, TR, BL, BR
        if (r.covers(s.L, s.R, s.T, s.Bm)) {
            const int rT = (s.T - r.y0) * r.pitch, rB = (s.Bm - r.y0) * r.pitch;
            const int cL = swz_col(s.L - r.x0), cR = swz_col(s.R - r.x0);
            q[0] = tile[rT + cL];  q[1] = tile[rT + cR];  q[2] = tile[rB + cL];  q[3] = tile[rB + cR];
        } else {             // rare: the corner is outside the staged box
            const int o[4] = {s.T * s1h + s.L, s.T * s1h + s.R, s.Bm * s1h + s.L, s.Bm * s1h + s.R};
            const int c[4] = {s.T * sch + s.L, s.T * sch + s.R, s.Bm * sch + s.L, s.Bm * sch + s.R};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float inv = 1.0f / cn[c[k]];
                q[k] = f32x4{widen<T>(go[o[k]]) * inv, widen<T>(go[s1c + o[k]]) * inv, 0.f, 0.f};
            }
        }
        float gx = 0.0f, gy = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; k++) gx += -q[k][0];
#pragma unroll
        for (int k = 0; k < 4; k++) gy += -q[k][1];
        acc_x[j] = gx;  acc_y[j] = gy;
    }
    // the sums are fp32 values, rounded to T once: the quads go through an empty asm so that no conversion is folded into
    // the addition that produced its operand (memc_lp.hpp: narrow_f32)
    asm volatile("" : "+v"(acc_x), "+v"(acc_y));
    const u16x4 ox = {narrow<T>(acc_x[0]), narrow<T>(acc_x[1]), narrow<T>(acc_x[2]), narrow<T>(acc_x[3])};
    const u16x4 oy = {narrow<T>(acc_y[0]), narrow<T>(acc_y[1]), narrow<T>(acc_y[2]), narrow<T>(acc_y[3])};
    *reinterpret_cast<u16x4a *>(g1p) = ox;
    *reinterpret_cast<u16x4a *>(g1p + s1c) = oy;
}

template <class T>
static void launch_proj_bwd_lp_tiled(hipStream_t stream, int w, int h, int batch, const memc_tensor4 *input1,
                                     const memc_tensor4 *count, const memc_tensor4 *gradoutput, const memc_tensor4 *gradinput1)
{
    using G = TileGeom<16>;
    const int sw = kDefaultStripe;
    const int ntx = (w + G::kTW - 1) / G::kTW, nty = (h + G::kTH - 1) / G::kTH;
    hipLaunchKernelGGL(proj_bwd_lp_tiled<T>, dim3(walk_grid(ntx, nty, batch, sw)), dim3(256),
                       (tile_lds_bytes<16, kProjBwdCap>()), stream, w, h, ntx, nty, input1->stride[0], input1->stride[1],
                       (int)input1->stride[2], count->stride[0], (int)count->stride[2],
                       reinterpret_cast<const st_t<T> *>(input1->data), reinterpret_cast<const float *>(count->data),
                       reinterpret_cast<const st_t<T> *>(gradoutput->data), reinterpret_cast<st_t<T> *>(gradinput1->data), sw);
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_lp_proj_grad.h)
// ==================================================================================================
using namespace memc;

static bool count_matches(const memc_tensor4 *flow, const memc_tensor4 *count)
{
    return count->size[0] == flow->size[0] && count->size[1] == 1 && count->size[2] == flow->size[2] &&
           count->size[3] == flow->size[3];
}

extern "C" {

const char *memc_lp_proj_grad_version(void) { return "memc_hip_lp_proj_grad 0.1 gfx950"; }

const char *memc_lp_proj_grad_last_kernel_path(void) { return memc::t_lp_proj_grad_path; }

int FlowProjectionLayer_gpu_backward_lp(memc_stream_t stream, memc_dtype payload, const memc_tensor4 *input1,
                                        const memc_tensor4 *count, const memc_tensor4 *gradoutput,
                                        const memc_tensor4 *gradinput1)
{
    // malformed (-1), the checks of FlowProjectionLayer_gpu_backward (layer_api.cpp) in its order
    if (payload != MEMC_F16 && payload != MEMC_BF16) return -1;
    if (!ok(input1) || !ok(count) || !ok(gradoutput) || !ok(gradinput1)) return -1;
    if (input1->size[1] != 2) return -1;
    if (!count_matches(input1, count)) return -1;
    if (!same_layout(input1, gradinput1)) return -1;
    if (!same_layout(input1, gradoutput)) return -1;
    // empty (0)
    const int n = (int)input1->size[0], h = (int)input1->size[2], w = (int)input1->size[3];
    if (n == 0 || h == 0 || w == 0) return 0;
    // coverage: whole 8-byte quads of T, at least two per row; a dword-aligned count; 32-bit in-plane offsets
    if (!(w % 4 == 0 && w >= 8 && quad_ok(input1) && quad_ok(gradoutput) && quad_ok(gradinput1) &&
          reinterpret_cast<uintptr_t>(count->data) % 4 == 0 &&
          plane_fits_u32(w, h, {(long)input1->stride[2], (long)count->stride[2]})))
        return 1;
    t_lp_proj_grad_path = "proj_bwd_lp:tiled";
    if (payload == MEMC_F16)
        launch_proj_bwd_lp_tiled<F16>((hipStream_t)stream, w, h, n, input1, count, gradoutput, gradinput1);
    else
        launch_proj_bwd_lp_tiled<BF16>((hipStream_t)stream, w, h, n, input1, count, gradoutput, gradinput1);
    return launch_status();
}

}  // extern "C"
