// lp_depth_flow_projection_bwd.hip -- the backward of DepthFlowProjectionLayer on fp16 / bf16 storage, for gfx950: a half
// flow, depth, gradoutput and two half gradients beside the float32 count and the float32 output of the (float32) forward.
// The kernel and the C ABI of libmemc_hip_lp_dproj_grad.so (include/memc_warp_lp_dproj_grad.h).
//
// This is the depth-weighted projection's backward of a model cast to bf16 / fp16.  Widened on the host the call is a cast
// pass over gradoutput, the fp32 kernel and two cast passes over the gradients (~74 B per site, four launches); read as they
// are the tensors are 28 B per site: flow 4 + depth 2 + gradoutput 4 (staged, once per tile box) + count 4 + forward output 8
// (staged) read, gradinput1 4 + gradinput2 2 written.
//
// dproj_bwd_lp_tiled RESTATES the fp32 kernel proj_bwd_tiled<true, 2496, false> (flow_projection.hip, "Backward, tiled": the
// whole kernel body -- tile walk, site location, tile_region, the staging of (gx / count, gy / count, out_x, out_y), the
// covered gather from LDS, the uncovered gather from global memory, the corner sums, the three stores) without the ragged
// width's branches, as lp_flow_projection_bwd.hip restates the DEPTH = false instantiation; it is written out rather than
// shared as a body for the same reason (the fp32 kernel stages its five planes through one float loader, this one two half
// planes and three float planes).  The arithmetic is the fp32 kernel's in its order: 1.0f / count and gradoutput * that
// once per staged cell (the same two products for a corner gathered from global memory), then per site over the corners
// TL, TR, BL, BR  gx += -qx * d,  gy += -qy * d,  gd += -qx * (fx - ox),  gd += -qy * (fy - oy), all in fp32 on exactly
// widened inputs; each gradient element is rounded once.  The fp32 unit's device code keeps every one of those products
// apart from the sum it goes into (its products are packed in pairs, the sums are scalar: nothing is contracted), so the
// site arithmetic is spelled unfused here (site_sums: contraction off) whatever the compiler would choose for this unit.
// So the result equals, bit for bit, the fp32 library's on the widened inputs after one `.to(dtype)`.  No atomics, no
// workspace; every element is assigned.
#include "memc_common.hpp"
#include "memc_lp.hpp"
#include "memc_desc.hpp"
#include "memc_warp_lp_dproj_grad.h"

namespace memc {

thread_local const char *t_lp_dproj_grad_path = "";

constexpr int kProjBwdCap = 2496;          // the fp32 kernel's staging budget: 39 KiB of cells, four workgroups per CU

// One site's three sums over its corners q[k] = (gx / count, gy / count, out_x, out_y), k = TL, TR, BL, BR: every product
// rounded to fp32 before it is added, as the fp32 kernel's device code has it.
__device__ __forceinline__ void site_sums(const f32x4 (&q)[4], float fx, float fy, float d, float &gx, float &gy, float &gd)
{
#pragma clang fp contract(off)
    gx = 0.0f;  gy = 0.0f;  gd = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) gx += -q[k][0] * d;
#pragma unroll
    for (int k = 0; k < 4; k++) gy += -q[k][1] * d;
#pragma unroll
    for (int k = 0; k < 4; k++) gd += -q[k][0] * (fx - q[k][2]);
#pragma unroll
    for (int k = 0; k < 4; k++) gd += -q[k][1] * (fy - q[k][3]);
}

// T: the flow, gradoutput and gradinput1 (s1: their common strides; the fp32 forward output is indexed with them too), the
// depth and gradinput2 (sd); the count is fp32 (sc).
template <class T>
__global__ __launch_bounds__(256) void dproj_bwd_lp_tiled(
    int W, int H, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t sdb, int sdh, int64_t scb, int sch,
    const st_t<T> *__restrict__ flow, const st_t<T> *__restrict__ depth, const float *__restrict__ count,
    const float *__restrict__ fwd_out, const st_t<T> *__restrict__ gout,
    st_t<T> *__restrict__ gin1, st_t<T> *__restrict__ gin2, int sw)
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
    const f32x4 d4 = ld4_stream<T>(depth + b * sdb + (int64_t)ys * sdh + xs);
    // every site owns its three gradient elements: they are STORED once (invalid sites store zero), the buffers need no fill
    st_t<T> *g1p = gin1 + b * s1b + (int64_t)ys * s1h + xs;
    st_t<T> *g2p = gin2 + b * sdb + (int64_t)ys * sdh + xs;
    f32x4 acc_x = {0.f, 0.f, 0.f, 0.f}, acc_y = acc_x, acc_d = acc_x;

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
    const float *cn = count + b * scb, *fo = fwd_out + b * s1b;
    // the staged pixel quad is (gout_x / count, gout_y / count, out_x, out_y), the division done once per staged cell:
    // gradoutput as 8-byte quads of T (lp_stage_load), the count and the forward output as the fp32 kernel reads them
    {
        const StageSlot sl = stage_slots(r);
        LpStageRegs<2> sg;
        StageRegs<3> sc;
        const st_t<T> *const gplanes[2] = {go, go + s1c};
        const float *const cplanes[3] = {cn, fo, fo + s1c};
        const int chs[3] = {sch, s1h, s1h};
        lp_stage_load<2>(r, sl, gplanes, s1h, sg);
        tile_stage_load_planes<3, false>(r, sl, cplanes, chs, sc);
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
                    const f32x4 px = {gx * inv, gy * inv, sc.v[it][1][i], sc.v[it][2][i]};
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
        f32x4 q[4];          // (gx / count, gy / count, ox, oy) at TL, TR, BL, BR
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
                q[k] = f32x4{widen<T>(go[o[k]]) * inv, widen<T>(go[s1c + o[k]]) * inv, fo[o[k]], fo[s1c + o[k]]};
            }
        }
        float gx, gy, gd;
        site_sums(q, fx4[j], fy4[j], d4[j], gx, gy, gd);
        acc_x[j] = gx;  acc_y[j] = gy;  acc_d[j] = gd;
    }
    // the sums are fp32 values, rounded to T once: the quads go through an empty asm so that no conversion is folded into
    // the addition that produced its operand (memc_lp.hpp: narrow_f32)
    asm volatile("" : "+v"(acc_x), "+v"(acc_y), "+v"(acc_d));
    const u16x4 ox = {narrow<T>(acc_x[0]), narrow<T>(acc_x[1]), narrow<T>(acc_x[2]), narrow<T>(acc_x[3])};
    const u16x4 oy = {narrow<T>(acc_y[0]), narrow<T>(acc_y[1]), narrow<T>(acc_y[2]), narrow<T>(acc_y[3])};
    const u16x4 od = {narrow<T>(acc_d[0]), narrow<T>(acc_d[1]), narrow<T>(acc_d[2]), narrow<T>(acc_d[3])};
    *reinterpret_cast<u16x4a *>(g1p) = ox;
    *reinterpret_cast<u16x4a *>(g1p + s1c) = oy;
    *reinterpret_cast<u16x4a *>(g2p) = od;
}

struct DprojBwdLpCall {
    const memc_tensor4 *input1, *input2, *count, *output, *gradoutput, *gradinput1, *gradinput2;
};

template <class T>
static void launch_dproj_bwd_lp_tiled(hipStream_t stream, int w, int h, int batch, const DprojBwdLpCall &k)
{
    using G = TileGeom<16>;
    const int sw = kDefaultStripe;
    const int ntx = (w + G::kTW - 1) / G::kTW, nty = (h + G::kTH - 1) / G::kTH;
    hipLaunchKernelGGL(dproj_bwd_lp_tiled<T>, dim3(walk_grid(ntx, nty, batch, sw)), dim3(256),
                       (tile_lds_bytes<16, kProjBwdCap>()), stream, w, h, ntx, nty, k.input1->stride[0], k.input1->stride[1],
                       (int)k.input1->stride[2], k.input2->stride[0], (int)k.input2->stride[2], k.count->stride[0],
                       (int)k.count->stride[2], reinterpret_cast<const st_t<T> *>(k.input1->data),
                       reinterpret_cast<const st_t<T> *>(k.input2->data), reinterpret_cast<const float *>(k.count->data),
                       reinterpret_cast<const float *>(k.output->data), reinterpret_cast<const st_t<T> *>(k.gradoutput->data),
                       reinterpret_cast<st_t<T> *>(k.gradinput1->data), reinterpret_cast<st_t<T> *>(k.gradinput2->data), sw);
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_lp_dproj_grad.h)
// ==================================================================================================
using namespace memc;

static bool count_matches(const memc_tensor4 *flow, const memc_tensor4 *count)
{
    return count->size[0] == flow->size[0] && count->size[1] == 1 && count->size[2] == flow->size[2] &&
           count->size[3] == flow->size[3];
}

static bool dword_aligned(const memc_tensor4 *t) { return reinterpret_cast<uintptr_t>(t->data) % 4 == 0; }

extern "C" {

const char *memc_lp_dproj_grad_version(void) { return "memc_hip_lp_dproj_grad 0.1 gfx950"; }

const char *memc_lp_dproj_grad_last_kernel_path(void) { return memc::t_lp_dproj_grad_path; }

int DepthFlowProjectionLayer_gpu_backward_lp(memc_stream_t stream, memc_dtype payload, const memc_tensor4 *input1,
                                             const memc_tensor4 *input2, const memc_tensor4 *count,
                                             const memc_tensor4 *output, const memc_tensor4 *gradoutput,
                                             const memc_tensor4 *gradinput1, const memc_tensor4 *gradinput2)
{
    // malformed (-1), the checks of DepthFlowProjectionLayer_gpu_backward (layer_api.cpp) in its order
    if (payload != MEMC_F16 && payload != MEMC_BF16) return -1;
    if (!ok(input1) || !ok(input2) || !ok(count) || !ok(output) || !ok(gradoutput) || !ok(gradinput1) || !ok(gradinput2))
        return -1;
    if (input1->size[1] != 2) return -1;
    if (input2->size[1] != 1) return -1;
    if (!count_matches(input1, input2) || !count_matches(input1, count)) return -1;
    if (!same_layout(input1, gradinput1)) return -1;
    if (!same_layout(input1, gradoutput) || !same_layout(input1, output)) return -1;
    if (!same_layout(input2, gradinput2)) return -1;
    // empty (0)
    const int n = (int)input1->size[0], h = (int)input1->size[2], w = (int)input1->size[3];
    if (n == 0 || h == 0 || w == 0) return 0;
    // coverage: whole 8-byte quads of T, at least two per row; a dword-aligned count and output; 32-bit in-plane offsets
    if (!(w % 4 == 0 && w >= 8 && quad_ok(input1) && quad_ok(input2) && quad_ok(gradoutput) && quad_ok(gradinput1) &&
          quad_ok(gradinput2) && dword_aligned(count) && dword_aligned(output) &&
          plane_fits_u32(w, h, {(long)input1->stride[2], (long)input2->stride[2], (long)count->stride[2]})))
        return 1;
    t_lp_dproj_grad_path = "dproj_bwd_lp:tiled";
    const DprojBwdLpCall k = {input1, input2, count, output, gradoutput, gradinput1, gradinput2};
    if (payload == MEMC_F16)
        launch_dproj_bwd_lp_tiled<F16>((hipStream_t)stream, w, h, n, k);
    else
        launch_dproj_bwd_lp_tiled<BF16>((hipStream_t)stream, w, h, n, k);
    return launch_status();
}

}  // extern "C"
