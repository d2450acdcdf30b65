// fi_blend_bwd_c3.hip -- the backward of ONE direction of the dual warp + occlusion blend
//     out = occ0 * FI(frame0, flow0, taps0) + occ1 * FI(frame2, flow1, taps1)
// for callers that do not want the image gradient (the frames are data: networks/MEMC_Net_star.py:266-277), RGB, fs == 4,
// fp32, for gfx950: the kernel and the C ABI of libmemc_hip_blend_grad.so (include/memc_warp_blend_grad.h).
//
// fi_blend_bwd_c3 is fi_bwd_c3_pk<false, 256, 2> (fi_bwd_c3.hip, fi_bwd_c3_body.inc with PART == 2: no packed planes, the
// staged image and phase 1 only) with the occlusion folded in.  Per tap k of a site that kernel forms
//     s_k = sum_c gout_c * pix_c(k),   t_k = w_k * s_k            (t_k: the warp's tap gradient)
// and the gradients are linear in gradoutput, so on the RAW gradoutput
//     grad_taps[k] = occ * t_k,   grad_flow = occ * (gx, gy),   grad_occ = sum_k tap_k * t_k  (= sum_c gout_c * warped_c).
// A site whose target lies outside the image: zero tap and flow gradients, grad_occ = sum_c gout_c * in_c (the forward
// copies the input pixel there).
// Over PART 2: one more input plane (occ), one more output plane, two more f32x4 per lane, no atomics.  What the host
// composition around the warp's entry points did per direction -- a forward warp written and read back, gout * warped
// summed over the channels, gout * occ written, a zero-filled image gradient, the whole backward -- is this one pass.
// Same tile machinery and geometry as the PART 2 path (64 x 16 sites per workgroup, 3072 staged pixel quads, kMaxBands
// bands): tests/_lowp_paths.py::census describes this kernel's in-kernel paths too.
// Every element of the three outputs is assigned; the results are a pure function of the inputs.
#include "memc_common.hpp"
#include "memc_fi_bwd_c3.hpp"
#include "memc_fi_abi.hpp"
#include "memc_warp_blend_grad.h"

namespace memc {

thread_local const char *t_blend_grad_path = "";

// One direction of the blend's backward.  s1: the image and gradoutput; s2: the flow and its gradient; s3: the taps and
// their gradient; s4: the occlusion and its gradient (one channel: no channel stride).
struct FiBlendBwdCall {
    hipStream_t stream;
    int w, h, batch;
    Plane s1, s2, s3, s4;
    const float *in1, *flow, *filt, *occ, *gout;
    float *gflow, *gfilt, *gocc;
};

// fi_bwd_phase1 (memc_fi_bwd_c3.hpp) for the blend: quads whose four sites the band covers.  Same loop order and the same
// laundering -- read the comments there before rearranging anything: the nest lives on staying clear of spills.
__device__ __forceinline__ void fi_blend_bwd_phase1(const Region &r, unsigned fast, FiSite4 &g, f32x4 (&tp)[16],
                                                    const f32x4 (&go)[3], const f32x4 &oc, const f32x4 *tile, int W, int H,
                                                    float *gflow_b, int64_t s2c, unsigned o2, float *gfilt_b, int64_t s3c,
                                                    unsigned o3, float *gocc_b, unsigned o4)
{
    MEMC_FI_LAUNDER(tp, g);                    // inside the caller's band loop
    if (fast != 0xFu) return;                  // mixed quads: site by site (fi_blend_bwd_site)
    f32x4 gx4 = {0.f, 0.f, 0.f, 0.f}, gy4 = gx4, gc4 = gx4;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int ro[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            asm volatile("" : "+v"(g.ix[j]));
            ro[j] = (clampi(g.iy[j] - 1 + k, H - 1) - r.y0) * r.pitch;
        }
#pragma unroll
        for (int m = 0; m < 4; m++) {
            f32x4 gt;                          // gt[j]: the warp's gradient of tap (k, m) of site j
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float a = g.a[j], bt = g.b[j];
                const int co = swz_col(clampi(g.ix[j] - 1 + m, W - 1) - r.x0);
                const f32x4 pix = tile[ro[j] + co];
                float sv = 0.0f;
                sv += go[0][j] * pix[0];  sv += go[1][j] * pix[1];  sv += go[2][j] * pix[2];
                const float wa = m < 2 ? (1 - a) : a, wb = k < 2 ? (1 - bt) : bt;
                gt[j] = (wa * wb) * sv;
                const float st = sv * tp[k * 4 + m][j];
                gx4[j] += (m < 2 ? -wb : wb) * st;
                gy4[j] += (k < 2 ? -wa : wa) * st;
                gc4[j] += gt[j] * tp[k * 4 + m][j];
            }
            st4_stream_u<F32>(gfilt_b + (k * 4 + m) * s3c, o3, oc * gt);
        }
    }
    st4_stream_u<F32>(gflow_b, o2, oc * gx4);
    st4_stream_u<F32>(gflow_b + s2c, o2, oc * gy4);
    st4_stream_u<F32>(gocc_b, o4, gc4);
}

// The three gradients of ONE site straight from global memory (fi_bwd_site_taps of memc_fi.hpp with the occlusion): mixed
// quads and sites that no band covers.  An invalid site keeps what fi_blend_bwd_store_invalid stored.
__device__ __noinline__ void fi_blend_bwd_site(int x, int y, int W, int H, const float *in_b, int64_t s1c, int s1h,
                                               const float *flow_p, float *g2, int64_t s2c, const float *tap_p, float *g3,
                                               int64_t s3c, const float *gout_p, const float *occ_p, float *gocc_p)
{
    const FiSite s = fi_locate(x, y, W, H, flow_p[0], flow_p[s2c]);
    if (!s.valid) return;
    const float g0 = gout_p[0], g1 = gout_p[s1c], gc2 = gout_p[2 * s1c], oc = occ_p[0];
    float gx = 0.0f, gy = 0.0f, gc = 0.0f;
    for (int k = 0; k < 4; k++) {
        const float *row = in_b + (int64_t)clampi(s.iy - 1 + k, H - 1) * s1h;
        for (int m = 0; m < 4; m++) {
            const float *p = row + clampi(s.ix - 1 + m, W - 1);
            float sv = 0.0f;
            sv += g0 * p[0];  sv += g1 * p[s1c];  sv += gc2 * p[2 * s1c];
            const float wa = m < 2 ? (1 - s.a) : s.a, wb = k < 2 ? (1 - s.b) : s.b;
            const float gt = (wa * wb) * sv, tap = tap_p[(k * 4 + m) * s3c];
            g3[(k * 4 + m) * s3c] = oc * gt;
            const float st = sv * tap;
            gx += (m < 2 ? -wb : wb) * st;
            gy += (k < 2 ? -wa : wa) * st;
            gc += gt * tap;
        }
    }
    g2[0] = oc * gx;
    g2[s2c] = oc * gy;
    gocc_p[0] = gc;
}

// A quad that contains an invalid site first stores its 16 + 2 + 1 float4: zeros to the tap and flow gradients
// (fi_bwd_zero_invalid), and to the occlusion gradient, per site, 0 where the site is valid and sum_c gout_c * in_c(x, y)
// where it is not -- the forward copies the input pixel at a site whose target lies outside the image, so that is what
// the occlusion multiplies there.  The quad's valid sites are then stored site by site by the same lane, and therefore
// after these.
__device__ __forceinline__ void fi_blend_bwd_store_invalid(bool inb, unsigned valid, const f32x4 (&go)[3], const float *in_b,
                                                           int64_t s1c, unsigned o1, float *gflow_b, int64_t s2c,
                                                           unsigned o2, float *gfilt_b, int64_t s3c, unsigned o3,
                                                           float *gocc_b, unsigned o4)
{
    fi_bwd_zero_invalid<F32, F32>(inb, valid, gflow_b, s2c, o2, gfilt_b, s3c, o3);
    if (!inb || valid == 0xFu) return;         // rare (image borders, |flow| guard): ordinary 64-bit addressing
    const float *p = in_b + o1 / 4u;
    f32x4 gc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; c++) gc += go[c] * *reinterpret_cast<const f32x4u *>(p + c * s1c);
#pragma unroll
    for (int j = 0; j < 4; j++) gc[j] = ((valid >> j) & 1u) ? 0.0f : gc[j];
    *reinterpret_cast<f32x4u *>(gocc_b + o4 / 4u) = gc;
}

// One 64 x NT / 16 tile of sites per workgroup, one direction per launch; 48 KiB of LDS: the staged image (3072 pixel
// quads) and the box words.  Serial chain of a tile: load -> box -> stage -> phase 1: two barriers.  W % 4 == 0, W >= 8.
template <int NT = 256>
__global__ __launch_bounds__(NT, 2) void fi_blend_bwd_c3(
    int W, int H, int tiles_x, int tiles_y, int batch,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    int64_t s4b, int s4h,
    const float *__restrict__ in1, const float *__restrict__ flow, const float *__restrict__ filt,
    const float *__restrict__ occ, const float *__restrict__ gout, float *__restrict__ gflow,
    float *__restrict__ gfilt, float *__restrict__ gocc)
{
    constexpr int LX = 16;
    using PG = PkGeomT<NT>;
    using G = TileGeom<LX, PG::kCap, NT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem);
    int *bb = reinterpret_cast<int *>(smem + PG::kImageBytes);           // 16 ints: the waves' boxes

    const TileCoord tc = strip_walk(blockIdx.x, gridDim.x, tiles_x, tiles_y, batch);
    const int b = tc.b;
    const unsigned tid = tid_now();
    const int x = tc.tx * G::kTW + 4 * (int)(tid % LX), y = tc.ty * G::kTH + (int)(tid / LX);
    const bool inb = x < W && y < H;
    const int xs = min(x, W - 4), ys = min(y, H - 1);
    const float *in_b = in1 + b * s1b;
    const float *flow_b = flow + b * s2b;
    const float *filt_b = filt + b * s3b;
    const float *occ_b = occ + b * s4b;
    const float *gout_b = gout + b * s1b;
    float *gflow_b = gflow + b * s2b;
    float *gfilt_b = gfilt + b * s3b;
    float *gocc_b = gocc + b * s4b;
    // byte offsets of the lane's quad in the planes of the four layouts
    const unsigned o1 = 4u * (unsigned)(ys * s1h + xs), o2 = 4u * (unsigned)(ys * s2h + xs),
                   o3 = 4u * (unsigned)(ys * s3h + xs), o4 = 4u * (unsigned)(ys * s4h + xs);
    f32x4 go[3], tp[16];
    const f32x4 fx4 = ld4_stream_u<F32>(flow_b, o2), fy4 = ld4_stream_u<F32>(flow_b + s2c, o2);
#pragma unroll
    for (int c = 0; c < 3; c++) go[c] = ld4_stream_u<F32>(gout_b + c * s1c, o1);
    const f32x4 oc = ld4_stream_u<F32>(occ_b, o4);
#pragma unroll
    for (int k = 0; k < 16; k++) tp[k] = ld4_stream_u<F32>(filt_b + k * s3c, o3);

    MEMC_FI_SITES(g, x, y, W, H, inb, fx4, fy4);
    const BBox box = tile_bbox<LX, NT>(cmin, cmax, rmin, rmax, bb);
    const Bands bands = make_bands<LX, true, PG::kCap>(box);
    unsigned done = 0;
    fi_blend_bwd_store_invalid(inb, g.valid, go, in_b, s1c, o1, gflow_b, s2c, o2, gfilt_b, s3c, o3, gocc_b, o4);
    auto site = [&](int j) {                   // one site from global memory
        fi_blend_bwd_site(x + j, y, W, H, in_b, s1c, s1h, flow_b + o2 / 4 + j, gflow_b + o2 / 4 + j, s2c,
                          filt_b + o3 / 4 + j, gfilt_b + o3 / 4 + j, s3c, gout_b + o1 / 4 + j, occ_b + o4 / 4 + j,
                          gocc_b + o4 / 4 + j);
    };
#pragma unroll 1
    for (int bi = 0; bi < bands.n; bi++) {
        const Region r = band_region(box, bands, bi, 0);
        const unsigned fast = inb ? fi_covered(r, g, W, H) & ~done : 0u;
        // later bands run only if some site still needs them; the vote is also the barrier that frees the LDS
        if (bi > 0 && !__syncthreads_or(fast != 0)) continue;
        done |= fast;
        const StageSlot sl = stage_slots<NT>(r);
        StageRegs<3> sr;
        tile_stage_load<3, false>(r, sl, in_b, s1c, s1h, sr);
        tile_stage_store<3, false>(r, sl, sr, tile);
        __syncthreads();
        fi_blend_bwd_phase1(r, fast, g, tp, go, oc, tile, W, H, gflow_b, s2c, o2, gfilt_b, s3c, o3, gocc_b, o4);
        if (fast != 0xFu) {                    // mixed quads (rare): site by site
            unsigned todo = fast;
            while (todo) {
                const int j = __ffs(todo) - 1;
                todo &= todo - 1;
                site(j);
            }
        }
    }
    unsigned slow = inb ? g.valid & ~done : 0u;            // not coverable within kMaxBands bands (rare)
    while (slow) {
        const int j = __ffs(slow) - 1;
        slow &= slow - 1;
        site(j);
    }
}

// The tiles cover the width's quads: 64 x NT / 16 sites each.
template <int NT = 256>
static void launch_fi_blend_bwd_c3(const FiBlendBwdCall &k)
{
    const TileGrid g = fi_tile_grid<TileGeom<16, 3072, NT>>(k.w, k.h);
    hipLaunchKernelGGL((fi_blend_bwd_c3<NT>), dim3((unsigned)g.ntx * g.nty * k.batch), dim3(NT), PkGeomT<NT>::kLds, k.stream,
                       k.w, k.h, g.ntx, g.nty, k.batch, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c, k.s2.h, k.s3.b, k.s3.c, k.s3.h,
                       k.s4.b, k.s4.h, k.in1, k.flow, k.filt, k.occ, k.gout, k.gflow, k.gfilt, k.gocc);
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_blend_grad.h)
// ==================================================================================================
using namespace memc;

extern "C" {

const char *memc_blend_grad_version(void) { return "memc_hip_blend_grad 0.1 gfx950"; }

const char *memc_blend_grad_last_kernel_path(void) { return memc::t_blend_grad_path; }

int FilterInterpolationBlendLayer_gpu_backward(memc_stream_t stream, const memc_tensor4 *input, const memc_tensor4 *flow,
                                               const memc_tensor4 *filter, const memc_tensor4 *occlusion,
                                               const memc_tensor4 *gradoutput, const memc_tensor4 *gradflow,
                                               const memc_tensor4 *gradfilter, const memc_tensor4 *gradocclusion)
{
    for (const memc_tensor4 *t : {input, flow, filter, occlusion, gradoutput, gradflow, gradfilter, gradocclusion})
        if (!ok(t)) return kErr;
    if (!flow_matches(input, flow) || !taps_match(input, filter) || !occlusion_matches(input, occlusion)) return kErr;
    const int fs = fi_filter_side_exact(filter->size[1]);
    if (fs < 1) return kErr;
    if (!same_layout(input, gradoutput) || !same_layout(flow, gradflow) || !same_layout(filter, gradfilter) ||
        !same_layout(occlusion, gradocclusion))
        return kErr;
    const FiChecked q = fi_sizes(fs, input);
    if (q.done) return q.code;
    // coverage: the tiled RGB kernel; anything else is the caller's composition of the warp's entry points
    if (!(fi_rgb_tiled_shape(q.c, fs, q.w) &&
          plane_fits_u32(q.w, q.h, {(long)input->stride[2], (long)flow->stride[2], (long)filter->stride[2],
                                    (long)occlusion->stride[2]})))
        return kNotCovered;
    const FiBlendBwdCall k = {
        (hipStream_t)stream, q.w, q.h, q.n, plane(input), plane(flow), plane(filter), plane(occlusion),
        reinterpret_cast<const float *>(input->data), reinterpret_cast<const float *>(flow->data),
        reinterpret_cast<const float *>(filter->data), reinterpret_cast<const float *>(occlusion->data),
        reinterpret_cast<const float *>(gradoutput->data), reinterpret_cast<float *>(gradflow->data),
        reinterpret_cast<float *>(gradfilter->data), reinterpret_cast<float *>(gradocclusion->data)};
    t_blend_grad_path = "fi_blend_bwd:tiled_c3";
    launch_fi_blend_bwd_c3<256>(k);
    return launch_status();
}

}  // extern "C"
