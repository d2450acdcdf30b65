// lp_interpolation.hip -- the plain bilinear backward warp (Interpolation / InterpolationCh) on fp16 / bf16 storage, for
// gfx950: forward for any channel count, backward for RGB.  The kernels and the C ABI of libmemc_hip_lp_bl.so
// (include/memc_warp_lp_bl.h).
//
// This is the bilinear warp of a model cast to bf16 / fp16.  Widened on the host the RGB forward is a cast pass over the
// image, one over the flow, the fp32 kernel and a cast pass over the output (~80 B per site, four launches); read as they
// are the tensors are 16 B per site: image 6 (staged, once per tile box) + flow 4 read, output 6 written.
//
// The kernels RESTATE interpolation.hip's (that file is untouched): bl_fwd_lp_tiled is bl_fwd_tiled<CT, CAP, false> with
// bl_fwd_chunk, bl_fwd_lp is bl_fwd<CT> (x0 == 0), bl_bwd_lp_c3_pk is bl_bwd_c3_pk<4096, 512, false> -- without the ragged
// width's branches and the measurement arms.  They are written out rather than shared as a body: the fp32 kernels stage
// through one float loader and store float quads where these stage 8-byte quads of T into the same fp32 LDS image and
// narrow at every store, and the flow has a storage of its own.  Same geometry (64 x 16 tiles on 256 lanes forward,
// 64 x 32 on 512 backward, tile_region<16, true, CAP>), same arithmetic in the same order in fp32 on exactly widened
// inputs; every stored element of the output and of the flow gradient is rounded once.  So they equal, bit for bit, the
// fp32 library's on the widened inputs after one `.to(dtype)`.  The image gradient stays an fp32 buffer that the backward
// ADDS into (packed LDS planes flushed with global atomics, per-site atomics outside the box: memc_pk.hpp), as in
// libmemc_hip_lp_grad.so.  Nothing is allocated, no workspace.
#include "memc_common.hpp"
#include "memc_lp.hpp"
#include "memc_pk.hpp"
#include "memc_fi_abi.hpp"
#include "memc_warp_lp_bl.h"

namespace memc {

thread_local const char *t_lp_bl_path = "";

// scalar accesses of either storage (the one-lane-per-site kernel, the rare global corner gathers): widened as an opaque
// fp32 value, so that the arithmetic contracts as the fp32 kernels' does (memc_lp.hpp: widen_f32)
template <class S>
__device__ __forceinline__ float ld1_stream(const st_t<S> *p) { return widen_f32<S>(__builtin_nontemporal_load(p)); }
template <class S>
__device__ __forceinline__ float ld1(const st_t<S> *p) { return widen_f32<S>(*p); }
template <class S>
__device__ __forceinline__ void st1_stream(st_t<S> *p, float v) { __builtin_nontemporal_store(narrow_f32<S>(v), p); }

// the NCH channel planes of one tensor from plane0 on, as lp_stage_load takes them
template <int NCH>
struct LpPlanes {
    const unsigned short *p[NCH];
};
template <int NCH>
__device__ __forceinline__ LpPlanes<NCH> lp_planes(const unsigned short *plane0, int64_t cstride)
{
    LpPlanes<NCH> pl;
#pragma unroll
    for (int c = 0; c < NCH; c++) pl.p[c] = plane0 + c * cstride;
    return pl;
}

// a quad of fp32 results narrowed and stored: the quad goes through an empty asm so that no conversion is folded into the
// FMA that produced its operand (memc_lp.hpp: narrow_f32, st4_stream_u)
template <class S>
__device__ __forceinline__ void st4_rounded(st_t<S> *p, f32x4 v)
{
    if constexpr (sizeof(st_t<S>) != 4) asm volatile("" : "+v"(v));
    st4_stream<S>(p, v);
}

// --------------------------------------------------------------------------------------------------
// Forward, one lane per site: any width, stride and alignment (bl_fwd<CT> of interpolation.hip)
// --------------------------------------------------------------------------------------------------
template <class T, class FT, int CT>
__global__ __launch_bounds__(256) void bl_fwd_lp(
    int W, int H, int C, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h,
    const st_t<T> *__restrict__ in1, const st_t<FT> *__restrict__ flow, st_t<T> *__restrict__ out)
{
    const unsigned tile = xcd_chunked_id(blockIdx.x, gridDim.x);
    const int tx = tile % tiles_x;
    const int ty = (tile / tiles_x) % tiles_y;
    const int b = tile / (tiles_x * tiles_y);
    const int x = tx * kWave + (threadIdx.x & (kWave - 1));
    const int y = ty * 4 + (threadIdx.x / kWave);
    if (x >= W || y >= H) return;

    const st_t<FT> *flow_b = flow + b * s2b + (int64_t)y * s2h + x;
    const float fx = ld1_stream<FT>(flow_b);
    const float fy = ld1_stream<FT>(flow_b + s2c);
    const BlSite s = bl_locate<true>(x, y, W, H, fx, fy);
    const st_t<T> *in_b = in1 + b * s1b;
    st_t<T> *out_p = out + b * s1b + (int64_t)y * s1h + x;
    const int nc = CT > 0 ? CT : C;
    constexpr int kUnroll = CT > 0 ? CT : 4;
    if (s.valid) {
        const int oTL = s.T * s1h + s.L, oTR = s.T * s1h + s.R;
        const int oBL = s.Bm * s1h + s.L, oBR = s.Bm * s1h + s.R;
        const float w00 = (1 - s.a) * (1 - s.b), w01 = s.a * (1 - s.b);
        const float w10 = (1 - s.a) * s.b, w11 = s.a * s.b;
#pragma unroll kUnroll
        for (int c = 0; c < nc; c++) {
            const st_t<T> *p = in_b + c * s1c;
            st1_stream<T>(out_p + c * s1c,
                          w00 * ld1<T>(p + oTL) + w01 * ld1<T>(p + oTR) + w10 * ld1<T>(p + oBL) + w11 * ld1<T>(p + oBR));
        }
    } else {
        for (int c = 0; c < nc; c++) st1_stream<T>(out_p + c * s1c, 0.0f);
    }
}

// --------------------------------------------------------------------------------------------------
// Forward, LDS-tiled (bl_fwd_tiled / bl_fwd_chunk of interpolation.hip): the LDS image is the fp32 pixel-quad tile, staged
// from 8-byte quads of T
// --------------------------------------------------------------------------------------------------
struct BlSite4 {
    int oTL[4], oTR[4], oBL[4], oBR[4];   // LDS pixel indices of the four corners (0 when not staged)
    f32x4 w00, w01, w10, w11;             // (vectors, not arrays: the struct then never lives in memory)
    unsigned valid, staged;
};

template <class T, int NCH>
__device__ __forceinline__ void bl_fwd_lp_chunk(const Region &r, const BlSite4 &g, const BlSite (&st)[4], bool inb,
                                                const st_t<T> *__restrict__ plane0, st_t<T> *__restrict__ out_p,
                                                int64_t s1c, int s1h, f32x4 *tile)
{
    {
        const StageSlot sl = stage_slots(r);
        LpStageRegs<NCH> sr;
        const LpPlanes<NCH> pl = lp_planes<NCH>(plane0, s1c);
        lp_stage_load<NCH>(r, sl, pl.p, s1h, sr);
        lp_stage_store<T, NCH>(r, sl, sr, tile);
    }
    __syncthreads();
    if (!inb) return;
    f32x4 res[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        res[j] = g.w00[j] * tile[g.oTL[j]] + g.w01[j] * tile[g.oTR[j]] + g.w10[j] * tile[g.oBL[j]] +
                 g.w11[j] * tile[g.oBR[j]];
        const bool valid = (g.valid >> j) & 1, staged = (g.staged >> j) & 1;
        if (valid && !staged) {               // rare: corners outside the staged box -> global gathers
            const BlSite &s = st[j];
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const st_t<T> *p = plane0 + c * s1c;
                res[j][c] = g.w00[j] * ld1<T>(p + s.T * s1h + s.L) + g.w01[j] * ld1<T>(p + s.T * s1h + s.R) +
                            g.w10[j] * ld1<T>(p + s.Bm * s1h + s.L) + g.w11[j] * ld1<T>(p + s.Bm * s1h + s.R);
            }
        }
        if (!valid) res[j] = f32x4{0.f, 0.f, 0.f, 0.f};     // out-of-range site -> 0
    }
#pragma unroll
    for (int c = 0; c < NCH; c++)
        st4_rounded<T>(out_p + c * s1c, f32x4{res[0][c], res[1][c], res[2][c], res[3][c]});
}

// CT == 3: RGB in one chunk; CT == 0: chunks of four planes and a tail of one to three
template <class T, class FT, int CT, int CAP>
__global__ __launch_bounds__(256, 2) void bl_fwd_lp_tiled(
    int W, int H, int C, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h,
    const st_t<T> *__restrict__ in1, const st_t<FT> *__restrict__ flow, st_t<T> *__restrict__ out, int sw)
{
    constexpr int LX = 16;
    using G = TileGeom<LX, CAP>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem);
    int *bb = reinterpret_cast<int *>(smem + G::kCapPx * 16);

    const TileCoord tc = tile_walk(blockIdx.x, gridDim.x, tiles_x, tiles_y, sw);
    if (tc.tx >= tiles_x) return;
    const int b = tc.b, tile_x0 = tc.tx * G::kTW, tile_y0 = tc.ty * G::kTH;
    const int x = tile_x0 + 4 * (threadIdx.x % LX), y = tile_y0 + threadIdx.x / LX;
    const bool inb = x < W && y < H;
    const int xs = min(x, W - 4), ys = min(y, H - 1);
    const st_t<FT> *flow_p = flow + b * s2b + (int64_t)ys * s2h + xs;
    const f32x4 fx4 = opaque4<FT>(ld4_stream<FT>(flow_p)), fy4 = opaque4<FT>(ld4_stream<FT>(flow_p + s2c));

    BlSite st[4];
    int cmin = INT_MAX, cmax = -1, rmin = INT_MAX, rmax = -1;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        st[j] = bl_locate<true>(x + j, y, W, H, fx4[j], fy4[j]);
        st[j].valid = st[j].valid && inb;
        if (st[j].valid) {
            cmin = min(cmin, st[j].L);  cmax = max(cmax, st[j].R);
            rmin = min(rmin, st[j].T);  rmax = max(rmax, st[j].Bm);
        }
    }
    const Region r = tile_region<LX, true, CAP>(cmin, cmax, rmin, rmax, tile_x0, tile_y0, bb);
    BlSite4 g;
    g.valid = g.staged = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const BlSite &s = st[j];
        const bool staged = s.valid && r.covers(s.L, s.R, s.T, s.Bm);
        g.valid |= (s.valid ? 1u : 0u) << j;
        g.staged |= (staged ? 1u : 0u) << j;
        const int rT = staged ? (s.T - r.y0) * r.pitch : 0, rB = staged ? (s.Bm - r.y0) * r.pitch : 0;
        const int cL = staged ? swz_col(s.L - r.x0) : 0, cR = staged ? swz_col(s.R - r.x0) : 0;
        g.oTL[j] = rT + cL;  g.oTR[j] = rT + cR;  g.oBL[j] = rB + cL;  g.oBR[j] = rB + cR;
        g.w00[j] = (1 - s.a) * (1 - s.b);  g.w01[j] = s.a * (1 - s.b);
        g.w10[j] = (1 - s.a) * s.b;        g.w11[j] = s.a * s.b;
    }
    const st_t<T> *in_b = in1 + b * s1b;
    st_t<T> *out_p = out + b * s1b + (int64_t)y * s1h + x;
    if (CT == 3) {
        bl_fwd_lp_chunk<T, 3>(r, g, st, inb, in_b, out_p, s1c, s1h, tile);
    } else {
        int c0 = 0;
#pragma unroll 1
        for (; c0 + 4 <= C; c0 += 4) {
            if (c0 > 0) __syncthreads();
            // keep what only depends on the site inside the loop (interpolation.hip: hoisted, the per-plane addresses
            // derived from it outgrow the register file and spill)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                asm volatile("" : "+v"(g.oTL[j]), "+v"(g.oTR[j]), "+v"(g.oBL[j]), "+v"(g.oBR[j]));
                asm volatile("" : "+v"(st[j].L), "+v"(st[j].R), "+v"(st[j].T), "+v"(st[j].Bm));
            }
            bl_fwd_lp_chunk<T, 4>(r, g, st, inb, in_b + c0 * s1c, out_p + c0 * s1c, s1c, s1h, tile);
        }
        if (c0 < C) {
            if (c0 > 0) __syncthreads();
            const int nch = C - c0;
            if (nch == 3)      bl_fwd_lp_chunk<T, 3>(r, g, st, inb, in_b + c0 * s1c, out_p + c0 * s1c, s1c, s1h, tile);
            else if (nch == 2) bl_fwd_lp_chunk<T, 2>(r, g, st, inb, in_b + c0 * s1c, out_p + c0 * s1c, s1c, s1h, tile);
            else               bl_fwd_lp_chunk<T, 1>(r, g, st, inb, in_b + c0 * s1c, out_p + c0 * s1c, s1c, s1h, tile);
        }
    }
}

// --------------------------------------------------------------------------------------------------
// Backward, RGB (bl_bwd_c3_pk<4096, 512> of interpolation.hip): packed fixed-point planes first, then -- the same LDS
// bytes -- the image staged from T.  gin1 is fp32 and added into, gin2 (FT) is assigned at every site.
// --------------------------------------------------------------------------------------------------
constexpr int kBlBwdCap = 4096, kBlBwdNT = 512;

template <class T, class FT>
__global__ __launch_bounds__(kBlBwdNT, 4) void bl_bwd_lp_c3_pk(
    int W, int H, int tiles_x, int tiles_y,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h,
    const st_t<T> *__restrict__ in1, const st_t<FT> *__restrict__ flow, const st_t<T> *__restrict__ gout,
    float *__restrict__ gin1, st_t<FT> *__restrict__ gin2, int sw)
{
    constexpr int LX = 16, CAP = kBlBwdCap, NT = kBlBwdNT;
    using G = TileGeom<LX, CAP, NT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem);
    unsigned long long *const accA = reinterpret_cast<unsigned long long *>(smem);   // the planes alias the image
    unsigned long long *const accB = accA + CAP;
    int *bb = reinterpret_cast<int *>(smem + G::kCapPx * 16);            // 4 ints per wave: boxes; then 4 per wave: bound statistics
    int *mx = bb + 4 * (NT / kWave);

    const TileCoord tc = tile_walk(blockIdx.x, gridDim.x, tiles_x, tiles_y, sw);
    if (tc.tx >= tiles_x) return;
    const int b = tc.b, tile_x0 = tc.tx * G::kTW, tile_y0 = tc.ty * G::kTH;
    const unsigned tid = tid_now();
    const int x = tile_x0 + 4 * (int)(tid % LX), y = tile_y0 + (int)(tid / LX);
    const bool inb = x < W && y < H;
    const int xs = min(x, W - 4), ys = min(y, H - 1);
    const st_t<FT> *flow_p = flow + b * s2b + (int64_t)ys * s2h + xs;
    const f32x4 fx4 = opaque4<FT>(ld4_stream<FT>(flow_p)), fy4 = opaque4<FT>(ld4_stream<FT>(flow_p + s2c));
    const st_t<T> *gout_p = gout + b * s1b + (int64_t)ys * s1h + xs;
    f32x4 go[3];
#pragma unroll
    for (int c = 0; c < 3; c++) go[c] = opaque4<T>(ld4_stream<T>(gout_p + c * s1c));
    {                                          // both planes, while the loads are in flight
        f32x4 *pz = reinterpret_cast<f32x4 *>(smem);
#pragma unroll
        for (int i = 0; i < (CAP + NT - 1) / NT; i++)
            if (CAP % NT == 0 || (int)tid + i * NT < CAP) pz[tid + i * NT] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    BlSite st[4];
    int cmin = INT_MAX, cmax = -1, rmin = INT_MAX, rmax = -1;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        st[j] = bl_locate<true>(x + j, y, W, H, fx4[j], fy4[j]);
        st[j].valid = st[j].valid && inb;
        if (st[j].valid) {
            cmin = min(cmin, st[j].L);  cmax = max(cmax, st[j].R);
            rmin = min(rmin, st[j].T);  rmax = max(rmax, st[j].Bm);
        }
    }
    // per-site bounds of the packed planes (memc_pk.hpp): the bilinear weights are <= 1, so a site's bound is its largest
    // |gradoutput|; published per wave and handed over by the barrier inside tile_region
    int sbits[4];
    unsigned vmask = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int mg = 0;
#pragma unroll
        for (int c = 0; c < 3; c++) mg = max(mg, __float_as_int(go[c][j]) & 0x7FFFFFFF);
        sbits[j] = mg;                         // (>= 0x7F800000: Inf / NaN -- per-site global atomics)
        vmask |= (st[j].valid ? 1u : 0u) << j;
    }
    pk_tile_publish(mx, tid, sbits, sbits, vmask, 0x3F800000);
    const Region r = tile_region<LX, true, CAP, NT>(cmin, cmax, rmin, rmax, tile_x0, tile_y0, bb);
    const PkTile ps = pk_tile_resolve<NT / kWave>(mx);
    const unsigned packed = pk_packed_sites(ps, sbits, vmask);
    const int mode = ps.any;                   // 0: no packed site has anything to add (workgroup-uniform)
    const st_t<T> *in_b = in1 + b * s1b;
    float *gin1_b = gin1 + b * s1b;
    const StageSlot sl = stage_slots<NT>(r);
    LpStageRegs<3> sr;
    const LpPlanes<3> pl = lp_planes<3>(in_b, s1c);
    lp_stage_load<3>(r, sl, pl.p, s1h, sr);                    // in flight during adds and flush

    // ---- image gradient: 4 corners x 3 colours per site = 8 packed LDS adds
    unsigned staged_mask = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!st[j].valid) continue;
        const BlSite &s = st[j];
        const bool staged = r.covers(s.L, s.R, s.T, s.Bm);
        staged_mask |= (staged ? 1u : 0u) << j;
        if (sbits[j] == 0) continue;           // a zero gradient adds nothing
        if (staged && ((packed >> j) & 1u)) {
            const int aT = (s.T - r.y0) * r.pitch, aB = (s.Bm - r.y0) * r.pitch;
            const int aL = pk_col(s.L - r.x0, r.pitch >> 2), aR = pk_col(s.R - r.x0, r.pitch >> 2);
            const float g0 = ps.sa * go[0][j], g1 = ps.sa * go[1][j], g2 = ps.sa * go[2][j];
            pk_add3(accA, accB, aT + aL, g0, g1, g2, ps.sb * ((1 - s.a) * (1 - s.b)));
            pk_add3(accA, accB, aT + aR, g0, g1, g2, ps.sb * (s.a * (1 - s.b)));
            pk_add3(accA, accB, aB + aL, g0, g1, g2, ps.sb * ((1 - s.a) * s.b));
            pk_add3(accA, accB, aB + aR, g0, g1, g2, ps.sb * (s.a * s.b));
        } else {
#pragma unroll 1
            for (int c = 0; c < 3; c++) {
                const float gv = c == 0 ? go[0][j] : (c == 1 ? go[1][j] : go[2][j]);
                float *q = gin1_b + c * s1c;
                atomic_add_f32(q + s.T * s1h + s.L, gv * (1 - s.a) * (1 - s.b));
                atomic_add_f32(q + s.T * s1h + s.R, gv * s.a * (1 - s.b));
                atomic_add_f32(q + s.Bm * s1h + s.L, gv * (1 - s.a) * s.b);
                atomic_add_f32(q + s.Bm * s1h + s.R, gv * s.a * s.b);
            }
        }
    }
    if (mode == 1) {                           // (workgroup-uniform)
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kStageIts; it++)                 // the staged rows have landed: take the wait here, not
#pragma unroll                                                 // behind the flush's conditional atomics (vmcnt is in order)
            for (int c = 0; c < 3; c++) asm volatile("" : "+v"(sr.v[it][c].x), "+v"(sr.v[it][c].y));
        pk_flush<NT>(r, accA, accB, ps.inv, gin1_b, s1c, s1h);
    }
    __syncthreads();                           // the planes have been read (or never used): the LDS becomes the image
    lp_stage_store<T, 3>(r, sl, sr, tile);
    __syncthreads();

    // ---- flow gradient from the four corner values
    f32x4 gx4 = {0.f, 0.f, 0.f, 0.f}, gy4 = gx4;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (!st[j].valid) continue;
        const BlSite &s = st[j];
        const float x2 = (float)(x + j) + fx4[j], y2 = (float)y + fy4[j];
        const float gam_x = (float)s.Bm - y2, gam_y = (float)s.R - x2;   // clamped corners
        f32x4 vTL, vTR, vBL, vBR;
        if ((staged_mask >> j) & 1) {
            const int rT = (s.T - r.y0) * r.pitch, rB = (s.Bm - r.y0) * r.pitch;
            const int cL = swz_col(s.L - r.x0), cR = swz_col(s.R - r.x0);
            vTL = tile[rT + cL];  vTR = tile[rT + cR];  vBL = tile[rB + cL];  vBR = tile[rB + cR];
        } else {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const st_t<T> *p = in_b + c * s1c;
                vTL[c] = ld1<T>(p + s.T * s1h + s.L);   vTR[c] = ld1<T>(p + s.T * s1h + s.R);
                vBL[c] = ld1<T>(p + s.Bm * s1h + s.L);  vBR[c] = ld1<T>(p + s.Bm * s1h + s.R);
            }
        }
        float botx = 0.0f, boty = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float gv = go[c][j];
            float tmp = 0.0f;
            tmp += gam_x * (vTR[c] - vTL[c]);
            tmp += (1 - gam_x) * (vBR[c] - vBL[c]);
            botx += gv * tmp;
            tmp = 0.0f;
            tmp += gam_y * (vBL[c] - vTL[c]);
            tmp += (1 - gam_y) * (vBR[c] - vTR[c]);
            boty += gv * tmp;
        }
        gx4[j] = botx;
        gy4[j] = boty;
    }
    // gradinput2 is ASSIGNED at every site (zeros at the invalid ones): the buffer needs no memset beforehand
    if (inb) {
        st_t<FT> *g2 = gin2 + b * s2b + (int64_t)y * s2h + x;
        st4_rounded<FT>(g2, gx4);
        st4_rounded<FT>(g2 + s2c, gy4);
    }
}

// --------------------------------------------------------------------------------------------------
// Host: the call descriptors and one launch function per kernel family
// --------------------------------------------------------------------------------------------------
template <class T, class FT>
struct BlLpFwdCall {
    hipStream_t stream;
    int w, h, channel, batch;
    Plane s1, s2;
    const st_t<T> *in1;  const st_t<FT> *flow;  st_t<T> *out;
};
template <class T, class FT>
struct BlLpBwdCall {
    hipStream_t stream;
    int w, h, batch;
    Plane s1, s2;
    const st_t<T> *in1;  const st_t<FT> *flow;  const st_t<T> *gout;
    float *gin1;  st_t<FT> *gin2;
};

template <int CT, int CAP, class T, class FT>
static void launch_bl_fwd_lp_tiled(const BlLpFwdCall<T, FT> &k)
{
    using G = TileGeom<16, CAP>;
    const TileGrid g = fi_tile_grid<G>(k.w, k.h);
    const int sw = kDefaultStripe;
    hipLaunchKernelGGL((bl_fwd_lp_tiled<T, FT, CT, CAP>), dim3(walk_grid(g.ntx, g.nty, k.batch, sw)), dim3(256),
                       (tile_lds_bytes<16, CAP>()), k.stream, k.w, k.h, k.channel, g.ntx, g.nty, k.s1.b, k.s1.c, k.s1.h,
                       k.s2.b, k.s2.c, k.s2.h, k.in1, k.flow, k.out, sw);
}

template <int CT, class T, class FT>
static void launch_bl_fwd_lp_direct(const BlLpFwdCall<T, FT> &k)
{
    const int tiles_x = (k.w + kWave - 1) / kWave, tiles_y = (k.h + 3) / 4;
    hipLaunchKernelGGL((bl_fwd_lp<T, FT, CT>), dim3((unsigned)tiles_x * tiles_y * k.batch), dim3(256), 0, k.stream, k.w, k.h,
                       k.channel, tiles_x, tiles_y, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c, k.s2.h, k.in1, k.flow, k.out);
}

template <class T, class FT>
static void launch_bl_bwd_lp_c3_pk(const BlLpBwdCall<T, FT> &k)
{
    using G = TileGeom<16, kBlBwdCap, kBlBwdNT>;
    constexpr size_t lds = kBlBwdCap * 16 + 32 * (kBlBwdNT / kWave);   // image or planes; 32 bytes per wave: box, bounds
    const TileGrid g = fi_tile_grid<G>(k.w, k.h);
    const int sw = kDefaultStripe;
    const auto kernel = bl_bwd_lp_c3_pk<T, FT>;
    allow_big_lds(kernel, lds);                // per launch: the attribute belongs to the CURRENT device
    hipLaunchKernelGGL(kernel, dim3(walk_grid(g.ntx, g.nty, k.batch, sw)), dim3(kBlBwdNT), lds, k.stream, k.w, k.h, g.ntx,
                       g.nty, k.s1.b, k.s1.c, k.s1.h, k.s2.b, k.s2.c, k.s2.h, k.in1, k.flow, k.gout, k.gin1, k.gin2, sw);
}

// the shapes and layouts the tiled kernels take: whole 8-byte quads of T, at least two per row; the flow's tensors (`fts`)
// aligned for their storage
static bool bl_lp_tiled_ok(int w, memc_dtype flowt, std::initializer_list<const memc_tensor4 *> ts,
                           std::initializer_list<const memc_tensor4 *> fts)
{
    if (w % 4 != 0 || w < 8) return false;
    for (const memc_tensor4 *t : ts)
        if (!quad_ok(t)) return false;
    return storage_ok(flowt, fts);
}

static int bl_lp_forward(bool require_c3, hipStream_t stream, memc_dtype payload, memc_dtype flowt,
                         const memc_tensor4 *input1, const memc_tensor4 *input2, const memc_tensor4 *output)
{
    // malformed (-1): the dtype rule, then the checks of bilinear_forward (layer_api.cpp) in its order
    if (!dtypes_ok(payload, flowt)) return kErr;
    if (!ok(input1) || !ok(input2) || !ok(output)) return kErr;
    if (require_c3 && input1->size[1] != 3) return kErr;
    if (!flow_matches(input1, input2)) return kErr;
    if (!same_layout(input1, output)) return kErr;
    // empty (0)
    const int n = (int)input1->size[0], c = (int)input1->size[1], h = (int)input1->size[2], w = (int)input1->size[3];
    if (n == 0 || c == 0 || h == 0 || w == 0) return 0;
    // coverage (1): every forward kernel forms the row offsets of a site's four source pixels in int ELEMENTS of input1's
    // layout (row * row_stride + column); the flow's offsets are 64-bit
    if ((int64_t)(h - 1) * input1->stride[2] + w > (int64_t)INT32_MAX) return kNotCovered;
    const bool tiled = bl_lp_tiled_ok(w, flowt, {input1, output}, {input2});
    return fi_dispatch(payload, flowt, [&](auto p, auto ft) {
        using T = decltype(p);
        using FT = decltype(ft);
        const BlLpFwdCall<T, FT> k = {stream, w, h, c, n, plane(input1), plane(input2),
                                      data_of<T>(input1), data_of<FT>(input2), data_of<T>(output)};
        if (tiled && c == 3) {
            t_lp_bl_path = "bl_fwd_lp:tiled_c3";
            launch_bl_fwd_lp_tiled<3, 2496>(k);        // 39 KiB: four workgroups per CU (interpolation.hip: launch_bl_fwd)
        } else if (tiled) {
            t_lp_bl_path = "bl_fwd_lp:tiled_chunks";
            launch_bl_fwd_lp_tiled<0, 3072>(k);
        } else {
            t_lp_bl_path = "bl_fwd_lp:direct";
            if (c == 3) launch_bl_fwd_lp_direct<3>(k);
            else launch_bl_fwd_lp_direct<0>(k);
        }
        return launch_status();
    });
}

static int bl_lp_backward(bool require_c3, hipStream_t stream, memc_dtype payload, memc_dtype flowt,
                          const memc_tensor4 *input1, const memc_tensor4 *input2, const memc_tensor4 *gradoutput,
                          const memc_tensor4 *gradinput1, const memc_tensor4 *gradinput2)
{
    // malformed (-1): the dtype rule, then the checks of bilinear_backward (layer_api.cpp) in its order
    if (!dtypes_ok(payload, flowt)) return kErr;
    if (!ok(input1) || !ok(input2) || !ok(gradoutput) || !ok(gradinput1) || !ok(gradinput2)) return kErr;
    if (require_c3 && input1->size[1] != 3) return kErr;
    if (!flow_matches(input1, input2)) return kErr;
    if (!same_layout(input1, gradinput1) || !same_layout(input2, gradinput2)) return kErr;
    if (!same_layout(input1, gradoutput)) return kErr;
    // empty (0)
    const int n = (int)input1->size[0], c = (int)input1->size[1], h = (int)input1->size[2], w = (int)input1->size[3];
    if (n == 0 || c == 0 || h == 0 || w == 0) return 0;
    // coverage (1): RGB, whole quads, aligned storage, 32-bit in-plane offsets (the flush: memc_pk.hpp)
    if (!(c == 3 && bl_lp_tiled_ok(w, flowt, {input1, gradoutput}, {input2, gradinput2}) && dword_ok(gradinput1) &&
          plane_fits_u32(w, h, {(long)input1->stride[2]})))
        return kNotCovered;
    t_lp_bl_path = "bl_bwd_lp:tiled_c3";
    return fi_dispatch(payload, flowt, [&](auto p, auto ft) {
        using T = decltype(p);
        using FT = decltype(ft);
        launch_bl_bwd_lp_c3_pk<T, FT>({stream, w, h, n, plane(input1), plane(input2), data_of<T>(input1),
                                       data_of<FT>(input2), data_of<T>(gradoutput), data_of<F32>(gradinput1),
                                       data_of<FT>(gradinput2)});
        return launch_status();
    });
}

}  // namespace memc

// ==================================================================================================
// C ABI (include/memc_warp_lp_bl.h)
// ==================================================================================================
using namespace memc;

extern "C" {

const char *memc_lp_bl_version(void) { return "memc_hip_lp_bl 0.1 gfx950"; }

const char *memc_lp_bl_last_kernel_path(void) { return memc::t_lp_bl_path; }

int InterpolationLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype payload, memc_dtype flowt, const memc_tensor4 *input1,
                                      const memc_tensor4 *input2, const memc_tensor4 *output)
{ return bl_lp_forward(true, (hipStream_t)stream, payload, flowt, input1, input2, output); }

int InterpolationChLayer_gpu_forward_lp(memc_stream_t stream, memc_dtype payload, memc_dtype flowt, const memc_tensor4 *input1,
                                        const memc_tensor4 *input2, const memc_tensor4 *output)
{ return bl_lp_forward(false, (hipStream_t)stream, payload, flowt, input1, input2, output); }

int InterpolationLayer_gpu_backward_lp(memc_stream_t stream, memc_dtype payload, memc_dtype flowt, const memc_tensor4 *input1,
                                       const memc_tensor4 *input2, const memc_tensor4 *gradoutput,
                                       const memc_tensor4 *gradinput1, const memc_tensor4 *gradinput2)
{ return bl_lp_backward(true, (hipStream_t)stream, payload, flowt, input1, input2, gradoutput, gradinput1, gradinput2); }

int InterpolationChLayer_gpu_backward_lp(memc_stream_t stream, memc_dtype payload, memc_dtype flowt,
                                         const memc_tensor4 *input1, const memc_tensor4 *input2,
                                         const memc_tensor4 *gradoutput, const memc_tensor4 *gradinput1,
                                         const memc_tensor4 *gradinput2)
{ return bl_lp_backward(false, (hipStream_t)stream, payload, flowt, input1, input2, gradoutput, gradinput1, gradinput2); }

}  // extern "C"
