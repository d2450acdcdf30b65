// fi_blend_bwd_c3_body.inc -- the body of the RGB (C == 3, fs == 4) LDS-tiled backward of one direction of the blend,
// included INSIDE the kernels that run it:
//   fi_blend_bwd_c3      (fi_blend_bwd_c3.hip, libmemc_hip_blend_grad.so)          I = T = FT = GT = F32;
//   fi_blend_bwd_c3_mx   (mx_fi_blend_bwd_c3.hip, libmemc_hip_mx_blend_grad.so)    I = GT = F32, T = F16 / BF16, FT = F32 or T;
//   fi_blend_bwd_c3_lp   (lp_fi_blend_bwd_c3.hip, libmemc_hip_lp_blend_grad.so)    I = T = F16 / BF16, FT and GT = F32 or T.
// The including kernel defines the storage tags I (image), T (taps, occlusion and their gradients), FT (flow, flow
// gradient) and GT (gradoutput), the compile-time NT, and the parameters W, H, tiles_x, tiles_y, batch, s1b .. s4h, in1,
// flow, filt, occ, gout, gflow, gfilt, gocc.  The image is staged into the fp32 LDS tile as the warp's backward stages it
// (fi_bwd_stage_load / fi_bwd_stage_store of memc_fi_bwd_c3.hpp: fp32 quads, or half quads widened when they are written);
// every global load widens exactly (memc_lp.hpp) and every stored gradient is rounded once.  (Included text rather than an
// always-inline function: see fi_bwd_c3_body.inc.)  Description: fi_blend_bwd_c3.hip and memc_fi_blend_bwd_c3.hpp.
{
    constexpr bool kF32 = sizeof(st_t<T>) == 4 && sizeof(st_t<FT>) == 4;
    constexpr bool kMx = sizeof(st_t<I>) == 4 && sizeof(st_t<GT>) == 4;              // fp32 image and gradoutput
    static_assert(!kF32 || kMx, "fp32 taps: an fp32 image and gradoutput");
    constexpr unsigned zT = sizeof(st_t<T>), zF = sizeof(st_t<FT>), zI = sizeof(st_t<I>), zG = sizeof(st_t<GT>);   // bytes per element
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
    const st_t<I> *in_b = in1 + b * s1b;
    const st_t<FT> *flow_b = flow + b * s2b;
    const st_t<T> *filt_b = filt + b * s3b;
    const st_t<T> *occ_b = occ + b * s4b;
    const st_t<GT> *gout_b = gout + b * s1b;
    st_t<FT> *gflow_b = gflow + b * s2b;
    st_t<T> *gfilt_b = gfilt + b * s3b;
    st_t<T> *gocc_b = gocc + b * s4b;
    // byte offsets of the lane's quad in the planes of the four layouts (o1: gradoutput's; oi: the image's)
    const unsigned o1 = zG * (unsigned)(ys * s1h + xs), oi = zI * (unsigned)(ys * s1h + xs), o2 = zF * (unsigned)(ys * s2h + xs),
                   o3 = zT * (unsigned)(ys * s3h + xs), o4 = zT * (unsigned)(ys * s4h + xs);
    f32x4 go[3], tp[16];
    const f32x4 fx4 = opaque4<FT>(ld4_stream_u<FT>(flow_b, o2)), fy4 = opaque4<FT>(ld4_stream_u<FT>(flow_b + s2c, o2));
#pragma unroll
    for (int c = 0; c < 3; c++) go[c] = ld4_stream_u<GT>(gout_b + c * s1c, o1);
    const f32x4 oc = ld4_stream_u<T>(occ_b, o4);
#pragma unroll
    for (int k = 0; k < 16; k++) tp[k] = ld4_stream_u<T>(filt_b + k * s3c, o3);

    MEMC_FI_SITES(g, x, y, W, H, inb, fx4, fy4);
    const BBox box = tile_bbox<LX, NT>(cmin, cmax, rmin, rmax, bb);
    const Bands bands = make_bands<LX, true, PG::kCap>(box);
    unsigned done = 0;
    fi_blend_bwd_store_invalid<T, FT, I>(inb, g.valid, go, in_b, s1c, oi, gflow_b, s2c, o2, gfilt_b, s3c, o3, gocc_b, o4);
    // one site from global memory: the fp32 unit's named function, its mixed or its half instantiation
#define MEMC_BLEND_SITE_ARGS(j)                                                                                         \
    x + j, y, W, H, in_b, s1c, s1h, flow_b + o2 / zF + j, gflow_b + o2 / zF + j, s2c, filt_b + o3 / zT + j,             \
        gfilt_b + o3 / zT + j, s3c, gout_b + o1 / zG + j, occ_b + o4 / zT + j, gocc_b + o4 / zT + j
    auto site = [&](int j) {
        if constexpr (kF32) fi_blend_bwd_site(MEMC_BLEND_SITE_ARGS(j));
        else if constexpr (kMx) fi_blend_bwd_site_mx<T, FT>(MEMC_BLEND_SITE_ARGS(j));
        else fi_blend_bwd_site_lp<T, FT, GT>(MEMC_BLEND_SITE_ARGS(j));
    };
#pragma unroll 1
    for (int bi = 0; bi < bands.n; bi++) {
        const Region r = band_region(box, bands, bi, 0);
        const unsigned fast = inb ? fi_covered(r, g, W, H) & ~done : 0u;
        // later bands run only if some site still needs them; the vote is also the barrier that frees the LDS
        if (bi > 0 && !__syncthreads_or(fast != 0)) continue;
        done |= fast;
        const StageSlot sl = stage_slots<NT>(r);
        StageRegsOf<I> sr;
        fi_bwd_stage_load<I, false>(r, sl, in_b, s1c, s1h, sr);
        fi_bwd_stage_store<I, false>(r, sl, sr, tile);
        __syncthreads();
        fi_blend_bwd_phase1<T, FT>(r, fast, g, tp, go, oc, tile, W, H, gflow_b, s2c, o2, gfilt_b, s3c, o3, gocc_b, o4);
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
#undef MEMC_BLEND_SITE_ARGS
}
