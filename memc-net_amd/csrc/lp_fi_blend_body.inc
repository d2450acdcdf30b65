// lp_fi_blend_body.inc -- the body of the fused dual warp + occlusion blend on half-width taps and occlusions, RGB, fs == 4
// (fi_fwd_blend_c3), included INSIDE the kernels that run it:
//   fi_blend_lp_tiled   (lp_filter_interpolation.hip, libmemc_hip_lp.so)   I = T: images and output in T;
//   fi_blend_mx_tiled   (mx_filter_interpolation.hip, libmemc_hip_mx.so)   I = F32: fp32 images and output.
// The including kernel defines the storage tags T (taps, occlusions), FT (flows) and I (images, output) and the parameters
// W, H, tiles_x, tiles_y, s1b .. s3h, sob, soh, in0, in2, flow0, flow1, filt0, filt1, occ0, occ1, out.  (Included text
// rather than an always-inline function: see lp_fi_fwd_body.inc.)
//
//     out = occ0 * FI(in0, flow0, filt0) + occ1 * FI(in2, flow1, filt1)       (two products, one sum, rounded once to I)
// Both directions' streams are requested up front -- direction 1's taps stay packed (two registers per quad) until
// direction 0 is done -- then each direction runs its own box -> (bands of) stage -> gather round on the same LDS bytes.
{
    constexpr int LX = 16;
    using G = TileGeom<LX>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem);
    int *bb = reinterpret_cast<int *>(smem + G::kCapPx * 16);

    const TileCoord tc = strip_walk(blockIdx.x, gridDim.x, tiles_x, tiles_y, gridDim.x / (tiles_x * tiles_y));
    const int b = tc.b;
    const int x = tc.tx * G::kTW + 4 * (int)(threadIdx.x % LX), y = tc.ty * G::kTH + (int)(threadIdx.x / LX);
    const bool inb = x < W && y < H;
    const int xs = min(x, W - 4), ys = min(y, H - 1);
    const int64_t o2 = (int64_t)ys * s2h + xs, o3 = (int64_t)ys * s3h + xs, oo = (int64_t)ys * soh + xs;
    // all streams of both directions first
    f32x4 fx[2], fy[2], oc[2], tp[16];
    u16x4 tq1[16];
    fx[0] = ld4_stream<FT>(flow0 + b * s2b + o2);  fy[0] = ld4_stream<FT>(flow0 + b * s2b + s2c + o2);
    fx[1] = ld4_stream<FT>(flow1 + b * s2b + o2);  fy[1] = ld4_stream<FT>(flow1 + b * s2b + s2c + o2);
#pragma unroll
    for (int k = 0; k < 16; k++) tp[k] = ld4_stream<T>(filt0 + b * s3b + k * s3c + o3);
#pragma unroll
    for (int k = 0; k < 16; k++) tq1[k] = __builtin_nontemporal_load(reinterpret_cast<const u16x4a *>(filt1 + b * s3b + k * s3c + o3));
    oc[0] = ld4_stream<T>(occ0 + b * sob + oo);
    oc[1] = ld4_stream<T>(occ1 + b * sob + oo);

    // one direction: box -> (bands of) stage -> gather; returns the warped RGB of the lane's four sites
    auto warp = [&](const st_t<I> *in_b, const st_t<FT> *flow_b, const st_t<T> *filt_b, const f32x4 &fx4, const f32x4 &fy4,
                    f32x4 (&res)[4]) {
        int cmin, cmax, rmin, rmax;
        FiSite4 g = fi_sites_fn(x, y, W, H, inb, fx4, fy4, cmin, cmax, rmin, rmax);
        const BBox box = tile_bbox<LX>(cmin, cmax, rmin, rmax, bb);
        const Bands bands = make_bands<LX>(box);
#pragma unroll
        for (int j = 0; j < 4; j++) res[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        unsigned done = 0;
#pragma unroll 1
        for (int bi = 0; bi < bands.n; bi++) {
            const Region rb = band_region(box, bands, bi);
            const unsigned sel = inb ? fi_covered(rb, g, W, H) & ~done : 0u;
            if (bi > 0 && !__syncthreads_or(sel != 0)) continue;
            done |= sel;
            const StageSlot sl = stage_slots(rb);
            const st_t<I> *plane[3] = {in_b, in_b + s1c, in_b + 2 * s1c};
            ImgStageRegs<I, 3> sr;
            img_stage_load<I, 3>(rb, sl, plane, s1h, sr);
            img_stage_store<I, 3>(rb, sl, sr, tile);
            __syncthreads();
            fi_launder_fn(tp, g);
            fi_gather<LX, 3>(rb, g, tp, sel, W, H, tile, res);
        }
        if (!inb) return;
        unsigned slow = g.valid & ~done;                   // rare: not coverable within kMaxBands bands
        while (slow) {
            const int j = __ffs(slow) - 1;
            slow &= slow - 1;
            const st_t<FT> *fp = flow_b + (int64_t)y * s2h + x + j;
            const FiSite s = fi_locate(x + j, y, W, H, widen<FT>(fp[0]), widen<FT>(fp[s2c]));
            const int L = s.ix - 1, Tp = s.iy - 1;               // the site's 4 x 4 window
            f32x4 v;
#pragma unroll 1
            for (int c = 0; c < 3; c++)
                v[c] = fi_site_chan<I, int64_t, T>(s, 4, L, Tp, L + 4, Tp + 4, W, H, in_b + c * s1c, s1h, filt_b + (int64_t)y * s3h + x + j, s3c);
            v[3] = 0.f;
#pragma unroll
            for (int jj = 0; jj < 4; jj++) res[jj] = jj == j ? v : res[jj];
        }
        if (g.valid != 0xFu) {                             // out-of-range sites copy the input pixel
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const f32x4 own = ld4_cached<I>(in_b + c * s1c + (int64_t)y * s1h + x);
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (!((g.valid >> j) & 1)) res[j][c] = own[j];
            }
        }
    };

    f32x4 w0[4], w2[4];
    warp(in0 + b * s1b, flow0 + b * s2b, filt0 + b * s3b, fx[0], fy[0], w0);
    __syncthreads();                                       // direction 0's gathers are done: the LDS is free again
#pragma unroll
    for (int k = 0; k < 16; k++) tp[k] = widen4<T>(tq1[k]);
    warp(in2 + b * s1b, flow1 + b * s2b, filt1 + b * s3b, fx[1], fy[1], w2);
    if (!inb) return;
    st_t<I> *o = out + b * s1b + (int64_t)y * s1h + x;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float p0 = oc[0][j] * w0[j][c], p2 = oc[1][j] * w2[j][c];     // two products, one sum (fi_fwd_blend_c3)
            v[j] = p0 + p2;
        }
        st4_stream<I>(o + c * s1c, v);
    }
}
