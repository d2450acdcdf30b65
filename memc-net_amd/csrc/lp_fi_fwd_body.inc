// lp_fi_fwd_body.inc -- the body of the LDS-tiled adaptive-warp (FilterInterpolation) forward on half-width taps, fs == 4,
// included INSIDE the kernels that run it:
//   fi_fwd_lp_tiled   (lp_filter_interpolation.hip, libmemc_hip_lp.so)   I = T: image and output in T; RGB or many channels;
//   fi_fwd_mx_tiled   (mx_filter_interpolation.hip, libmemc_hip_mx.so)   I = F32: an fp32 image and output; RGB only.
// The including kernel defines the storage tags T (taps), FT (flow) and I (image, output), the compile-time RGB and RAGGED,
// C, and the parameters W, H, tiles_x, tiles_y, s1b .. s3h, in1, flow, filt, out.  Every input is widened exactly and the
// arithmetic is fp32 in one order, so the two storages of the image differ in what is read and in the rounding of the
// store alone: I = F32 stages with memc_tile.hpp's dword-aligned fp32 quads and stores the value as computed.  (Included
// text rather than an always-inline function: behind an inlined call the half library's kernels compile to other machine
// code, its many-channel bf16 ones with private scratch; tools/isa_diff.py is the check.)
//
// 64 x 16 tiles of 256 lanes, one lane = four consecutive sites of a row, strip walk.  RGB: one chunk of three channels,
// bands outside (fi_fwd_tiled_fs4<16, 3, 2, 0>).  Otherwise: bands outside, chunks of four channels inside, the next chunk's
// staging loads issued before this chunk's gathers (fi_fwd_tiled_c4n<0, 256, RAGGED>).  RAGGED (a channel count that is
// not a multiple of four, a separate instantiation): the last chunk re-reads the last plane and stores only the channels
// it has; one workgroup per CU (at two, the bf16 instantiation spills).
{
    static_assert(RGB || std::is_same_v<I, T>, "an image of another storage than the taps: the RGB kernel only");
    constexpr int LX = 16;
    using G = TileGeom<LX>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem);
    int *bb = reinterpret_cast<int *>(smem + G::kCapPx * 16);

    const TileCoord tc = strip_walk(blockIdx.x, gridDim.x, tiles_x, tiles_y, gridDim.x / (tiles_x * tiles_y));
    const int b = tc.b, tile_x0 = tc.tx * G::kTW, tile_y0 = tc.ty * G::kTH;
    const int x = tile_x0 + 4 * (threadIdx.x % LX), y = tile_y0 + threadIdx.x / LX;
    const bool inb = x < W && y < H;                       // W % 4 == 0: a lane's four sites are in or out together
    // streams first, unconditional (a clamped in-range address for lanes past the edge; see fi_fwd_tiled_fs4)
    const int xs = min(x, W - 4), ys = min(y, H - 1);
    const st_t<FT> *flow_p = flow + b * s2b + (int64_t)ys * s2h + xs;
    const st_t<T> *tap_p = filt + b * s3b + (int64_t)ys * s3h + xs;
    const f32x4 fx4 = ld4_stream<FT>(flow_p), fy4 = ld4_stream<FT>(flow_p + s2c);
    f32x4 tp[16];
#pragma unroll
    for (int k = 0; k < 16; k++) tp[k] = ld4_stream<T>(tap_p + k * s3c);

    MEMC_FI_SITES(g, x, y, W, H, inb, fx4, fy4);
    const BBox box = tile_bbox<LX>(cmin, cmax, rmin, rmax, bb);
    const Bands bands = make_bands<LX>(box);
    const st_t<I> *in_b = in1 + b * s1b;
    st_t<I> *out_p = out + b * s1b + (int64_t)y * s1h + x;
    unsigned done = 0;

    if constexpr (RGB) {
        f32x4 res[4];
#pragma unroll
        for (int j = 0; j < 4; j++) res[j] = f32x4{0.f, 0.f, 0.f, 0.f};
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
            MEMC_FI_LAUNDER(tp, g);
            fi_gather<LX, 3>(rb, g, tp, sel, W, H, tile, res);
        }
        if (inb) {
            if (g.valid != 0xFu) {                         // out-of-range sites copy the input pixel
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const f32x4 own = ld4_cached<I>(in_b + c * s1c + (int64_t)y * s1h + x);
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (!((g.valid >> j) & 1)) res[j][c] = own[j];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; c++) st4_stream<I>(out_p + c * s1c, f32x4{res[0][c], res[1][c], res[2][c], res[3][c]});
        }
    } else {
#pragma unroll 1
        for (int bi = 0; bi < bands.n; bi++) {
            const Region r = band_region(box, bands, bi);
            const unsigned sel = inb ? fi_covered(r, g, W, H) & ~done : 0u;
            // later bands only run when somebody still needs them; the vote is also the barrier that frees the LDS
            if (bi > 0 && !__syncthreads_or(sel != 0)) continue;
            done |= sel;
            // band 0 also writes the out-of-range sites (they copy the input pixel)
            const unsigned wr = sel | (bi == 0 && inb ? ~g.valid & 0xFu : 0u);
            const StageSlot sl = stage_slots(r);
            ImgStageRegs<I, 4> sr;
            auto stage_load = [&](int cb) {                // planes past the last one: the last one again
                const st_t<I> *plane[4];
#pragma unroll
                for (int c = 0; c < 4; c++) plane[c] = in_b + (RAGGED ? min(cb + c, C - 1) : cb + c) * s1c;
                img_stage_load<I, 4>(r, sl, plane, s1h, sr);
            };
            stage_load(0);
#pragma unroll 1
            for (int c0 = 0; c0 < C; c0 += 4) {
                img_stage_store<I, 4>(r, sl, sr, tile);
                __syncthreads();
                // next chunk's rows: in flight while this chunk is gathered (the last iteration re-reads its own chunk)
                stage_load(c0 + 4 < C ? c0 + 4 : c0);
                MEMC_FI_LAUNDER(tp, g);
                f32x4 res[4];
#pragma unroll
                for (int j = 0; j < 4; j++) res[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                fi_gather<LX, 4>(r, g, tp, sel, W, H, tile, res);
                const st_t<I> *plane0 = in_b + c0 * s1c;
                st_t<I> *o = out_p + c0 * s1c;
                if (wr & ~g.valid) {                       // out-of-range sites copy the input pixel
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        if (RAGGED && c0 + c >= C) continue;
                        const f32x4 own = ld4_cached<I>(plane0 + c * s1c + (int64_t)y * s1h + x);
#pragma unroll
                        for (int j = 0; j < 4; j++)
                            if (!((g.valid >> j) & 1)) res[j][c] = own[j];
                    }
                }
                if (wr == 0xFu) {
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        if (!RAGGED || c0 + c < C) st4_stream<I>(o + c * s1c, f32x4{res[0][c], res[1][c], res[2][c], res[3][c]});
                } else if (wr) {                           // a lane whose sites are split over bands
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if ((wr >> j) & 1) {
#pragma unroll
                            for (int c = 0; c < 4; c++)
                                if (!RAGGED || c0 + c < C) o[c * s1c + j] = narrow<I>(res[j][c]);
                        }
                }
                __syncthreads();
            }
        }
    }
    unsigned slow = inb ? g.valid & ~done : 0u;            // rare: not coverable within kMaxBands bands
    while (slow) {
        const int j = __ffs(slow) - 1;
        slow &= slow - 1;
        if constexpr (std::is_same_v<I, T>)
            fi_site_scalar_lp<T, FT>(x + j, y, W, H, C, 4, in_b, s1c, s1h, flow_p + j, s2c, tap_p + j, s3c, out_p + j);
        else
            fi_site_scalar_mx<I, FT, T>(x + j, y, W, H, C, 4, in_b, s1c, s1h, flow_p + j, s2c, tap_p + j, s3c, out_p + j);
    }
}
