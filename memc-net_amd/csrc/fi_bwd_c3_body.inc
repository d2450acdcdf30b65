// fi_bwd_c3_body.inc -- the body of the RGB (C == 3, fs == 4) LDS-tiled FilterInterpolation backward, included INSIDE
// the kernels that run it:
//   fi_bwd_c3_pk   (fi_bwd_c3.hip, libmemc_hip.so)            I = P = FT = GT = F32;
//   fi_bwd_c3_lp   (lp_fi_bwd_c3.hip, libmemc_hip_lp_grad.so) I = P = F16 / BF16, FT and GT = F32 or P, RAG = false;
//   fi_bwd_c3_mx   (mx_fi_bwd_c3.hip, libmemc_hip_mx_grad.so) I = GT = F32, P = F16 / BF16, FT = F32 or P, RAG = false.
// The including kernel defines the storage tags I (image), P (taps, tap gradient), FT (flow, flow gradient) and GT
// (gradoutput), the compile-time TR, NT, PART and RAG, and the parameters W, H, tiles_x, tiles_y, batch, s1b .. s3h, in1,
// flow, filt, gout, gin1 (fp32: ADDED into, flushed with atomics), gin2, gin3.  Only the staging of the image box and
// the per-site paths from global memory read the image: with I = P they are the *_lp helpers (memc_fi.hpp), else *_mx.  Every global load widens exactly
// (memc_lp.hpp) and every stored gradient is rounded once: the LDS image, the packed planes and the arithmetic are the
// same for every storage.  (Included text rather than an always-inline function: the extra inlined call level changes
// the compiler's vectorisation and contraction choices, and the fp32 kernel keeps its machine code bit for bit.)
// Description and measurements: fi_bwd_c3.hip and memc_fi_bwd_c3.hpp.
{
    constexpr bool kF32 = sizeof(st_t<P>) == 4 && sizeof(st_t<FT>) == 4 && sizeof(st_t<GT>) == 4;
    static_assert(kF32 || !RAG, "half storage: widths that are a multiple of four");
    constexpr unsigned zP = sizeof(st_t<P>), zF = sizeof(st_t<FT>), zG = sizeof(st_t<GT>);      // bytes per element
    // One site (x + j, y) from global memory, each helper's call spelled once: the fp32 kernel's named function, its half
    // instantiation where the image is stored as the taps are, else the mixed one (memc_fi.hpp; the image gradient's
    // atomics read no image: no mixed one).  Macros, so that the text the compiler sees stays what it was.
#define MEMC_SITE_3WAY(NAME, ...)                                                                                       \
    do {                                                                                                                \
        if constexpr (kF32) NAME(__VA_ARGS__);                                                                          \
        else if constexpr (std::is_same_v<I, P>) NAME##_lp<P, FT, GT>(__VA_ARGS__);                                     \
        else NAME##_mx<P, FT, GT, I>(__VA_ARGS__);                                                                      \
    } while (0)
#define MEMC_SITE_TAPS(j)                                                                                               \
    MEMC_SITE_3WAY(fi_bwd_site_taps, x + j, y, W, H, in_b, s1c, s1h, flow_b + o2 / zF + j, gin2_b + o2 / zF + j, s2c,   \
                   filt_b + o3 / zP + j, gin3_b + o3 / zP + j, s3c, gout_b + o1 / zG + j)
#define MEMC_SITE_SCALAR(j)                                                                                             \
    MEMC_SITE_3WAY(fi_bwd_site_scalar, x + j, y, W, H, 3, 4, in_b, gin1_b, s1c, s1h, flow_b + o2 / zF + j,              \
                   gin2_b + o2 / zF + j, s2c, filt_b + o3 / zP + j, gin3_b + o3 / zP + j, s3c, gout_b + o1 / zG + j)
#define MEMC_SITE_IMAGE_ATOMICS_ARGS(j)                                                                                 \
    x + j, y, W, H, gin1_b, s1c, s1h, flow_b + o2 / zF + j, s2c, filt_b + o3 / zP + j, s3c, gout_b + o1 / zG + j
#define MEMC_SITE_IMAGE_ATOMICS(j)                                                                                      \
    do {                                                                                                                \
        if constexpr (kF32) fi_bwd_site_image_atomics(MEMC_SITE_IMAGE_ATOMICS_ARGS(j));                                 \
        else fi_bwd_site_image_atomics_lp<P, FT, GT>(MEMC_SITE_IMAGE_ATOMICS_ARGS(j));                                  \
    } while (0)
    constexpr int LX = 16;
    using PG = PkGeomT<NT>;
    using G = TileGeom<LX, PG::kCap, NT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4 *tile = reinterpret_cast<f32x4 *>(smem);
    unsigned long long *const accA = reinterpret_cast<unsigned long long *>(smem);   // the planes alias the image
    unsigned long long *const accB = accA + PG::kCap;
    int *bb = reinterpret_cast<int *>(smem + PG::kImageBytes);           // 16 ints: boxes; 16 ints: the waves' bound statistics
    int *mx = bb + 16;

    trace_mark<TR>(0);
    const TileCoord tc = strip_walk(blockIdx.x, gridDim.x, tiles_x, tiles_y, batch);
    const int b = tc.b;
    const unsigned tid = tid_now();
    const int x = tc.tx * G::kTW + 4 * (int)(tid % LX), y = tc.ty * G::kTH + (int)(tid / LX);
    const int Ws = RAG ? W & ~3 : W;
    const bool inb = x < Ws && y < H;
    const int xs = min(x, Ws - 4), ys = min(y, H - 1);
    const st_t<FT> *flow_b = flow + b * s2b;
    const st_t<P> *filt_b = filt + b * s3b;
    const st_t<GT> *gout_b = gout + b * s1b;
    st_t<FT> *gin2_b = gin2 + b * s2b;
    st_t<P> *gin3_b = gin3 + b * s3b;
    // byte offsets of the lane's quad in the planes of input2 / input3 / gradoutput's layouts
    const unsigned o1 = zG * (unsigned)(ys * s1h + xs), o2 = zF * (unsigned)(ys * s2h + xs),
                   o3 = zP * (unsigned)(ys * s3h + xs);
    f32x4 go[3], tp[16];
    const f32x4 fx4 = opaque4<FT>(ld4_stream_u<FT>(flow_b, o2)), fy4 = opaque4<FT>(ld4_stream_u<FT>(flow_b + s2c, o2));
#pragma unroll
    for (int c = 0; c < 3; c++) go[c] = ld4_stream_u<GT>(gout_b + c * s1c, o1);
#pragma unroll
    for (int k = 0; k < 16; k++) tp[k] = ld4_stream_u<P>(filt_b + k * s3c, o3);
    auto zero_planes = [&](int cells) {        // the first `cells` slots of both planes (whole 16-byte units)
        f32x4 *pa = reinterpret_cast<f32x4 *>(accA), *pb = reinterpret_cast<f32x4 *>(accB);
        for (int i = (int)tid_now(); i < (cells >> 1); i += NT) {
            pa[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            pb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    if (PART != 2) zero_planes(PG::kCap);      // while the loads are in flight
    if (TR) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    trace_mark<TR>(1);                                         // inputs have arrived

    MEMC_FI_SITES(g, x, y, W, H, inb, fx4, fy4);
    // per-site bounds of the packed planes (memc_pk.hpp): s = (the site's largest |gradoutput|) x (its largest |tap|),
    // published per wave and handed over by the barrier inside tile_bbox
    int sbits[4] = {0, 0, 0, 0}, gbits[4] = {0, 0, 0, 0}, tmax = 0;
    if (PART != 2) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int mg = 0, mt = 0;
#pragma unroll
            for (int c = 0; c < 3; c++) mg = max(mg, __float_as_int(go[c][j]) & 0x7FFFFFFF);
#pragma unroll
            for (int k = 0; k < 16; k++) mt = max(mt, __float_as_int(tp[k][j]) & 0x7FFFFFFF);
            const float sv = __int_as_float(mg) * __int_as_float(mt);
            gbits[j] = mg;
            tmax = max(tmax, ((g.valid >> j) & 1u) ? mt : 0);
            // (Inf x 0 = NaN: not finite, per-site atomics put it where the reference does; a zero bound adds nothing)
            sbits[j] = (mg >= 0x7F800000 || mt >= 0x7F800000) ? 0x7FC00000 : __float_as_int(sv);
        }
        pk_tile_publish(mx, tid, sbits, gbits, g.valid, tmax);
    }
    const BBox box = tile_bbox<LX, NT>(cmin, cmax, rmin, rmax, bb);
    const Bands bands = make_bands<LX, true, PG::kCap>(box);
    PkTile ps;
    ps.sa = ps.sb = 1.0f;  ps.inv = 1.0;  ps.limit = -1.0f;  ps.any = 0;
    if (PART != 2) ps = pk_tile_resolve<NT / kWave>(mx);
    // packed: the site's image gradient goes through the planes; outl: per-site global atomics (a bound beyond the tile's
    // block exponent, or an Inf / NaN among the site's inputs -- which then land exactly where the reference puts them)
    const unsigned packed = PART != 2 ? pk_packed_sites(ps, sbits, g.valid) : 0u;
    const unsigned outl = PART != 2 ? pk_outlier_sites(ps, sbits, g.valid) : 0u;
    const int mode = ps.any;                   // 0: no packed site has anything to add (workgroup-uniform)
    const st_t<I> *in_b = in1 + b * s1b;
    float *gin1_b = gin1 + b * s1b;
    unsigned done = 0;
    trace_mark<TR>(2);                                         // bounding box known
    if (PART != 1) fi_bwd_zero_invalid<P, FT>(inb, g.valid, gin2_b, s2c, o2, gin3_b, s3c, o3);
    // one site from global memory: the fp32 kernel's named functions, or their half instantiations (memc_fi.hpp)
    auto image_atomics = [&](unsigned todo) {  // outlier sites
        while (todo) {
            const int j = __ffs(todo) - 1;
            todo &= todo - 1;
            MEMC_SITE_IMAGE_ATOMICS(j);
        }
    };
    auto phase1 = [&](const Region &r, unsigned fast) {
        fi_bwd_phase1<P, FT>(r, fast, g, tp, go, tile, W, H, gin2_b, s2c, o2, gin3_b, s3c, o3);
        if (fast != 0xFu) {                    // mixed quads (rare): their tap gradients, site by site
            unsigned todo = fast;
            while (todo) {
                const int j = __ffs(todo) - 1;
                todo &= todo - 1;
                MEMC_SITE_TAPS(j);
            }
        }
    };
#pragma unroll 1
    for (int bi = 0; bi < bands.n; bi++) {
    const Region r = band_region(box, bands, bi, RAG ? W : 0);
    const unsigned fast = inb ? fi_covered(r, g, W, H) & ~done : 0u;
    // later bands run only if some site still needs them; the vote is also the barrier that frees the LDS
    if (bi > 0 && !__syncthreads_or(fast != 0)) continue;
    done |= fast;
    const StageSlot sl = stage_slots<NT>(r);
    // the image box: fp32 quads, or half quads as two packed dwords (widened when they are written to the LDS)
    StageRegsOf<I> sr;
    if (PART != 1) fi_bwd_stage_load<I, RAG>(r, sl, in_b, s1c, s1h, sr);   // in flight during adds and flush
    if (PART != 2 && mode == 1) {
        if (bi > 0) {                      // (band 0: zeroed at the top, ordered by the barrier of tile_bbox)
            zero_planes(r.h * r.pitch);
            __syncthreads();
        }
        // (a mixed image keeps fp32 staging registers beside the half kernel's 64-bit store addresses: with the scaled
        // gradoutput -- 12 products -- hoisted out of the band loop as well, the whole backward spills; opaque scales
        // keep the products inside the loop)
        float sa = ps.sa, sb = ps.sb;
        if constexpr (!std::is_same_v<I, P>) asm volatile("" : "+v"(sa), "+v"(sb));
        fi_bwd_adds_pk(r, fast & packed, g, tp, go, sa, sb, accA, accB, W, H);
        __syncthreads();
        if (bi == 0) trace_mark<TR>(3);                    // accumulated
        if (PART != 1) fi_bwd_stage_touch<I>(sr);      // the staged rows have landed long ago: take the wait
                                                           // here, not behind the flush's atomics
        pk_flush<NT>(r, accA, accB, ps.inv, gin1_b, s1c, s1h);
        if (PART != 1) __syncthreads();    // the planes have been read: the LDS becomes the image
        if (bi == 0) trace_mark<TR>(4);                    // flushed
    }
    if (PART != 2 && (fast & outl)) image_atomics(fast & outl);
    if (PART != 1) {
        fi_bwd_stage_store<I, RAG>(r, sl, sr, tile);
        __syncthreads();
        if (bi == 0) trace_mark<TR>(5);                    // image staged
        phase1(r, fast);
        if (bi == 0) trace_mark<TR>(6);                    // phase 1 done (this wave)
    }
    }   // bands
    trace_mark<TR>(12);
    unsigned slow = inb ? g.valid & ~done : 0u;            // not coverable within kMaxBands bands
    while (slow) {                            // rare: redone from global memory with global atomics
        const int j = __ffs(slow) - 1;
        slow &= slow - 1;
        // PART 0 and PART 2 sum gradinput2 in different orders (fi_bwd_site_scalar vs fi_bwd_site_taps): the half
        // kernels take the one the fp32 library takes for the same call
        static_assert(kF32 || PART != 1, "half storage: PART 0 or 2");
        if (PART == 0) MEMC_SITE_SCALAR(j);
        else if (PART == 1) MEMC_SITE_IMAGE_ATOMICS(j);
        else MEMC_SITE_TAPS(j);
    }
#undef MEMC_SITE_3WAY
#undef MEMC_SITE_TAPS
#undef MEMC_SITE_SCALAR
#undef MEMC_SITE_IMAGE_ATOMICS_ARGS
#undef MEMC_SITE_IMAGE_ATOMICS
}
