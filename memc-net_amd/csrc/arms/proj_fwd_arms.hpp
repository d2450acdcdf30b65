// arms/proj_fwd_arms.hpp -- MEASUREMENT BUILD ONLY.  Textually included by flow_projection.hip under MEMC_MEASURE, behind
// run_proj_fwd and the launch functions of the product's kernels; never part of libmemc_hip.so.
//   launch_proj_owner ... launch_proj_fillhole_carry   the launch functions of the superseded kernels (proj_owner_arms.hpp)
//   proj_arm_run         one arm's sequence of launches
//   proj_fwd_arm_launch  the forward launcher's table of A/B, timing and geometry arms (memc_debug_set_projection_variant)
#ifndef MEMC_MEASURE
#error "measurement arms: build with -DMEMC_MEASURE (make measure)"
#endif

template <bool DEPTH, int REACH, bool TRACE>
static void launch_proj_owner(const ProjFwdCall &a, const ProjRun &r)
{
    hipLaunchKernelGGL((proj_owner<DEPTH, REACH, TRACE>), dim3(r.ntiles), dim3(256), 0, a.stream, a.w, a.h, r.ntx, r.nty, a.s1.b,
                       a.s1.c, a.s1.h, a.sd.b, a.sd.h, a.sc.b, a.sc.h, a.flow, a.depth, a.count, a.out, r.flag, r.ws);
}

template <bool DEPTH, int TH, int ABL, bool TRACE>
static void launch_proj_owner2(const ProjFwdCall &a, const ProjRun &r)
{
    hipLaunchKernelGGL((proj_owner2<DEPTH, TH, 24, ABL, TRACE>), dim3(walk_grid(r.ntx, r.nty, a.batch, r.sw)), dim3(16 * TH), 0,
                       a.stream, a.w, a.h, r.ntx, r.nty, a.s1.b, a.s1.c, a.s1.h, a.sd.b, a.sd.h, a.sc.b, a.sc.h, a.flow, a.depth,
                       a.count, a.out, r.flag, r.ws, r.sw);
}

template <bool DEPTH>
static void launch_proj_owner3(const ProjFwdCall &a, const ProjRun &r)
{
    const unsigned npos = walk_grid(r.ntx, r.nty, a.batch, r.sw), pg = persistent_grid(2);
    hipLaunchKernelGGL((proj_owner3<DEPTH, 32, 24, 2>), dim3(npos < pg ? (npos + 7) / 8 * 8 : pg), dim3(512), 0, a.stream, a.w,
                       a.h, r.ntx, r.nty, npos, a.s1.b, a.s1.c, a.s1.h, a.sd.b, a.sd.h, a.sc.b, a.sc.h, a.flow, a.depth, a.count,
                       a.out, r.flag, r.ws, r.sw);
}

template <bool DEPTH, int TH, int MINW>
static void launch_proj_owner4(const ProjFwdCall &a, const ProjRun &r)
{
    hipLaunchKernelGGL((proj_owner4<DEPTH, TH, 24, MINW>), dim3(walk_grid(r.ntx, r.nty, a.batch, r.sw)), dim3(16 * TH), 0,
                       a.stream, a.w, a.h, r.ntx, r.nty, a.s1.b, a.s1.c, a.s1.h, a.sd.b, a.sd.h, a.sc.b, a.sc.h, a.flow, a.depth,
                       a.count, a.out, r.flag, r.bounds, r.ws, r.sw, r.nonce);
}

template <bool DEPTH, int TH>
static void launch_proj_owner_far_r3(const ProjFwdCall &a, const ProjRun &r)
{
    const unsigned pg = persistent_grid(1);
    hipLaunchKernelGGL((proj_owner_far_r3<DEPTH, TH, 24>), dim3(r.ntiles < pg ? r.ntiles : pg), dim3(16 * TH), 0, a.stream, a.w,
                       a.h, r.ntx, r.nty, a.batch, a.s1.b, a.s1.c, a.s1.h, a.sd.b, a.sd.h, a.sc.b, a.sc.h, a.flow, a.depth,
                       a.count, a.out, r.flag, r.bounds, r.ws, r.nonce);
}

template <int TH>
static void launch_proj_fill_summary(const ProjFwdCall &a, const ProjRun &r, unsigned grid, const int *flag)
{
    hipLaunchKernelGGL(proj_fill_summary<TH>, dim3(grid), dim3(256), 0, a.stream, a.w, a.h, r.ntx, r.nty, a.batch, a.sc.b,
                       a.sc.h, a.count, r.ws, flag);
}

// round 3's filler: workgroup i looks after the tiles i, i + grid, ... (one flag per lane of a wave)
template <int TH>
static void launch_proj_fillhole_carry(const ProjFwdCall &a, const ProjRun &r)
{
    const unsigned n = r.ntiles, fg = n < 4096u ? n : (n + 63u) / 64u > 4096u ? (n + 63u) / 64u : 4096u;
    hipLaunchKernelGGL(proj_fillhole_carry<TH>, dim3(fg), dim3(256), 0, a.stream, a.w, a.h, r.ntx, r.nty, a.batch, a.s1.b,
                       a.s1.c, a.s1.h, a.sc.b, a.sc.h, a.count, a.out, r.ws);
}

// One arm: v as proj_fwd_arm_launch decoded it, on 64 x TH owner tiles in stripes sw tile columns wide.  0 or -1.
// Three sets of kernels: the product's (with one piece swapped or left out), round 3's (proj_owner4 / proj_owner_far_r3 /
// proj_fillhole_carry: their own summaries and filler) and the owners of rounds 1-2 (0 / 1 flags cleared by a memset,
// flagged images redone by the general path queued behind the flag).  Several return WRONG results by construction.
// Keep the launches in this order: the order of first use is the order of the kernels in the code object.
// RAG: no arm runs on a ragged width; the instantiation is kept (proj_fwd_arm_launch) for the code object's sake.
template <bool DEPTH, int TH, bool RAG = false>
static int proj_arm_run(const ProjFwdCall &a, int sw, int v)
{
    const bool r3_set = v == -40 || v == -20;
    const bool legacy_owner = v == -10 || v == -7 || v == -6 || v == -30 || v == -31 || (v <= -21 && v >= -29);
    constexpr bool kNewOk = TH <= 32;                        // a column mask of proj_fill.hpp is one 32-bit word
    if (!kNewOk && !legacy_owner) return -1;
    const bool old_fill = r3_set || legacy_owner;
    ProjRun r;
    // 1 and the ablations from 2 on: no owner path; -8 / -9: the literal hole walker
    if (proj_resolve<TH>(a, sw, r, v != 1 && v < 2, v != -8 && v != -9, !old_fill) != 0) return -1;
    if (legacy_owner && r.base && hipMemsetAsync(r.base, 0, kProjWsHead * sizeof(int), a.stream) != hipSuccess) return -1;
    MEMC_PATH(r.flag ? (DEPTH ? "dproj_fwd:owner" : "proj_fwd:owner") : (DEPTH ? "dproj_fwd:general" : "proj_fwd:general"));
    constexpr int kMinW = owner_min_waves<DEPTH, TH>(false);
    [[maybe_unused]] constexpr int kMinWR = owner_min_waves<DEPTH, TH>(RAG);
    bool only_part = false, skip_pending = false;            // arms that time one piece
    const auto general = [&](unsigned grid, const int *flag, unsigned scatter_grid) {      // zero, scatter, average
        launch_proj_plane_pass(proj_redo_zero, a, grid, flag);
        launch_proj_scatter_tiled<DEPTH, 0>(a, r, flag, scatter_grid);
        launch_proj_plane_pass(proj_average_v4, a, grid, flag);
    };
    if (r.flag && !legacy_owner) {
        if constexpr (kNewOk) {
            if (r.nonce == 0) hipLaunchKernelGGL(proj_bump_nonce, dim3(1), dim3(1), 0, a.stream, r.flag);
            WalkPlan plan = make_walk_plan(r.ntx, r.nty, a.batch, sw);
            if (v == -43) plan.fast = 0;        // test arm: the kernel's own tile_walk (what grids beyond n * d < 2^32 take)
            only_part = v == -5 || v == -20 || v == -41;
            skip_pending = v == -42;            // timing arm: everything but proj_fill_pending (pending holes stay unfilled)
            if (r3_set) launch_proj_owner4<DEPTH, TH, kMinW>(a, r);
            // timing arm: 64-bit fixed-point planes on ds_add_u64 (proj_owner5.hpp, FIX64)
            else if (v == -46 && DEPTH) launch_proj_owner5<DEPTH, TH, kMinW, false, true>(a, r, plan);
            // how the motion estimate reaches the scan (proj_owner5.hpp, MOT):
            else if (v == -47) launch_proj_owner5<DEPTH, TH, kMinWR, false, false, RAG, 1>(a, r, plan);   // speculative m = 0 pass, samples by LDS DMA (round 6, lost)
            else if (v == -48) launch_proj_owner5<DEPTH, TH, kMinWR, false, false, RAG, 2>(a, r, plan);   // no estimate (timing arm)
            else if (v == -49) launch_proj_owner5<DEPTH, TH, kMinWR, false, false, RAG, 3>(a, r, plan);   // 16 samples, one lane each (timing arm)
            else if (v == -50) launch_proj_owner5<DEPTH, TH, kMinWR, false, false, RAG, 4>(a, r, plan);   // 16 samples through the scalar unit (timing arm)
            else if (v == -54) launch_proj_owner5<DEPTH, TH, kMinWR, false, false, RAG, 5>(a, r, plan);   // the estimate cached per image in the call's scratch
            // tiles with many holes leave ALL of them pending (proj_fill.hpp, PENDT):
            else if (v == -51) launch_proj_owner5<DEPTH, TH, kMinWR, false, false, RAG, 0, 0>(a, r, plan);    // every tile with a hole
            else if (v == -52) launch_proj_owner5<DEPTH, TH, kMinWR, false, false, RAG, 0, 8>(a, r, plan);    // more than 8 lanes with a hole
            else if (v == -53) launch_proj_owner5<DEPTH, TH, kMinWR, false, false, RAG, 0, 32>(a, r, plan);   // more than 32
            else if (v == -41) launch_proj_owner5<DEPTH, TH, kMinW, true>(a, r, plan);    // timestamps (tools/trace_kernel.py proj5)
            else launch_proj_owner5<DEPTH, TH, kMinWR, false, false, RAG>(a, r, plan);
            if (launch_status() != 0) return -1;
            if (g_proj_stall_us > 0) hipLaunchKernelGGL(proj_stall, dim3(1), dim3(64), 0, a.stream, g_proj_stall_us);
            if (!only_part) {
                if (r3_set) launch_proj_owner_far_r3<DEPTH, TH>(a, r);
                else launch_proj_owner_far<DEPTH, TH, RAG>(a, r);
                if (launch_status() != 0) return -1;
            }
        }
    } else if (r.flag) {
        const unsigned gq = 256 * 2;
        only_part = v == -7 || (v <= -21 && v >= -29);       // -21 .. -26: timing arms of proj_owner2 (wrong results); -7 / -29: timestamps
        if (v == -10 || v == -7 || v == -6) {                // round-1 owner kernel (64x16, strips)
            if (TH != 16) return -1;
            if (v == -7) launch_proj_owner<DEPTH, 24, true>(a, r);
            else if (v == -6) launch_proj_owner<DEPTH, 16, false>(a, r);
            else launch_proj_owner<DEPTH, 24, false>(a, r);
        }
        else if (v == -21) launch_proj_owner2<DEPTH, TH, 1, false>(a, r);
        else if (v == -22) launch_proj_owner2<DEPTH, TH, 2, false>(a, r);
        else if (v == -23) launch_proj_owner2<DEPTH, TH, 3, false>(a, r);
        else if (v == -24) launch_proj_owner2<DEPTH, TH, 4, false>(a, r);
        else if (v == -25) launch_proj_owner2<DEPTH, TH, 5, false>(a, r);
        else if (v == -26) launch_proj_owner2<DEPTH, TH, 6, false>(a, r);
        else if (v == -29) launch_proj_owner2<DEPTH, TH, 0, true>(a, r);
        else if (v == -30) launch_proj_owner2<DEPTH, TH, 0, false>(a, r);     // proj_owner2: LDS rings, three planes
        else if (v == -31 && TH == 32) launch_proj_owner3<DEPTH>(a, r);       // proj_owner3: persistent, next tile's fy prefetched
        else return -1;
        if (launch_status() != 0) return -1;
        if (!only_part) {
            general(gq, r.flag, r.sntiles > gq ? gq : r.sntiles);
            if (r.ws.up) launch_proj_fill_summary<TH>(a, r, gq, r.flag);      // summaries of the images the general path redid
            if (launch_status() != 0) return -1;
        }
    } else {
        const unsigned gs = 256 * 8;
        only_part = v >= 2;                     // (the ablation arms 2 / 3 time the scatter pass alone)
        if (v == 2) launch_proj_scatter_tiled<DEPTH, 2>(a, r, nullptr, r.sntiles);
        else if (v == 3) launch_proj_scatter_tiled<DEPTH, 3>(a, r, nullptr, r.sntiles);
        if (!only_part) {
            general(gs, nullptr, r.sntiles);
            if (r.ws.up && old_fill) launch_proj_fill_summary<TH>(a, r, gs, nullptr);
            else if (r.ws.up) {
                if constexpr (kNewOk) launch_proj_fill_masks<TH>(a, r, gs);
            }
        }
        if (launch_status() != 0) return -1;
    }
    if (a.fillhole && !only_part && !skip_pending) {
        if (r.ws.up && old_fill) launch_proj_fillhole_carry<TH>(a, r);
        else if (r.ws.up) {
            if constexpr (kNewOk) launch_proj_fill_pending<TH>(a, r);
        } else launch_proj_fillhole_v4(a, r, v == -8 ? 1 : 0);
        if (launch_status() != 0) return -1;
    }
    return 0;
}

// --------------------------------------------------------------------------------------------------
// The forward launcher's arms (memc_debug_set_projection_variant; tools/bench_ops.py --proj-variants, tools/trace_kernel.py)
// for a width of whole quads.  1: launched; 0: not an arm (the product's decision takes the call); -1: error.
//   100 + 10 * log2(TH / 16) + stripe width   the product's sequence (run_proj_fwd) in another owner geometry (TH 16 / 32)
//   400 + ...   round 3's production set (proj_owner4 + carry filler), same geometry code + 300
//   130 + ...   proj_owner2 (LDS rings, three planes), same geometry code + 30
//   160 + stripe width   proj_owner3 (persistent, TH = 32)
//   200 + 10 * arm + log2(TH / 16)   timing arms / timestamps of proj_owner2
//   -10 / -7 / -6   the round-1 owner (TH 16, strips);  the other negative ones, 1, 2, 3: proj_arm_run
// --------------------------------------------------------------------------------------------------
template <bool DEPTH>
static int proj_fwd_arm_launch(int variant, const ProjFwdCall &a)
{
    int v = variant, th = kOwnerTH, sw = kOwnerSW;
    const auto geometry = [&](int base, int arm) { th = 16 << ((v - base) / 10);  sw = (v - base) % 10;  v = arm; };
    if (v >= 100 && v < 120) geometry(100, -1);
    else if (v >= 400 && v < 420) geometry(400, -40);
    else if (v >= 130 && v < 160) geometry(130, -30);
    else if (v >= 160 && v < 170) geometry(150, -31);        // (TH = 32, stripe width v - 160)
    else if (v == -10 || v == -7 || v == -6) th = 16, sw = 0;
    else if (v >= 200 && v < 300) th = 16 << (v % 10), sw = 0, v = -(20 + (v - 200) / 10);
    (void)&proj_arm_run<DEPTH, kOwnerTH, true>;              // (never called: see proj_arm_run, RAG)
    int r;
    if (v == -1 && variant == -1) return 0;
    else if (v == -1) r = th == 16 ? run_proj_fwd<DEPTH, 16>(a, sw) : run_proj_fwd<DEPTH, 32>(a, sw);
    else if (th == 16) r = proj_arm_run<DEPTH, 16>(a, sw, v);
    else if (th == 64) r = proj_arm_run<DEPTH, 64>(a, sw, v);
    else r = proj_arm_run<DEPTH, 32>(a, sw, v);
    return r == 0 ? 1 : -1;
}
