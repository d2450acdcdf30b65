// arms/fi_fwd_arms.hpp -- MEASUREMENT BUILD ONLY.  Textually included by filter_interpolation.hip under MEMC_MEASURE, behind
// the forward kernels and their launch functions; never part of libmemc_hip.so.
//   fi_fwd_refshape    the reference-shaped forward (block 32 x 16, taps re-read per channel, no LDS): what a straight port
//                      gives on this chip (2130 us, 16.6 % of the HBM peak -- DESIGN.md section 4)
//   fi_fwd_arm_launch  the forward launcher's table of A/B and ablation arms
#ifndef MEMC_MEASURE
#error "measurement arms: build with -DMEMC_MEASURE (make measure)"
#endif
// --------------------------------------------------------------------------------------------------
// Measurement arm only (bench_ops.py): a kernel with the REFERENCE's structure -- block (32,16), one
// thread per site, taps re-read from global for every channel, no streaming hints, blockIdx-ordered
// tiles -- to show what a straight port achieves on MI355X.  Never selected by the product path.
// --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void fi_fwd_refshape(
    int W, int H, int C, int fs,
    int64_t s1b, int64_t s1c, int s1h, int64_t s2b, int64_t s2c, int s2h, int64_t s3b, int64_t s3c, int s3h,
    const float *in1, const float *flow, const float *filt, float *out)
{
    const int x = blockIdx.x * 32 + threadIdx.x;
    const int y = blockIdx.y * 16 + threadIdx.y;
    const int b = blockIdx.z;
    if (x >= W || y >= H) return;
    const float *flow_b = flow + b * s2b + (int64_t)y * s2h + x;
    const float fx = flow_b[0], fy = flow_b[s2c];
    const FiSite s = fi_locate(x, y, W, H, fx, fy);
    const float *tap_p = filt + b * s3b + (int64_t)y * s3h + x;
    const float *in_b = in1 + b * s1b;
    float *out_p = out + b * s1b + (int64_t)y * s1h + x;
    if (s.valid) {
        const int L = s.ix + 1 - fs / 2, T = s.iy + 1 - fs / 2, R = L + fs, Bm = T + fs;
        for (int c = 0; c < C; c++)
            out_p[c * s1c] = fi_site_chan(s, fs, L, T, R, Bm, W, H, in_b + c * s1c, s1h, tap_p, s3c);
    } else {
        const float *p = in_b + (int64_t)y * s1h + x;
        for (int c = 0; c < C; c++) out_p[c * s1c] = p[c * s1c];
    }
}

// --------------------------------------------------------------------------------------------------
// The forward launcher's A/B and ablation arms (memc_debug_set_fi_fwd_variant, tools/bench_ops.py); several return WRONG
// results by construction.  1: launched; 0: no arm for this shape (the product's decision takes the call); -1: launch error.
// Keep the launches in this order: the order of first use is the order of the kernels in the code object.
// --------------------------------------------------------------------------------------------------
static int fi_fwd_arm_launch(int variant, const FiFwdCall<> &k, bool vec)
{
    const int channel = k.channel;
    if (variant == 0) {  // reference-structure measurement arm
        dim3 block(32, 16, 1), grid((k.w + 31) / 32, (k.h + 15) / 16, k.batch);
        hipLaunchKernelGGL(fi_fwd_refshape, grid, block, 0, k.stream, k.w, k.h, channel, k.filter_size, k.s1.b, k.s1.c,
                           k.s1.h, k.s2.b, k.s2.c, k.s2.h, k.s3.b, k.s3.c, k.s3.h, k.in1, k.flow, k.filt, k.out);
    } else if (k.filter_size == 4 && variant >= 1 && variant <= 3) {      // force the scalar direct-gather kernels
        if (channel == 3) {
            if (variant == 2) launch_fi_fwd_direct_fs4<3, 8>(k);
            else if (variant == 3) launch_fi_fwd_direct_fs4<3, 2>(k);
            else launch_fi_fwd_direct_fs4<3, 4>(k);
        } else {
            if (variant == 2) launch_fi_fwd_direct_fs4<0, 8>(k);
            else if (variant == 3) launch_fi_fwd_direct_fs4<0, 2>(k);
            else launch_fi_fwd_direct_fs4<0, 4>(k);
        }
    } else if (k.filter_size != 4 || !vec || variant < 4) {
        return 0;
    } else if (variant == 5) {
        if (channel == 3) launch_fi_fwd_tiled_fs4<8, 3, 3, 0>(k); else launch_fi_fwd_tiled_fs4<8, 0, 3, 0>(k);
    } else if (variant == 6) {
        if (channel == 3) launch_fi_fwd_tiled_fs4<16, 3, 2, 0>(k); else launch_fi_fwd_tiled_fs4<16, 0, 2, 0>(k);
    } else if (variant == 7) {
        if (channel == 3) launch_fi_fwd_tiled_fs4<8, 3, 2, 0>(k); else launch_fi_fwd_tiled_fs4<8, 0, 2, 0>(k);
    } else if (variant == 4) {
        if (channel == 3) launch_fi_fwd_tiled_fs4<16, 3, 3, 0>(k); else launch_fi_fwd_tiled_fs4<16, 0, 3, 0>(k);
    } else if (channel == 3) {
        switch (variant) {
        case 8: launch_fi_fwd_tiled_fs4<16, 3, 2, 1>(k); break;
        case 11: launch_fi_fwd_tiled_fs4<16, 3, 3, 4>(k); break;
        case 15: launch_fi_fwd_tiled_fs4<16, 3, 2, 5>(k, 0, 2); break;             // stripes two tile columns wide
        case 16: launch_fi_fwd_tiled_fs4<16, 3, 2, 6>(k, 0, 4); break;             // ... four
        case 17: launch_fi_fwd_tiled_fs4<16, 3, 2, 4>(k, 0, 4); break;             // row-major chunk per XCD at 2 waves/SIMD
        case 26: launch_fi_fwd_tiled_fs4<16, 3, 2, 0, false, 3072, 1>(k); break;   // the product kernel with phased stores (memc_debug_set_fi_phase)
        // 20: 128 x 8 tiles (LX = 32) with a 4608-pixel budget, strips; 21: the same in hardware order; 22: 64 x 16 tiles
        // with a 4096-pixel budget (no band sweeps on i.i.d. flow); 23: 128 x 8 tiles on the product's 3072 pixels; 24 / 25:
        // 128 x 8 tiles on 3392 pixels (53 KiB: the most that leaves three workgroups per CU), registers for two / three
        case 20: launch_fi_fwd_tiled_fs4<32, 3, 2, 0, false, 4608>(k); break;
        case 21: launch_fi_fwd_tiled_fs4<32, 3, 2, 1, false, 4608>(k); break;
        case 22: launch_fi_fwd_tiled_fs4<16, 3, 2, 0, false, 4096>(k); break;
        case 23: launch_fi_fwd_tiled_fs4<32, 3, 2, 0, false, 3072>(k); break;
        case 24: launch_fi_fwd_tiled_fs4<32, 3, 2, 0, false, 3392>(k); break;
        case 25: launch_fi_fwd_tiled_fs4<32, 3, 3, 0, false, 3392>(k); break;
        default: return 0;
        }
    } else if (channel % 4 == 0 && channel >= 8) {
        switch (variant) {
        case 30: launch_fi_fwd_tiled_c4n<2>(k); break;
        case 31: launch_fi_fwd_tiled_c4n<4>(k); break;
        case 32: launch_fi_fwd_tiled_c4n<0, 512>(k); break;                // 64 x 32 tiles, 512 lanes
        case 35: launch_fi_fwd_tiled_c4n<4, 512>(k); break;                // ... in stripes four tile columns wide
        case 36: launch_fi_fwd_tiled_c4n<0, 256, false, 16, 1>(k); break;  // timing: no gathers
        case 37: launch_fi_fwd_tiled_c4n<0, 256, false, 16, 2>(k); break;  // timing: no image loads after the first chunk
        case 38: launch_fi_fwd_tiled_c4n<0, 512, false, 16, 1>(k); break;
        case 39: launch_fi_fwd_tiled_c4n<0, 512, false, 16, 2>(k); break;
        case 33: launch_fi_fwd_tiled_c4n<0, 256, false, 8>(k); break;      // 32 x 32 tiles: the box of a square tile is the least dilated
        case 34: launch_fi_fwd_tiled_c4n<4, 256, false, 8>(k); break;      // ... in stripes four tile columns wide
        default: return 0;
        }
    } else {
        return 0;
    }
    return launch_status() == 0 ? 1 : -1;
}
