// memc_lp.hpp -- half-width storage for the adaptive-warp forward of libmemc_hip_lp.so (lp_filter_interpolation.hip) and
// the RGB backward of libmemc_hip_lp_grad.so (lp_fi_bwd_c3.hip, memc_fi_bwd_c3.hpp).
//
// Numerics contract (include/memc_warp_lp.h):
//   * payload type T in {fp16, bf16}: the image / features, the filter taps, the occlusions (blend) and the output;
//   * the flow is fp32 or T, decoded in the kernel;
//   * every input is widened to fp32 exactly; the tap products, the quadrant sums and the bilinear blend are the fp32
//     kernels' (filter_interpolation.hip) in the same order;
//   * the output is rounded to T ONCE, round-to-nearest-even, overflow to +-inf -- exactly what `tensor.to(T)` does;
//   * sites outside the image copy the input pixel (widened and narrowed again: exact).
//
// The LDS image is the fp32 kernels' (memc_tile.hpp): one f32x4 pixel quad per pixel.  Only the global side narrows: a
// quad of four T is 8 bytes, so the tiled kernels need quads that are 8-byte aligned -- widths a multiple of four, row /
// channel / batch strides multiples of four elements, 8-byte aligned bases (the launcher checks; everything else takes
// the one-lane-per-site kernel).
#pragma once

#include "memc_tile.hpp"

#include <type_traits>

namespace memc {

// storage tags: the element type in memory and its exact widening / single rounding
struct F32 {
    using st = float;
};
struct F16 {
    using st = unsigned short;
};
struct BF16 {
    using st = unsigned short;
};
template <class S>
using st_t = typename S::st;

typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef u16x4 u16x4a __attribute__((aligned(8)));         // a quad of four halves in global memory: 8-byte aligned

template <class S> __device__ __forceinline__ float widen(st_t<S> v);
template <> __device__ __forceinline__ float widen<F32>(float v) { return v; }
template <> __device__ __forceinline__ float widen<F16>(unsigned short v) { return (float)__builtin_bit_cast(_Float16, v); }
template <> __device__ __forceinline__ float widen<BF16>(unsigned short v)
{
    return __builtin_bit_cast(float, (unsigned)v << 16);
}

// fp32 -> T, round-to-nearest-even, overflow to +-inf (v_cvt_f16_f32 / v_cvt_pk_bf16_f32)
template <class S> __device__ __forceinline__ st_t<S> narrow(float v);
template <> __device__ __forceinline__ float narrow<F32>(float v) { return v; }
template <> __device__ __forceinline__ unsigned short narrow<F16>(float v)
{
    return __builtin_bit_cast(unsigned short, (_Float16)v);
}
template <> __device__ __forceinline__ unsigned short narrow<BF16>(float v)
{
    return __builtin_bit_cast(unsigned short, (__bf16)v);
}

// fp32 -> T of a value that the fp32 kernels round to fp32 first (the backward of libmemc_hip_lp_grad.so).  For fp16 the
// empty asm keeps the compiler from folding the multiply or FMA that produced `v` into the conversion: v_fma_mixlo_f16
// rounds the exact result to fp16 once -- not the fp32 value, so an fp32 value that is an fp16 tie can round the other
// way (seen: one tap gradient in ~2000).  bf16 has no such fused form.
template <class S>
__device__ __forceinline__ st_t<S> narrow_f32(float v)
{
    if constexpr (std::is_same_v<S, F16>) asm volatile("" : "+v"(v));
    return narrow<S>(v);
}

// T -> fp32 as an opaque value (the per-site backward helpers, memc_fi.hpp): the compiler then sees an fp32 operand, as it
// does in the fp32 kernels, and cannot fold the conversion into a mixed-precision FMA (v_fma_mix_f32) -- which would fuse
// a multiply and an add that the fp32 code keeps apart, or keep apart ones it fuses (its vectoriser chooses differently).
template <class S>
__device__ __forceinline__ float widen_f32(st_t<S> v)
{
    float f = widen<S>(v);
    if constexpr (!std::is_same_v<S, F32>) asm volatile("" : "+v"(f));
    return f;
}

// a widened fp16 quad made opaque (the flow of the RGB backward): with the conversions in view the compiler vectorises the
// arithmetic that follows differently from the fp32 kernel's (other multiplies and adds end up fused); F32 / BF16: as is
template <class S>
__device__ __forceinline__ f32x4 opaque4(f32x4 v)
{
    if constexpr (std::is_same_v<S, F16>) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
    return v;
}

template <class S>
__device__ __forceinline__ f32x4 widen4(const u16x4 &q)
{
    return f32x4{widen<S>(q[0]), widen<S>(q[1]), widen<S>(q[2]), widen<S>(q[3])};
}

// quad loads, widened: streamed (non-temporal; flow, taps, occlusions) and cached (the image)
template <class S>
__device__ __forceinline__ f32x4 ld4_stream(const st_t<S> *p)
{
    if constexpr (sizeof(st_t<S>) == 4) return ld_stream4(reinterpret_cast<const float *>(p));
    else return widen4<S>(__builtin_nontemporal_load(reinterpret_cast<const u16x4a *>(p)));
}
template <class S>
__device__ __forceinline__ f32x4 ld4_cached(const st_t<S> *p)
{
    if constexpr (sizeof(st_t<S>) == 4) return ld_cached4(reinterpret_cast<const float *>(p));
    else return widen4<S>(*reinterpret_cast<const u16x4a *>(p));
}
// narrowed quad store (non-temporal: the output is single-use); F32: the quad as it is
template <class S>
__device__ __forceinline__ void st4_stream(st_t<S> *p, const f32x4 &v)
{
    if constexpr (sizeof(st_t<S>) == 4) {
        st_stream4(reinterpret_cast<float *>(p), v);
    } else {
        const u16x4 q = {narrow<S>(v[0]), narrow<S>(v[1]), narrow<S>(v[2]), narrow<S>(v[3])};
        __builtin_nontemporal_store(q, reinterpret_cast<u16x4a *>(p));
    }
}
// the same through wave-uniform base + 32-bit byte offset (ld_stream4_u / st_stream4_u of memc_tile.hpp; F32: those exactly);
// the store rounds fp32 values (see narrow_f32)
template <class S>
__device__ __forceinline__ f32x4 ld4_stream_u(const st_t<S> *ubase, unsigned byte_off)
{
    if constexpr (sizeof(st_t<S>) == 4) return ld_stream4_u(ubase, byte_off);
    else return widen4<S>(__builtin_nontemporal_load(reinterpret_cast<const MEMC_GLOBAL u16x4a *>(addr_u(ubase, byte_off))));
}
template <class S>
__device__ __forceinline__ void st4_stream_u(st_t<S> *ubase, unsigned byte_off, f32x4 v)
{
    if constexpr (sizeof(st_t<S>) == 4) {
        st_stream4_u(ubase, byte_off, v);
    } else {
        // the quad as a whole is the asm's operand: the compiler still sees one fp32 vector consumed, as by the fp32
        // store, and vectorises what computes it the same way (four scalar consumers -- narrow_f32 -- fuse differently)
        asm volatile("" : "+v"(v));
        const u16x4 q = {narrow<S>(v[0]), narrow<S>(v[1]), narrow<S>(v[2]), narrow<S>(v[3])};
        __builtin_nontemporal_store(q, reinterpret_cast<MEMC_GLOBAL u16x4a *>(addr_u(ubase, byte_off)));
    }
}

// Staging of NCH (1..4) T planes into the fp32 pixel-quad LDS image of memc_tile.hpp: the same slots and the same
// unconditional loads as tile_stage_load_planes (an empty slot reads the plane's first quad), 8 bytes per quad; widened
// when written to LDS.
template <int NCH>
struct LpStageRegs {
    uint2 v[kStageIts][NCH];               // a quad of four T as two packed dwords
};

// the two halves of a packed dword, widened
template <class S> __device__ __forceinline__ float widen_lo(unsigned w) { return widen<S>((unsigned short)(w & 0xFFFFu)); }
template <class S> __device__ __forceinline__ float widen_hi(unsigned w) { return widen<S>((unsigned short)(w >> 16)); }
template <> __device__ __forceinline__ float widen_lo<BF16>(unsigned w) { return __builtin_bit_cast(float, w << 16); }
template <> __device__ __forceinline__ float widen_hi<BF16>(unsigned w) { return __builtin_bit_cast(float, w & 0xFFFF0000u); }

template <int NCH>
__device__ __forceinline__ void lp_stage_load(const Region &r, const StageSlot &sl,
                                              const unsigned short *const (&plane)[NCH], int hstride, LpStageRegs<NCH> &sr)
{
#pragma unroll
    for (int it = 0; it < kStageIts; it++) {
        const bool on = sl.row[it] < r.h;
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const unsigned short *p = on ? plane[c] + (int64_t)(r.y0 + sl.row[it]) * hstride + r.x0 + 4 * sl.q[it] : plane[c];
            sr.v[it][c] = *reinterpret_cast<const uint2 *>(p);
        }
    }
}

template <class T, int NCH>
__device__ __forceinline__ void lp_stage_store(const Region &r, const StageSlot &sl, const LpStageRegs<NCH> &sr, f32x4 *tile)
{
#pragma unroll
    for (int it = 0; it < kStageIts; it++) {
        if (sl.row[it] < r.h) {
            f32x4 *dst = tile + sl.row[it] * r.pitch;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                f32x4 px = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int c = 0; c < NCH; c++) {
                    const unsigned wd = i < 2 ? sr.v[it][c].x : sr.v[it][c].y;
                    px[c] = (i & 1) ? widen_hi<T>(wd) : widen_lo<T>(wd);
                }
                dst[swz_col(4 * sl.q[it] + i)] = px;
            }
        }
    }
}

// Staging of an image of either storage: F32 planes through memc_tile.hpp's dword-aligned quads, T planes through the
// 8-byte quads above.  (The mixed kernels of libmemc_hip_mx.so: an fp32 image beside T taps.)
template <class S, int NCH>
using ImgStageRegs = std::conditional_t<sizeof(st_t<S>) == 4, StageRegs<NCH>, LpStageRegs<NCH>>;

template <class S, int NCH>
__device__ __forceinline__ void img_stage_load(const Region &r, const StageSlot &sl, const st_t<S> *const (&plane)[NCH],
                                               int hstride, ImgStageRegs<S, NCH> &sr)
{
    if constexpr (sizeof(st_t<S>) == 4) {
        int hs[NCH];
#pragma unroll
        for (int c = 0; c < NCH; c++) hs[c] = hstride;
        tile_stage_load_planes<NCH, false>(r, sl, plane, hs, sr);
    } else {
        lp_stage_load<NCH>(r, sl, plane, hstride, sr);
    }
}

template <class S, int NCH>
__device__ __forceinline__ void img_stage_store(const Region &r, const StageSlot &sl, const ImgStageRegs<S, NCH> &sr,
                                                f32x4 *tile)
{
    if constexpr (sizeof(st_t<S>) == 4) tile_stage_store<NCH, false>(r, sl, sr, tile);
    else lp_stage_store<S, NCH>(r, sl, sr, tile);
}

}  // namespace memc
