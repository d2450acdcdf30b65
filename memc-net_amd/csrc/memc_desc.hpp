// memc_desc.hpp -- the descriptor checks of the C ABIs (host code only): layer_api.cpp (include/memc_warp.h) and, through
// memc_fi_abi.hpp (the check sequences and predicates that only the satellite libraries share), the seven warp libraries
// among the ten satellites, listed there (the frame I/O libraries and the SSIM library check their own planes).  One contract: every
// check the reference performs (my_lib_cuda.c, cited where an entry point calls these) and, beyond it, what the kernels rely on --
// unit w strides, sizes and strides that fit the launchers' `int`, and the b/c/h strides of a tensor that a kernel
// indexes with ANOTHER tensor's strides (output / gradoutput / gradinput1 with input1's, gradinput2 with input2's,
// gradinput3 with input3's, exactly as my_lib_kernel.cu does).  The reference leaves those cases unchecked and silently
// reads / writes the wrong cells.  Each entry point keeps its own order of checks.
#pragma once

#include "memc_warp_lp.h"

#include <stdint.h>

namespace memc {

inline bool fits_int(const memc_tensor4 *t)
{
    for (int i = 0; i < 4; i++)
        if (t->size[i] < 0 || t->size[i] > INT32_MAX || t->stride[i] < 0 || t->stride[i] > INT32_MAX) return false;
    return true;
}

inline int64_t numel(const memc_tensor4 *t) { return t->size[0] * t->size[1] * t->size[2] * t->size[3]; }

// usable descriptor: sizes / strides fit the launcher ABI, unit w stride, non-null data unless empty
inline bool ok(const memc_tensor4 *t)
{
    return t && fits_int(t) && (t->stride[3] == 1 || t->size[3] <= 1) && (t->data || numel(t) == 0);
}

inline bool same_shape(const memc_tensor4 *a, const memc_tensor4 *b)
{
    return a->size[0] == b->size[0] && a->size[1] == b->size[1] && a->size[2] == b->size[2] && a->size[3] == b->size[3];
}

// same b/c/h strides (the kernels index `b` with `a`'s strides); the stride of a size-1 dimension is never used
inline bool same_layout(const memc_tensor4 *a, const memc_tensor4 *b)
{
    if (!same_shape(a, b)) return false;
    for (int i = 0; i < 3; i++)
        if (a->size[i] > 1 && a->stride[i] != b->stride[i]) return false;
    return true;
}

// flow [N, 2, H, W] matching input1 [N, C, H, W] (my_lib_cuda.c:375-381, :611-617, :685-691)
inline bool flow_matches(const memc_tensor4 *in1, const memc_tensor4 *flow)
{
    return flow->size[0] == in1->size[0] && flow->size[1] == 2 && flow->size[2] == in1->size[2] && flow->size[3] == in1->size[3];
}

// filter taps [N, K, H, W] matching input1 [N, C, H, W] (my_lib_cuda.c:611-617, :685-691)
inline bool taps_match(const memc_tensor4 *in1, const memc_tensor4 *filt)
{
    return filt->size[0] == in1->size[0] && filt->size[2] == in1->size[2] && filt->size[3] == in1->size[3];
}

// half-precision ABIs: an fp16 / bf16 payload; `other` (the flow, gradoutput) in fp32 or in the payload's type
inline bool dtypes_ok(memc_dtype payload, memc_dtype other)
{
    return (payload == MEMC_F16 || payload == MEMC_BF16) && (other == MEMC_F32 || other == payload);
}

// quads of four halves (the tiled half-precision kernels): strides of every dimension that is walked a multiple of four
// elements, 8-byte aligned base
inline bool quad_ok(const memc_tensor4 *t)
{
    for (int i = 0; i < 3; i++)
        if (t->size[i] > 1 && t->stride[i] % 4 != 0) return false;
    return reinterpret_cast<uintptr_t>(t->data) % 8 == 0;
}

}  // namespace memc
