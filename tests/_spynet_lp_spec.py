"""tests/_spynet_lp_spec.py -- what the tests of the half-precision SPyNet pyramid-level kernel (include/memc_spynet_lp.h)
share beyond tests/_spynet_spec.py: the dtypes, the inputs rounded to them, the host's family rule restated, and the strided
views of `first` and `out` that the GPU file runs, each with the family it must take.

The rule of the GPU tests: `out` equals, bit for bit, the float32 library on the widened inputs followed by one `.to(T)` --
and, on the exact cases (tests/test_spynet_lp_spec.py proves them T-representable and their float32 value exact), the numpy
restatement `_spynet_spec.level(..., np.float32)` followed by `.to(T)`.
"""
import functools

import numpy as np
import torch

import _spynet_spec as S

DTYPES = (torch.float16, torch.bfloat16)
QUAD, DIRECT = "spynet_level_lp:quad", "spynet_level_lp:direct"


def family(W, first, out):
    """The host's rule (lp_spynet_level.hip): quad for widths that are a multiple of four from 8 on where `first` and `out`
    -- each (address in bytes, sizes, element strides) -- have 8-byte aligned bases and b / c / h strides that are multiples
    of four elements (a dimension of size 1 is not walked); direct otherwise.  `second` and `coarse` have no say."""
    def quad_ok(addr, sizes, strides):
        return addr % 8 == 0 and all(strides[i] % 4 == 0 for i in range(3) if sizes[i] > 1)
    return QUAD if W % 4 == 0 and W >= 8 and quad_ok(*first) and quad_ok(*out) else DIRECT


def contiguous_family(W):
    """a contiguous call from a fresh allocation: the float32 library's family, by its other name"""
    return {"spynet_level:quad": QUAD, "spynet_level:direct": DIRECT}[S.family(W)]


# Views of `first` [B, 3, H, W] and `out` [B, 8, H, W] inside wider buffers [B, C + 1, H + 1, W + pad] (so the batch, channel
# and row strides are all padded), starting `offset` elements into a row: (name, pad, offset, family at a width that is a
# multiple of four from 8 on).  An offset of four elements is 8 bytes: still quad.  An offset of one element breaks the 8-byte
# base, a row stride of W + 5 the stride rule.
VIEWS = (("offset 4, row stride W + 8", 8, 4, QUAD),
         ("offset 1, row stride W + 8", 8, 1, DIRECT),
         ("offset 0, row stride W + 5", 5, 0, DIRECT))
VIEW_SHAPES = ((2, 24, 40), (2, 25, 40))


def view_geometry(shape, channels, pad, offset, base=0):
    """(address, sizes, strides) of such a view in a buffer at byte address `base` (2-byte elements)"""
    B, H, W = shape
    row, plane = W + pad, (H + 1) * (W + pad)
    return base + 2 * offset, (B, channels, H, W), ((channels + 1) * plane, plane, row, 1)


def pan(dtype):
    """the pan of the ordinary cases: 1e9 in x, or the dtype's largest finite value where 1e9 is beyond it"""
    return min(1e9, float(torch.finfo(dtype).max))


def ordinary_case(shape, flow, dtype):
    """_spynet_spec.ordinary_case rounded to `dtype`: three CPU tensors of that dtype"""
    first, second, coarse = S.ordinary_case(shape, flow)
    if flow == "pan":
        coarse[:, 0] = pan(dtype)
    return tuple(torch.from_numpy(a).to(dtype) for a in (first, second, coarse))


@functools.lru_cache(maxsize=None)
def exact_reference(shape):
    """(the exact case as float32 numpy arrays, _spynet_spec.level(..., np.float32) on it): computed once per shape, shared,
    never written to"""
    case = S.exact_case(shape)
    return case, S.level(*case, *S.EXACT_FLAGS, np.float32)
