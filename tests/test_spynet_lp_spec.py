"""The premises tests/test_gpu_spynet_level_lp.py leans on, proved on the CPU.

  * The exact cases of tests/_spynet_spec.exact_case are representable in float16 and in bfloat16 on every shape, so rounding
    the inputs to T changes nothing and the kernel's widened inputs are the case itself.
  * On those cases the float32 restatement of the rule equals the float64 one: the float32 value is exact, so "rounded to T
    once" is well defined -- it is `.to(T)` of that value, whatever the compiler contracts.
  * The host's family rule (W % 4 == 0, W >= 8, 8-byte bases and b / c / h strides % 4 of `first` and `out`), restated in
    tests/_spynet_lp_spec.family, gives the families the GPU file expects of its contiguous calls and of its views, and is
    what the source says.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd"), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _spynet_spec as S                   # noqa: E402
import _spynet_lp_spec as LP               # noqa: E402

import my_package._ext.my_lib_spynet_lp    # noqa: E402,F401   (the binding this file's premises are for)


@pytest.mark.parametrize("dtype", LP.DTYPES)
@pytest.mark.parametrize("shape", S.SHAPES)
def test_exact_cases_are_representable_and_their_float32_value_is_exact(shape, dtype):
    case, want32 = LP.exact_reference(shape)
    for a in case:
        t = torch.from_numpy(a)
        assert torch.equal(t.to(dtype).float(), t)
    want64 = S.level(*case, *S.EXACT_FLAGS, np.float64)
    assert want32.dtype == np.float32 and np.array_equal(want32.astype(np.float64), want64)
    # the result itself need not be representable (weights are multiples of 1/64): the single rounding has work to do
    if shape[1] * shape[2] > 64:
        r = torch.from_numpy(want32[:, 3:6])
        assert not torch.equal(r.to(torch.bfloat16).float(), r)


@pytest.mark.parametrize("dtype", LP.DTYPES)
def test_ordinary_cases_are_rounded_and_the_pan_is_finite(dtype):
    for flow in ("normal", "zero", "pan"):
        first, second, coarse = LP.ordinary_case((2, 24, 40), flow, dtype)
        assert first.dtype == second.dtype == coarse.dtype == dtype
        assert bool(torch.isfinite(coarse.float()).all())
    assert float(LP.ordinary_case((2, 24, 40), "pan", torch.float16)[2][0, 0, 0, 0]) == 65504.0
    assert float(LP.ordinary_case((2, 24, 40), "pan", torch.bfloat16)[2][0, 0, 0, 0]) > 9e8


def test_family_rule_on_the_cases_of_the_gpu_file():
    # contiguous calls from an aligned allocation: the float32 library's families
    for B, H, W in S.SHAPES:
        first = (0, (B, 3, H, W), (3 * H * W, H * W, W, 1))
        out = (0, (B, 8, H, W), (8 * H * W, H * W, W, 1))
        assert LP.family(W, first, out) == LP.contiguous_family(W), (B, H, W)
    assert [LP.contiguous_family(s[2]) for s in S.SHAPES] == [LP.QUAD, LP.QUAD, LP.DIRECT, LP.DIRECT, LP.QUAD, LP.DIRECT]
    # B == 1: the batch stride is not walked, so an odd one (33 x 49 has none that matters; 8 x 8 is 192) has no say
    assert LP.family(8, (0, (1, 3, 8, 8), (193, 64, 8, 1)), (0, (1, 8, 8, 8), (512, 64, 8, 1))) == LP.QUAD
    # the views: every allocation of torch's is at least 8-byte aligned, and so is one 8 bytes into it
    for shape in LP.VIEW_SHAPES:
        W = shape[2]
        for name, pad, offset, want in LP.VIEWS:
            for base in (0, 256, 512 + 8):
                got = LP.family(W, LP.view_geometry(shape, 3, pad, offset, base), LP.view_geometry(shape, 8, pad, offset, base))
                assert got == want, (shape, name, base)
    # either tensor alone breaks it; `second` and `coarse` are not asked
    shape = LP.VIEW_SHAPES[0]
    good_f, good_o = LP.view_geometry(shape, 3, 8, 4), LP.view_geometry(shape, 8, 8, 4)
    assert LP.family(40, good_f, good_o) == LP.QUAD
    assert LP.family(40, LP.view_geometry(shape, 3, 8, 1), good_o) == LP.DIRECT
    assert LP.family(40, good_f, LP.view_geometry(shape, 8, 5, 0)) == LP.DIRECT
    assert LP.family(40, (4,) + good_f[1:], good_o) == LP.DIRECT          # a 4-byte base is not enough


def test_the_restated_rule_is_the_source_s():
    src = open(os.path.join(ROOT, "memc-net_amd", "csrc", "lp_spynet_level.hip")).read()
    assert re.search(r"const bool quad = W % 4 == 0 && W >= 8 && quad_ok\(first\) && quad_ok\(out\);", src)
    desc = open(os.path.join(ROOT, "memc-net_amd", "csrc", "memc_desc.hpp")).read()
    body = desc.split("inline bool quad_ok(const memc_tensor4 *t)")[1].split("\n}\n")[0]
    assert "t->size[i] > 1 && t->stride[i] % 4 != 0" in body and "i < 3" in body
    assert "reinterpret_cast<uintptr_t>(t->data) % 8 == 0" in body
