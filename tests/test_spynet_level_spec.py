"""The premises of tests/test_gpu_spynet_level.py, proved on the CPU (tests/_spynet_spec.py has the rule and the cases):

(a) the float64 direct formula and torch's own float64 expression -- the layer's composed route: interpolate, pad,
    normalise, add the linspace grid, grid_sample, cat -- agree to 1e-9 on the ordinary cases for both `align_sample`
    values: computing the sample position directly is the same function as torch's normalise / un-normalise round trip;
(b) on the exact cases (pixels k / 16, integer coarse flows, flags (0, 1)) the fp32 restatement equals the float64 direct
    formula bit for bit and `up` equals torch's float64 `up` bit for bit: there the GPU tests may ask for equality;
(c) on the ordinary cases the fp32 restatement, and torch's own fp32 expression, satisfy tests/_parity.close's rule against
    float64 (1e-4), with the worst error printed.  Measured: 0.8e-6 to 1.8e-5 for either under (0, 0) and (0, 1); under
    (1, 1) up to 8.9e-5 (restatement) and 9.5e-5 (torch), because an align_corners source index is a rounded product whose
    half ulp is multiplied by the step between two coarse flows (up to 20 px here) and then by the image's gradient.  The
    GPU tests hold the kernel's warp to the direct formula on the kernel's OWN `up`, which leaves the position's rounding only;
(d) a census per case: sites with 0, 1, 2 or 4 corners inside, sites in the padded row or column, the kernel family.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _parity            # noqa: E402
import _spynet_spec as S  # noqa: E402

from my_package.functions.SpyNetLevelLayer import SpyNetLevelLayer      # noqa: E402  (CPU tensors: the torch expression)


def torch_expression(case, flags, dtype):
    first, second, coarse = (torch.from_numpy(a).to(dtype) for a in case)
    return SpyNetLevelLayer(*flags)(first, second, coarse).numpy()


@pytest.mark.parametrize("flags", S.FLAGS)
@pytest.mark.parametrize("shape", S.SHAPES)
def test_direct_position_is_torch_s_function_in_float64(shape, flags):
    case = S.ordinary_case(shape)
    want = torch_expression(case, flags, torch.float64)
    got = S.level(*case, *flags, np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape == (shape[0], 8, shape[1], shape[2])
    assert np.array_equal(got[:, 0:3], want[:, 0:3])
    err_up, err_warp = np.abs(got[:, 6:8] - want[:, 6:8]).max(), np.abs(got[:, 3:6] - want[:, 3:6]).max()
    print(shape, flags, "float64 direct - torch float64: up %.3g, warp %.3g" % (err_up, err_warp))
    assert err_up <= 1e-9 and err_warp <= 1e-9


@pytest.mark.parametrize("shape", S.SHAPES)
def test_exact_cases_are_exact_in_fp32(shape):
    case = S.exact_case(shape)
    f32, f64 = S.level(*case, *S.EXACT_FLAGS, np.float32), S.level(*case, *S.EXACT_FLAGS, np.float64)
    assert f32.dtype == np.float32
    assert np.array_equal(f32.astype(np.float64), f64)
    want = torch_expression(case, S.EXACT_FLAGS, torch.float64)
    assert np.array_equal(f32[:, 6:8].astype(np.float64), want[:, 6:8])
    assert np.array_equal(f32[:, 0:3].astype(np.float64), want[:, 0:3])
    # `up` is a multiple of 1/8 and the warp is not trivially zero
    assert np.array_equal(f64[:, 6:8] * 8, np.round(f64[:, 6:8] * 8))
    assert np.abs(f64[:, 3:6]).max() > 0
    # torch's float64 warp agrees too (to rounding of its normalised grid, not bit for bit)
    assert np.abs(f64[:, 3:6] - want[:, 3:6]).max() <= 1e-9


@pytest.mark.parametrize("flags", S.FLAGS)
@pytest.mark.parametrize("shape", S.SHAPES)
def test_fp32_evaluations_satisfy_the_parity_rule(shape, flags):
    case = S.ordinary_case(shape)
    want = S.level(*case, *flags, np.float64)
    ours = S.level(*case, *flags, np.float32)
    torchs = torch_expression(case, flags, torch.float32)
    e1 = _parity.close(ours.astype(np.float64), want, "fp32 restatement vs float64 %s %s" % (shape, flags))
    e2 = _parity.close(torchs.astype(np.float64), want, "torch fp32 expression vs float64 %s %s" % (shape, flags))
    print(shape, flags, "worst error against float64: fp32 restatement %.3g, torch fp32 %.3g" % (e1, e2))


@pytest.mark.parametrize("shape", S.SHAPES)
def test_census(shape):
    B, H, W = shape
    for flow in ("normal", "zero", "pan"):
        _first, _second, coarse = S.ordinary_case(shape, flow)
        for flags in S.FLAGS:
            c = S.census(coarse, H, W, *flags)
            print(shape, flow, flags, c)
            assert c["sites"] == B * H * W == sum(c["corners_%d" % k] for k in (0, 1, 2, 3, 4))
            assert c["corners_3"] == 0                     # an axis-aligned 2 x 2 cell has 0, 1, 2 or 4 corners inside
            assert c["padded"] == B * (H * W - (H // 2 * 2) * (W // 2 * 2))
            assert c["family"] == {40: "spynet_level:quad", 8: "spynet_level:quad"}.get(W, "spynet_level:direct")
            if flow == "pan":
                assert c["corners_0"] == c["sites"]
            if flow == "zero" and flags[1] == 1:
                # the sample sits on the pixel: the cell's far corners fall outside in the last row and column only
                assert c["corners_4"] == B * (H - 1) * (W - 1) and c["corners_0"] == 0
            if flow == "normal":
                assert 0 < c["corners_0"] < c["sites"] and c["corners_4"] > 0
                assert c["corners_2"] > 0 or c["sites"] < 64       # (a 6 x 5 image with a flow of sigma 4 has few edge cells)
    # the exact cases reach every class as well
    c = S.census(S.exact_case(shape)[2], H, W, *S.EXACT_FLAGS)
    print(shape, "exact", c)
    assert c["corners_4"] > 0 and c["corners_0"] + c["corners_1"] + c["corners_2"] > 0
