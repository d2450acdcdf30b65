"""The SPyNet pyramid-level kernels (libmemc_hip_spynet.so, my_lib_spynet, SpyNetLevelLayer) on the device.

Shapes (tests/_spynet_spec.SHAPES): 24 x 40 (the quad kernel), 25 x 40 (the quad kernel with a padded row), 26 x 42 (the
direct kernel), 33 x 49 (padded row and column), 8 x 8 (the smallest quad width), 6 x 5 (a width below 8); each under the
flag pairs (align_upsample, align_sample) = (0, 0), (1, 1), (0, 1) and with a coarse flow N(0, 4^2), zero, and a pan of 1e9
in x.  The rule (tests/_spynet_spec.check_level; its premises are proved in tests/test_spynet_level_spec.py):

    out[:, 0:3]  torch.equal to `first`
    out[:, 6:8]  within tests/_parity.close of torch's float64 expression; on the exact cases equal bit for bit
    out[:, 3:6]  within tests/_parity.close of the float64 direct formula evaluated on the kernel's own `up`; on the exact
                 cases equal bit for bit

`out` is pre-filled with NaN: every element must have been written.  At zero flow with align_sample = 1 the warp is
`second` itself; under the 1e9 pan it is all zeros while `first` and `up` are still right.
"""
import os
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

pytestmark = pytest.mark.gpu


def LIB():
    import my_package._ext.my_lib_spynet as M
    return M


def layer(flags):
    from my_package.functions.SpyNetLevelLayer import SpyNetLevelLayer
    return SpyNetLevelLayer(*flags)


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(case, flags):
    """the entry point on a NaN-filled `out`: (result as numpy, the kernel family it took)"""
    first, second, coarse = (D(a) for a in case)
    out = torch.full((first.size(0), 8, first.size(2), first.size(3)), float("nan"), device="cuda")
    assert LIB().SpyNetLevelLayer_gpu_forward(first, second, coarse, out, *flags) == 0
    path = LIB().last_kernel_path()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not np.isnan(got).any(), "an element of out was not written"
    return got, path


@pytest.mark.parametrize("flags", S.FLAGS)
@pytest.mark.parametrize("shape", S.SHAPES)
def test_level_against_the_float64_rule(shape, flags):
    for flow in ("normal", "zero", "pan"):
        case = S.ordinary_case(shape, flow)
        got, path = run(case, flags)
        assert path == S.census(case[2], shape[1], shape[2], *flags)["family"] == S.family(shape[2])
        e_up, e_warp = S.check_level(got, case, flags, "%s %s %s" % (shape, flags, flow))
        print(shape, flags, flow, path, "worst error: up %.3g, warp %.3g" % (e_up, e_warp))
        if flow == "zero":
            assert not got[:, 6:8].any()
            if flags[1]:
                assert np.array_equal(got[:, 3:6], case[1])            # the sample sits on the pixel
        if flow == "pan":
            assert not got[:, 3:6].any()                               # every corner is outside
        # the layer: the same call through the public interface, the same bits
        with torch.no_grad():
            via_layer = layer(flags)(*(D(a) for a in case))
        assert LIB().last_kernel_path() == path
        assert np.array_equal(via_layer.cpu().numpy(), got)


@pytest.mark.parametrize("shape", S.SHAPES)
def test_exact_cases_bit_for_bit(shape):
    case = S.exact_case(shape)
    got, path = run(case, S.EXACT_FLAGS)
    assert path == S.family(shape[2])
    S.check_level(got, case, S.EXACT_FLAGS, "exact %s" % (shape,), exact=True)
    # and the whole result is the fp32 restatement's
    assert np.array_equal(got, S.level(*case, *S.EXACT_FLAGS, np.float32))


def test_non_finite_flows_stay_inside_second():
    """NaN, +-inf and huge coarse flows (the position is clamped, NaN included, before it becomes an int: no address outside
    `second` can be formed): `first` is copied, and every site whose `up` is what it is without them has the same warp"""
    shape = (1, 24, 40)
    first, second, coarse = S.ordinary_case(shape)
    bad = coarse.copy()
    bad[0, 0, 2, 3], bad[0, 1, 5, 7], bad[0, 0, 8, 11], bad[0, 1, 9, 1] = np.nan, np.inf, -np.inf, 3e38
    for flags in S.FLAGS:
        want, _ = run((first, second, coarse), flags)
        got, _ = run_allowing_nan((first, second, bad), flags)
        assert np.array_equal(got[:, 0:3], first)
        same_up = np.broadcast_to((got[:, 6:8] == want[:, 6:8]).all(axis=1, keepdims=True), (1, 3, 24, 40))
        assert np.array_equal(got[:, 3:6][same_up], want[:, 3:6][same_up])
        assert 0 < (~same_up).sum() < same_up.size


def run_allowing_nan(case, flags):
    first, second, coarse = (D(a) for a in case)
    out = torch.zeros((first.size(0), 8, first.size(2), first.size(3)), device="cuda")
    assert LIB().SpyNetLevelLayer_gpu_forward(first, second, coarse, out, *flags) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), LIB().last_kernel_path()


@pytest.mark.parametrize("shape", [(2, 25, 40), (1, 33, 49)])
def test_padded_stride_views_give_the_contiguous_call_s_bits(shape):
    B, H, W = shape
    case = S.ordinary_case(shape)
    first, second, coarse = (D(a) for a in case)
    wide_f = torch.full((B, 3, H + 1, W + 3), 7.0, device="cuda")
    wide_s = torch.full((B, 3, H + 2, W + 5), -7.0, device="cuda")
    wide_f[:, :, :H, 1:W + 1] = first
    wide_s[:, :, 1:H + 1, 3:W + 3] = second
    vf, vs = wide_f[:, :, :H, 1:W + 1], wide_s[:, :, 1:H + 1, 3:W + 3]
    assert not vf.is_contiguous() and vf.stride(3) == 1 and vs.stride(2) == W + 5
    for flags in S.FLAGS:
        with torch.no_grad():
            want = layer(flags)(first, second, coarse)
            path = LIB().last_kernel_path()
            got = layer(flags)(vf, vs, coarse)
        assert LIB().last_kernel_path() == path == S.family(W)
        assert torch.equal(got, want)
    assert float(wide_f[:, :, H].min()) == 7.0 and float(wide_s[:, :, 0].max()) == -7.0    # the views' surroundings: untouched


def test_a_declined_call_takes_the_torch_expression():
    """a w-stride of 2: the library declines, the layer composes -- the same rule, by torch"""
    shape = (2, 24, 40)
    case = S.ordinary_case(shape)
    first, second, coarse = (D(a) for a in case)
    wide = torch.zeros((2, 3, 24, 80), device="cuda")
    wide[..., ::2] = second
    from my_package.functions.SpyNetLevelLayer import _composed
    with torch.no_grad():
        layer((0, 0))(first, second, coarse)
        assert LIB().last_kernel_path() == "spynet_level:quad"
        out = torch.empty((2, 8, 24, 40), device="cuda")
        assert LIB().SpyNetLevelLayer_gpu_forward(first, wide[..., ::2], coarse, out, 0, 0) == 1
        assert LIB().SpyNetLevelLayer_gpu_forward(first, second, coarse, out[:, :, :, :], 0, 0) == 0
        assert LIB().SpyNetLevelLayer_gpu_forward(out[:, 0:3], second, coarse, out, 0, 0) == 1      # out over an input
        got = layer((0, 0))(first, wide[..., ::2], coarse)
        assert torch.equal(got, _composed(first, wide[..., ::2], coarse, False, False))
    S.check_level(got.cpu().numpy(), case, (0, 0), "declined call, composed")


def test_a_call_that_needs_gradients_keeps_autograd():
    """no backward kernel: with gradients wanted the layer runs the torch expression -- the path string stays, gradients exist"""
    from my_package.functions.SpyNetLevelLayer import SpyNetLevelLayer, _composed
    quad, direct = S.ordinary_case((2, 24, 40)), S.ordinary_case((2, 26, 42))
    with torch.no_grad():
        layer((0, 0))(*(D(a) for a in quad))
    assert LIB().last_kernel_path() == "spynet_level:quad"
    first, second, coarse = (D(a).requires_grad_(True) for a in direct)
    out = SpyNetLevelLayer()(first, second, coarse)
    assert LIB().last_kernel_path() == "spynet_level:quad"             # the direct-width call did not reach the library
    assert out.requires_grad and torch.equal(out, _composed(first, second, coarse, False, False))
    out.square().sum().backward()
    for t in (first, second, coarse):
        assert t.grad is not None and t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all())
    assert float(coarse.grad.abs().max()) > 0
    # the same tensors under no_grad do reach it, and `fused = False` keeps every call away from it
    with torch.no_grad():
        SpyNetLevelLayer()(first, second, coarse)
        assert LIB().last_kernel_path() == "spynet_level:direct"
        off = SpyNetLevelLayer()
        off.fused = False
        off(*(D(a) for a in quad))
        assert LIB().last_kernel_path() == "spynet_level:direct"
    # autocast and other dtypes: the torch expression
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        SpyNetLevelLayer()(*(D(a) for a in quad))
    assert LIB().last_kernel_path() == "spynet_level:direct"
    with torch.no_grad():
        half = SpyNetLevelLayer()(*(D(a).half() for a in quad))
    assert half.dtype == torch.float16 and LIB().last_kernel_path() == "spynet_level:direct"
