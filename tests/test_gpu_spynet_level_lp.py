"""The half-precision SPyNet pyramid-level kernels (libmemc_hip_spynet_lp.so, my_lib_spynet_lp, SpyNetLevelLayer.native_half,
SPyNet.fused_level_half) on the device.

The rule: `out` equals, BIT FOR BIT, the float32 library (libmemc_hip_spynet.so) on the widened inputs followed by one
`.to(T)`, the families corresponding (quad where the float32 call took quad, direct where it took direct); on the exact cases
(tests/test_spynet_lp_spec.py: T-representable, their float32 value exact) it equals the numpy restatement
`_spynet_spec.level(..., np.float32)` followed by `.to(T)`.  out[:, 0:3] has `first`'s bits.

Shapes (tests/_spynet_spec.SHAPES): 24 x 40 (quad), 25 x 40 (quad with a padded row), 26 x 42 (direct), 33 x 49 (padded row
and column), 8 x 8 (the smallest quad width), 6 x 5 (a width below 8); the flag pairs (0, 0), (1, 1), (0, 1); coarse flows
N(0, 4^2), zero, and a pan of 1e9 (float16: 65504, its largest finite value) in x; both dtypes.  `out` is pre-filled with NaN
patterns of T: every element must have been written.
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
import _spynet_lp_spec as LP               # noqa: E402

pytestmark = pytest.mark.gpu
IDS = {torch.float16: "fp16", torch.bfloat16: "bf16"}
dtypes = pytest.mark.parametrize("dtype", LP.DTYPES, ids=[IDS[d] for d in LP.DTYPES])


def LIB():
    import my_package._ext.my_lib_spynet_lp as M
    return M


def F32():
    import my_package._ext.my_lib_spynet as M
    return M


def bits(t):
    return t.contiguous().view(torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def nan_filled(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def run(case, flags, allow_nan=False):
    """the entry point on a NaN-filled `out`: (out, the kernel family it took)"""
    first, second, coarse = case
    out = nan_filled((first.size(0), 8, first.size(2), first.size(3)), first.dtype)
    assert LIB().SpyNetLevelLayer_gpu_forward_lp(first, second, coarse, out, *flags) == 0
    path = LIB().last_kernel_path()
    torch.cuda.synchronize()
    if not allow_nan:
        assert not bool(torch.isnan(out).any()), "an element of out was not written"
    return out, path


def run_f32(case, flags):
    """the float32 library on the widened inputs: (its result rounded once to the case's dtype, the family it took)"""
    first, second, coarse = (t.float() for t in case)
    out = torch.full((first.size(0), 8, first.size(2), first.size(3)), float("nan"), device="cuda")
    assert F32().SpyNetLevelLayer_gpu_forward(first, second, coarse, out, *flags) == 0
    path = F32().last_kernel_path()
    torch.cuda.synchronize()
    return out.to(case[0].dtype), path


@dtypes
@pytest.mark.parametrize("flags", S.FLAGS)
@pytest.mark.parametrize("shape", S.SHAPES)
def test_level_is_the_float32_library_s_rounded_once(shape, flags, dtype):
    for flow in ("normal", "zero", "pan"):
        case = tuple(t.cuda() for t in LP.ordinary_case(shape, flow, dtype))
        got, path = run(case, flags)
        want, path32 = run_f32(case, flags)
        what = "%s %s %s %s" % (shape, flags, flow, dtype)
        assert path == path32.replace("spynet_level:", "spynet_level_lp:") == LP.contiguous_family(shape[2]), what
        assert same_bits(got[:, 0:3], case[0]), what + ": first"
        diff = got.float() != want.float()
        assert torch.equal(got, want), what + ": %d elements differ, channels %s" % (
            int(diff.sum()), sorted(set(torch.nonzero(diff)[:, 1].tolist())))
        if flow == "zero":
            assert not bool(got[:, 6:8].any())
            if flags[1]:
                assert same_bits(got[:, 3:6], case[1])                 # the sample sits on the pixel
        if flow == "pan":
            assert not bool(got[:, 3:6].any())                         # every corner is outside


@dtypes
@pytest.mark.parametrize("shape", S.SHAPES)
def test_exact_cases_bit_for_bit(shape, dtype):
    case32, want32 = LP.exact_reference(shape)
    case = tuple(torch.tensor(a).to(dtype).cuda() for a in case32)
    got, path = run(case, S.EXACT_FLAGS)
    assert path == LP.contiguous_family(shape[2])
    want = torch.tensor(want32).to(dtype)
    assert torch.equal(got.cpu(), want)
    assert same_bits(got[:, 0:3], case[0])


def wide_view(t, channels, pad, offset, fill):
    """`t` [B, channels, H, W] copied into a view of a wider buffer [B, channels + 1, H + 1, W + pad] filled with `fill`,
    `offset` elements into each row: (buffer, view)"""
    B, _c, H, W = t.shape
    buf = torch.full((B, channels + 1, H + 1, W + pad), fill, dtype=t.dtype, device="cuda")
    view = buf[:, :channels, :H, offset:offset + W]
    view.copy_(t)
    return buf, view


@dtypes
@pytest.mark.parametrize("shape", LP.VIEW_SHAPES)
def test_views_take_their_family_and_give_the_same_bits(shape, dtype):
    B, H, W = shape
    case32, want32 = LP.exact_reference(shape)
    first, second, coarse = (torch.tensor(a).to(dtype).cuda() for a in case32)
    want = torch.tensor(want32).to(dtype).cuda()
    for name, pad, offset, family in LP.VIEWS:
        fbuf, vf = wide_view(first, 3, pad, offset, 7.0)
        obuf, vo = wide_view(nan_filled((B, 8, H, W), dtype), 8, pad, offset, float("nan"))
        assert vf.stride() == LP.view_geometry(shape, 3, pad, offset)[2] and vf.stride(0) > 3 * H * (W + pad)
        assert vo.stride() == LP.view_geometry(shape, 8, pad, offset)[2]
        assert vf.data_ptr() == fbuf.data_ptr() + 2 * offset and fbuf.data_ptr() % 8 == 0 and obuf.data_ptr() % 8 == 0
        assert LP.family(W, (vf.data_ptr(), vf.shape, vf.stride()), (vo.data_ptr(), vo.shape, vo.stride())) == family
        assert LIB().SpyNetLevelLayer_gpu_forward_lp(vf, second, coarse, vo, *S.EXACT_FLAGS) == 0
        assert LIB().last_kernel_path() == family, name
        torch.cuda.synchronize()
        assert torch.equal(vo, want), name
        # the views' surroundings: untouched
        inside = torch.zeros(obuf.shape, dtype=torch.bool, device="cuda")
        inside[:, :8, :H, offset:offset + W] = True
        assert bool(torch.isnan(obuf[~inside]).all()) and int((~inside).sum()) > 0, name
        fin = torch.zeros(fbuf.shape, dtype=torch.bool, device="cuda")
        fin[:, :3, :H, offset:offset + W] = True
        assert bool((fbuf[~fin] == 7.0).all()) and torch.equal(vf, first), name
    # `second` and `coarse` have no say in the family: views of theirs one element into a row stay quad
    _sb, vs = wide_view(second, 3, 5, 1, -7.0)
    _cb, vc = wide_view(coarse, 2, 3, 1, 0.5)
    out = nan_filled((B, 8, H, W), dtype)
    assert LIB().SpyNetLevelLayer_gpu_forward_lp(first, vs, vc, out, *S.EXACT_FLAGS) == 0
    assert LIB().last_kernel_path() == LP.QUAD
    torch.cuda.synchronize()
    assert torch.equal(out, want)


@dtypes
def test_out_directly_behind_or_in_front_of_an_input_is_accepted(dtype):
    """the overlap test counts 2-byte elements: `out` starting at exactly an input's last byte + 1, and ending at exactly
    its first byte - 1, is accepted (spans computed with sizeof(float) would decline both); one element closer is declined"""
    shape = (1, 24, 40)
    _B, H, W = shape
    case32, want32 = LP.exact_reference((2, 24, 40))
    first, second, coarse = (torch.tensor(a[:1]).to(dtype).cuda() for a in case32)
    want = torch.tensor(want32[:1]).to(dtype).cuda()
    n_in, n_out = 3 * H * W, 8 * H * W
    for name in ("first", "second"):
        buf = torch.zeros(n_out + n_in + n_out, dtype=dtype, device="cuda")
        mid = buf[n_out:n_out + n_in].view(1, 3, H, W)
        mid.copy_(first if name == "first" else second)
        args = (mid, second, coarse) if name == "first" else (first, mid, coarse)
        for start in (n_out + n_in, 0):
            out = buf[start:start + n_out].view(1, 8, H, W)
            out.fill_(float("nan"))
            assert LIB().SpyNetLevelLayer_gpu_forward_lp(*args, out, *S.EXACT_FLAGS) == 0, (name, start)
            torch.cuda.synchronize()
            assert torch.equal(out, want), (name, start)
        for start in (n_out + n_in - 1, 1):
            out = buf[start:start + n_out].view(1, 8, H, W)
            assert LIB().SpyNetLevelLayer_gpu_forward_lp(*args, out, *S.EXACT_FLAGS) == 1, (name, start)


@dtypes
def test_non_finite_flows_stay_inside_second(dtype):
    """NaN, +-inf and the largest finite coarse flows (the position is clamped, NaN included, before it becomes an int: no
    address outside `second` can be formed): `first` is copied, and every site whose `up` is what it is without them has the
    same warp"""
    shape = (1, 24, 40)
    first, second, coarse = (t.cuda() for t in LP.ordinary_case(shape, "normal", dtype))
    bad = coarse.clone()
    bad[0, 0, 2, 3], bad[0, 1, 5, 7], bad[0, 0, 8, 11] = float("nan"), float("inf"), float("-inf")
    bad[0, 1, 9, 1] = float(torch.finfo(dtype).max)
    for flags in S.FLAGS:
        want, _ = run((first, second, coarse), flags)
        got, _ = run((first, second, bad), flags, allow_nan=True)
        want32, _ = run_f32((first, second, bad), flags)
        assert same_bits(got[:, 0:3], first)
        # `up` is still the float32 library's, rounded once (a NaN compared as a NaN, whatever its payload)
        assert torch.equal(torch.nan_to_num(got[:, 6:8].float(), nan=12345.0),
                           torch.nan_to_num(want32[:, 6:8].float(), nan=12345.0))
        same_up = (bits(got[:, 6:8]) == bits(want[:, 6:8])).all(dim=1, keepdim=True).expand(1, 3, 24, 40)
        assert torch.equal(bits(got[:, 3:6])[same_up], bits(want[:, 3:6])[same_up])
        assert 0 < int((~same_up).sum()) < same_up.numel()


def layer(flags, native_half):
    from my_package.functions.SpyNetLevelLayer import SpyNetLevelLayer
    f = SpyNetLevelLayer(*flags)
    if native_half is not None:
        f.native_half = native_half
    return f


@dtypes
def test_layer_routes(dtype):
    from my_package.functions.SpyNetLevelLayer import SpyNetLevelLayer, _composed
    assert SpyNetLevelLayer.native_half is False
    quad = tuple(t.cuda() for t in LP.ordinary_case((2, 24, 40), "normal", dtype))
    direct = tuple(t.cuda() for t in LP.ordinary_case((2, 26, 42), "normal", dtype))
    with torch.no_grad():
        layer((0, 0), None)(*(t.float() for t in direct))
    assert F32().last_kernel_path() == "spynet_level:direct"           # and no half call below may move it
    for flags in S.FLAGS:
        bflags = tuple(bool(f) for f in flags)
        with torch.no_grad():
            # native_half: the entry point's bits and path
            for case in (direct, quad):
                want, path = run(case, flags)
                got = layer(flags, True)(*case)
                assert LIB().last_kernel_path() == path and got.dtype == dtype and torch.equal(got, want)
            assert LIB().last_kernel_path() == LP.QUAD
            # the default: the torch expression, the library not called
            got = layer(flags, None)(*direct)
            assert torch.equal(got, _composed(*direct, *bflags)) and got.dtype == dtype
            assert LIB().last_kernel_path() == LP.QUAD
            # `fused` off: the torch expression whatever native_half says
            off = layer(flags, True)
            off.fused = False
            assert torch.equal(off(*direct), _composed(*direct, *bflags)) and LIB().last_kernel_path() == LP.QUAD
            # a declined call (a w-stride of 2) composes
            wide = torch.zeros((2, 3, 26, 84), dtype=dtype, device="cuda")
            wide[..., ::2] = direct[1]
            out = torch.empty((2, 8, 26, 42), dtype=dtype, device="cuda")
            assert LIB().SpyNetLevelLayer_gpu_forward_lp(direct[0], wide[..., ::2], direct[2], out, *flags) == 1
            got = layer(flags, True)(direct[0], wide[..., ::2], direct[2])
            assert torch.equal(got, _composed(direct[0], wide[..., ::2], direct[2], *bflags))
            assert LIB().last_kernel_path() == LP.QUAD
            # autocast composes
            with torch.autocast("cuda", dtype=dtype):
                got = layer(flags, True)(*direct)
                assert torch.equal(got, _composed(*direct, *bflags))
            assert LIB().last_kernel_path() == LP.QUAD
            # mixed dtypes compose: a float32 `first` beside a half `second` and coarse flow
            mixed = (direct[0].float(), direct[1], direct[2])
            got = layer(flags, True)(*mixed)
            assert got.dtype == torch.float32 and torch.equal(got, _composed(*mixed, *bflags))
            assert LIB().last_kernel_path() == LP.QUAD
        # a call that wants a gradient composes and back-propagates
        first, second, coarse = (t.clone().requires_grad_(True) for t in direct)
        out = layer(flags, True)(first, second, coarse)
        assert LIB().last_kernel_path() == LP.QUAD
        assert out.requires_grad and torch.equal(out, _composed(first, second, coarse, *bflags))
        out.float().square().sum().backward()
        for t in (first, second, coarse):
            assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == dtype
        assert float(coarse.grad.float().abs().max()) > 0
        # the same tensors under no_grad do reach the kernel
        with torch.no_grad():
            layer(flags, True)(first, second, coarse)
        assert LIB().last_kernel_path() == LP.DIRECT
        with torch.no_grad():
            layer(flags, True)(*quad)
    # the binding's own refusals, on device tensors
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    out = torch.empty((2, 8, 24, 40), dtype=dtype, device="cuda")
    with pytest.raises(TypeError, match="expected"):
        LIB().SpyNetLevelLayer_gpu_forward_lp(quad[0], quad[1], quad[2].to(other), out, 0, 0)
    with pytest.raises(TypeError, match="float16 or torch.bfloat16"):
        LIB().SpyNetLevelLayer_gpu_forward_lp(*(t.float() for t in quad), out.float(), 0, 0)
    with pytest.raises(TypeError, match="expected"):
        LIB().SpyNetLevelLayer_gpu_forward_lp(*quad, out.float(), 0, 0)
    assert F32().last_kernel_path() == "spynet_level:direct"           # no half call reached the float32 library


def test_network_levels_by_the_half_kernel(monkeypatch):
    """MEMC_Net_s cast to bfloat16, 1 x 64 x 96, `fused_level_half` on: every level input of both directions is the float32
    library's on the widened inputs, rounded once; with the switch off the half library is not called"""
    import networks
    import _netutil
    from networks._spynet import SPyNet
    dtype = torch.bfloat16
    net = networks.MEMC_Net_s(channel=3, filter_size=4, training=False).eval()
    net.load_state_dict(_netutil.named_weights(net.state_dict()), strict=True, warn_align_corners=False)
    net = net.cuda().to(dtype)
    x = _netutil.frames(33, 1, 64, 96).cuda().to(dtype)
    seen = []
    inner = SPyNet.level_input

    def recording(self, first, second, coarse):
        out = inner(self, first, second, coarse)
        seen.append((first, second, coarse, out, LIB().last_kernel_path()))
        return out
    monkeypatch.setattr(SPyNet, "level_input", recording)
    flags = (int(net.flownets.align_upsample), int(net.flownets.align_sample))
    with torch.no_grad():
        run(tuple(t.cuda() for t in LP.ordinary_case((1, 6, 5), "zero", dtype)), (0, 0))
        assert LIB().last_kernel_path() == LP.DIRECT
        assert net.flownets.fused_level_half is False
        net(x)
        assert len(seen) == 6 and all(rec[4] == LP.DIRECT for rec in seen)     # switch off: the half library is not called
        del seen[:]
        net.flownets.fused_level_half = True
        outs = net(x)
    assert [tuple(rec[0].shape[2:]) for rec in seen] == [(16, 24), (32, 48), (64, 96)] * 2
    for first, second, coarse, out, path in seen:
        assert path == LP.QUAD and out.dtype == dtype and out.shape == (1, 8) + tuple(first.shape[2:])
        want, path32 = run_f32((first, second, coarse), flags)
        assert path32 == "spynet_level:quad" and torch.equal(out, want)
    assert any(bool(rec[2].any()) for rec in seen)                             # some level saw a flow that moves things
    assert len(outs) == 4                                                      # frames, flows, filters, occlusions
    for group in outs:
        assert len(group) == 2
        for t in group:
            assert t.dtype == dtype and t.shape[0] == 1 and tuple(t.shape[2:]) == (64, 96) and bool(torch.isfinite(t).all())
