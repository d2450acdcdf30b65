"""The mixed-precision RGB adaptive-warp backward (libmemc_hip_mx_grad.so, include/memc_warp_mx_grad.h): an fp32 image and an
fp32 gradoutput beside fp16 / bf16 taps, the flow in fp32 or that dtype -- the backward of the call torch.autocast makes --
and the route _FilterInterpolationMxFunction.backward takes for it.

Inputs are the census table of tests/_lowp_paths.py (bands in both directions, capped tiles, slow sites, split and mixed
lanes, empty tiles, 4-column edge tiles, a ragged last tile row) plus the minimum width and a wide row of mostly invalid
sites, as in test_gpu_blend_grad.py.  Taps and half flows are rounded to T first (P.rounded); the image and gradoutput are
fp32 as generated, not on T's grid.  Rules:
  flow and tap gradients  torch.equal to libmemc_hip.so's FilterInterpolationLayer_gpu_backward on the widened inputs,
                          `.to(dtype)` once -- no tolerance: the fp32 kernel is the reference, with the same choice of
                          gradinput1 (a buffer or NULL).  Both start as NaN: the kernel defines every element;
  image gradient          fp32, flushed with atomics on both sides: test_gpu_lowp_grad.image_gradients_agree (every finite
                          cell of either side within tests/_image_grad.py's derived bound of the float64 restatement on the
                          call's inputs -- the packed planes' grid plus fp32's roundings, for any order of the atomics --
                          and 99.9 % equal after rounding to T) after the fp32 library run twice passed it; against the
                          oracle tests/_parity.close(..., RTOL), and 3 x RTOL for a buffer that already held 0.5 (as the half
                          library's test has it).
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

import _lowp_paths as P                      # noqa: E402
from _parity import RTOL, close              # noqa: E402
from test_gpu_blend_grad import EXTRA, Spy   # noqa: E402
from test_gpu_lowp_grad import image_gradients_agree, image_reference         # noqa: E402
from test_gpu_lowp_parity import DTYPES                               # noqa: E402
from test_gpu_lowp_paths import same_specials_and_finite_bits        # noqa: E402
from test_gpu_mx import (channel_slice_shifted, dev, leaves, module_inputs, promoted_grads, shifted_by_one,      # noqa: E402
                         warp_module)
from tools import synth                      # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
TNAMES = sorted(DTYPES)
FLOWS = ["fp32", "T"]
CASES = P.CASES + EXTRA
IDS = P.CASE_IDS + ["2x37x8-min-width", "1x20x1280-far"]
IMAGE = [True, False]
IMAGE_IDS = ["image", "noimage"]
PATHS = {True: "fi_bwd_mx:tiled_c3", False: "fi_bwd_mx:tiled_c3_noimage"}


def MXG():
    import my_package._ext.my_lib_mx_grad as M
    return M


def MX():
    import my_package._ext.my_lib_mx as M
    return M


def F32LIB():
    import my_package._ext.my_lib as M
    return M


_INPUTS = {}


def inputs(case, tname, flow_t):
    """(image fp32, flow fp32 or T, taps T, gradoutput fp32) of a case on the GPU; taps and half flows rounded to T, the
    image and gradoutput as generated.  Made once, never written."""
    key = (case, tname, flow_t)
    if key not in _INPUTS:
        T = DTYPES[tname]
        x, flow, filt, gout = P.case_inputs(case, 3)
        _INPUTS[key] = (dev(x), dev(P.rounded(flow, tname), T) if flow_t == "T" else dev(flow), dev(P.rounded(filt, tname), T),
                        dev(gout))
    return _INPUTS[key]


def run_mx(x, flow, filt, gout, g1, g2=None, g3=None):
    """the mixed library; g1: None or the fp32 buffer it adds into.  gradinput2 / gradinput3 start as NaN"""
    g2 = torch.full_like(flow, NAN) if g2 is None else g2
    g3 = torch.full_like(filt, NAN) if g3 is None else g3
    status = MXG().FilterInterpolationLayer_gpu_backward_mx(x, flow, filt, gout, g1, g2, g3)
    torch.cuda.synchronize()
    return status, g1, g2, g3


def run_f32(x, flow, filt, gout, with_image, fill=0.0):
    """the fp32 library on the widened inputs"""
    x, flow, filt, gout = (t.float().contiguous() for t in (x, flow, filt, gout))
    g1 = torch.full_like(x, fill) if with_image else None
    g2, g3 = torch.full_like(flow, NAN), torch.full_like(filt, NAN)
    assert F32LIB().FilterInterpolationLayer_gpu_backward(x, flow, filt, gout, g1, g2, g3) == 0
    torch.cuda.synchronize()
    assert F32LIB().last_kernel_path() == "fi_bwd:tiled_c3"
    return g1, g2, g3


_REFERENCE = {}


def reference(case, tname, flow_t, with_image):
    """run_f32 of a case's inputs, once: (gradinput1 or None, gradinput2, gradinput3), all fp32"""
    key = (case, tname, flow_t, with_image)
    if key not in _REFERENCE:
        _REFERENCE[key] = run_f32(*inputs(case, tname, flow_t), with_image)
    return _REFERENCE[key]


_IMAGE_REFERENCE = {}


def image_ref(case, tname, flow_t):
    """tests/_image_grad.Reference of a case's inputs, once"""
    key = (case, tname, flow_t)
    if key not in _IMAGE_REFERENCE:
        _x, flow, filt, gout = inputs(case, tname, flow_t)
        _IMAGE_REFERENCE[key] = image_reference(flow, filt, gout)
    return _IMAGE_REFERENCE[key]


_ORACLE = {}


def oracle_image_gradient(oracle, case, tname, flow_t):
    key = (case, tname, flow_t)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.filter_interpolation_backward(*(t.float().cpu().numpy() for t in inputs(case, tname, flow_t)))[0]
    return _ORACLE[key]


def zeros_like_image(x, fill=0.0):
    return torch.full(x.shape, fill, dtype=torch.float32, device=x.device)


# --------------------------------------------------------------------------------------------------------------
# 1: flow and tap gradients, bit for bit
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("with_image", IMAGE, ids=IMAGE_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_flow_and_tap_gradients_are_the_fp32_ones_rounded(case, tname, flow_t, with_image):
    T = DTYPES[tname]
    x, flow, filt, gout = inputs(case, tname, flow_t)
    assert x.dtype == gout.dtype == torch.float32 and filt.dtype == T
    assert not torch.equal(x.to(T).float(), x) and not torch.equal(gout.to(T).float(), gout)      # not on T's grid
    status, g1, g2, g3 = run_mx(x, flow, filt, gout, zeros_like_image(x) if with_image else None)
    assert status == 0 and MXG().last_kernel_path() == PATHS[with_image]
    assert g2.dtype == flow.dtype and g3.dtype == T
    assert not torch.isnan(g2).any() and not torch.isnan(g3).any(), "an element was not written"
    _w1, w2, w3 = reference(case, tname, flow_t, with_image)
    assert torch.equal(g2, w2.to(flow.dtype)), "flow gradient"
    assert torch.equal(g3, w3.to(T)), "tap gradient"


# --------------------------------------------------------------------------------------------------------------
# 2: the image gradient
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_image_gradient_matches_the_fp32_library(oracle, ci, tname, flow_t):
    T = DTYPES[tname]
    case = CASES[ci]
    x, flow, filt, gout = inputs(case, tname, flow_t)
    label = "%s %s flow %s" % (IDS[ci], tname, flow_t)
    a1 = reference(case, tname, flow_t, True)[0]
    b1, _, _ = run_f32(x, flow, filt, gout, True)
    image_gradients_agree(a1, b1, T, "control: fp32 twice, " + label, image_ref(case, tname, flow_t))
    status, g1, _, _ = run_mx(x, flow, filt, gout, zeros_like_image(x))
    assert status == 0 and g1.dtype == torch.float32
    image_gradients_agree(g1, a1, T, "mixed vs fp32, " + label, image_ref(case, tname, flow_t))
    if ci in (0, 2):
        err = close(g1.cpu().numpy(), oracle_image_gradient(oracle, case, tname, flow_t), "mx gradinput1 " + label, RTOL)
        print("oracle %s: max err %.3g" % (label, err))


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("ci", [0, 2], ids=[IDS[0], IDS[2]])
def test_adds_into_a_gradinput1_that_holds_values(oracle, ci, tname, flow_t):
    """The contract is "added into": a buffer pre-filled with 0.5 comes back as oracle + 0.5 (3 x RTOL, as
    test_gpu_lowp_paths.test_backward_adds_into_a_gradinput1_that_holds_values has it)."""
    case = CASES[ci]
    x, flow, filt, gout = inputs(case, tname, flow_t)
    status, g1, _, _ = run_mx(x, flow, filt, gout, zeros_like_image(x, 0.5))
    assert status == 0
    want = oracle_image_gradient(oracle, case, tname, flow_t) + np.float32(0.5)
    err = close(g1.cpu().numpy(), want, "mx gradinput1 += %s %s flow %s" % (IDS[ci], tname, flow_t), 3 * RTOL)
    print("gradinput1 += %s %s flow %s: max err %.3g" % (IDS[ci], tname, flow_t, err))


# --------------------------------------------------------------------------------------------------------------
# 3: determinism and views
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
def test_views_and_run_to_run(tname, flow_t):
    T = DTYPES[tname]
    case = P.CASES[1]
    x, flow, filt, gout = inputs(case, tname, flow_t)
    status, _, g2, g3 = run_mx(x, flow, filt, gout, None)
    assert status == 0
    _, w2, w3 = reference(case, tname, flow_t, False)
    assert torch.equal(g2, w2.to(flow.dtype)) and torch.equal(g3, w3.to(T))
    # a second identical call without the image gradient: no atomics
    status, _, again2, again3 = run_mx(x, flow, filt, gout, None)
    assert status == 0 and torch.equal(again2, g2) and torch.equal(again3, g3)
    # every tensor row-padded by 64 elements, the gradients included
    px, pf, pk, pg = (synth.padded_planes(t) for t in (x, flow, filt, gout))
    assert pk.stride(2) == case[2] + 64 and not pk.is_contiguous() and not px.is_contiguous()
    status, _, v2, v3 = run_mx(px, pf, pk, pg, None, synth.padded_planes(torch.full_like(flow, NAN)),
                               synth.padded_planes(torch.full_like(filt, NAN)))
    assert status == 0 and MXG().last_kernel_path() == PATHS[False]
    assert torch.equal(v2, g2) and torch.equal(v3, g3)
    status, v1, v2, v3 = run_mx(px, pf, pk, pg, synth.padded_planes(zeros_like_image(x)),
                                synth.padded_planes(torch.full_like(flow, NAN)), synth.padded_planes(torch.full_like(filt, NAN)))
    assert status == 0 and MXG().last_kernel_path() == PATHS[True]
    u1, u2, u3 = reference(case, tname, flow_t, True)
    assert torch.equal(v2, u2.to(flow.dtype)) and torch.equal(v3, u3.to(T))
    image_gradients_agree(v1.contiguous(), u1, T, "row-padded", image_ref(case, tname, flow_t))
    # the fp32 image and gradoutput as a channel slice of a larger buffer, one element off: dword alignment suffices
    _bx, xv = channel_slice_shifted(x)
    _bg, gv = channel_slice_shifted(gout)
    assert xv.data_ptr() % 8 == 4 and gv.data_ptr() % 8 == 4 and xv.stride() == gv.stride()
    status, _, v2, v3 = run_mx(xv, flow, filt, gv, None)
    assert status == 0 and torch.equal(v2, g2) and torch.equal(v3, g3)
    buf1, v1 = channel_slice_shifted(x, fill=NAN)            # gradinput1 of input1's layout, NaN around it
    v1.zero_()
    assert v1.stride() == xv.stride()
    status, v1, v2, v3 = run_mx(xv, flow, filt, gv, v1)
    assert status == 0 and torch.equal(v2, u2.to(flow.dtype)) and torch.equal(v3, u3.to(T))
    image_gradients_agree(v1.contiguous(), u1, T, "channel slice", image_ref(case, tname, flow_t))
    assert torch.isnan(buf1[1:].view(x.size(0), 5, *x.shape[2:])[:, (0, 4)]).all() and torch.isnan(buf1[0])
    # taps one half element off: declined, nothing touched
    for g1 in (None, zeros_like_image(x)):
        status, g1, v2, v3 = run_mx(x, flow, shifted_by_one(filt), gout, g1)
        assert status == 1 and torch.isnan(v2).all() and torch.isnan(v3).all()
        assert g1 is None or not g1.any()
    # ... and a tap gradient one half element off
    status, _, v2, v3 = run_mx(x, flow, filt, gout, None, None, shifted_by_one(torch.full_like(filt, NAN)))
    assert status == 1 and torch.isnan(v2).all() and torch.isnan(v3).all()


# --------------------------------------------------------------------------------------------------------------
# 4: special values
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("with_image", IMAGE, ids=IMAGE_IDS)
def test_fp16_tap_gradient_overflows_to_infinity(flow_t, with_image):
    """gradoutput of 6e4 everywhere: tap gradients (a weight x 6e4 x the pixel sum) beyond 65504 in places become +-inf
    exactly where the fp32 result rounds to it"""
    T = torch.float16
    x, flow, filt, gout = inputs(P.CASES[4], "fp16", flow_t)
    big = torch.full_like(gout, 6e4)
    status, g1, g2, g3 = run_mx(x, flow, filt, big, zeros_like_image(x) if with_image else None)
    assert status == 0
    _w1, w2, w3 = run_f32(x, flow, filt, big, with_image)
    w3T = w3.to(T)
    assert bool(torch.isinf(w3T).any()) and bool(torch.isfinite(w3T).any())
    assert torch.equal(torch.isinf(g3), torch.isinf(w3T)) and torch.equal(g3, w3T)
    same_specials_and_finite_bits(g2, w2.to(flow.dtype), "flow gradient")


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("with_image", IMAGE, ids=IMAGE_IDS)
def test_nan_and_inf_inputs(tname, flow_t, with_image):
    """One NaN and one +Inf gradoutput, one NaN tap and one -Inf tap, all at valid sites (as
    test_gpu_lowp_paths.test_backward_nan_and_inf_inputs has them): such sites take per-site atomics, and every gradient
    carries the fp32 library's NaN / Inf pattern after rounding."""
    T = DTYPES[tname]
    case = P.CASES[0]
    nan_tap, inf_tap, nan_gout, inf_gout = (0, 5, 40, 100), (0, 9, 70, 150), (0, 1, 50, 200), (0, 2, 30, 120)
    valid = P.locate(P.rounded(P.case_flow(case), tname if flow_t == "T" else "fp32"))[0]
    for _, _, y, xx in (nan_tap, inf_tap, nan_gout, inf_gout):
        assert valid[0, y, xx], "the special value must sit on a site that gathers"
    x, flow, filt, gout = inputs(case, tname, flow_t)
    filt, gout = filt.clone(), gout.clone()
    filt[nan_tap] = NAN
    filt[inf_tap] = -float("inf")
    gout[nan_gout] = NAN
    gout[inf_gout] = float("inf")
    status, g1, g2, g3 = run_mx(x, flow, filt, gout, zeros_like_image(x) if with_image else None)
    assert status == 0
    w1, w2, w3 = run_f32(x, flow, filt, gout, with_image)
    n2 = same_specials_and_finite_bits(g2, w2.to(flow.dtype), "flow gradient")
    n3 = same_specials_and_finite_bits(g3, w3.to(T), "tap gradient")
    assert n2[0] + n2[1] > 0 and n3[0] + n3[1] > 0
    print("specials %s flow %s %s: flow gradient NaN %d Inf %d, tap gradient NaN %d Inf %d"
          % ((tname, flow_t, with_image) + n2 + n3))
    if with_image:
        assert 0 < int((~torch.isfinite(w1.to(T))).sum()) < 400
        b1, _, _ = run_f32(x, flow, filt, gout, True)
        ref = image_reference(flow, filt, gout)
        image_gradients_agree(w1, b1, T, "control: fp32 twice, NaN / Inf inputs %s" % tname, ref)
        image_gradients_agree(g1, w1, T, "mixed vs fp32, NaN / Inf inputs %s" % tname, ref)


# --------------------------------------------------------------------------------------------------------------
# 5: routing of the layer's backward
# --------------------------------------------------------------------------------------------------------------
class PathSpy(Spy):
    """Spy that also keeps the library's kernel path behind each call, read on the calling thread (autograd runs the
    backward on a thread of its own, and the path is per thread)"""

    def __init__(self, monkeypatch, owner, name):
        self.paths = []
        real = getattr(owner, name)

        def with_path(*a, **k):
            r = real(*a, **k)
            self.paths.append(owner.last_kernel_path())
            return r
        monkeypatch.setattr(owner, name, with_path)
        Spy.__init__(self, monkeypatch, owner, name)


class Spies:
    def __init__(self, monkeypatch):
        self.mx_grad = PathSpy(monkeypatch, MXG(), "FilterInterpolationLayer_gpu_backward_mx")
        self.mx_fwd = Spy(monkeypatch, MX(), "FilterInterpolationLayer_gpu_forward_mx")
        self.f32_bwd = Spy(monkeypatch, F32LIB(), "FilterInterpolationLayer_gpu_backward")


def layer_backward(t, names, gout):
    """the warp layer on leaves `names` of t, backward of gout; the leaves"""
    m = leaves(t, names)
    warp_module(m["x0"], m["f0"], m["k0"]).backward(gout)
    torch.cuda.synchronize()
    return m


def signed_gradient(shape, seed=5):
    return dev(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("image_grad", [False, True], ids=["frames-are-data", "frame-gradient"])
@pytest.mark.parametrize("shape", [(2, 3, 40, 64), (1, 3, 96, 256)], ids=["2x3x40x64", "1x3x96x256"])
def test_the_layer_takes_the_mixed_backward(monkeypatch, shape, tname, flow_t, image_grad):
    _h, t = module_inputs(shape, 16, tname, flow_t, 89)
    names = ("f0", "k0") + (("x0",) if image_grad else ())
    gout = signed_gradient(shape)
    spy = Spies(monkeypatch)
    m = layer_backward(t, names, gout)
    assert spy.mx_fwd.returns == [0]
    assert spy.mx_grad.calls == 1 and spy.mx_grad.returns == [0] and spy.f32_bwd.calls == 0
    assert spy.mx_grad.paths == [PATHS[image_grad]]
    want = promoted_grads(warp_module, t, names, ("x0", "f0", "k0"), gout)
    torch.cuda.synchronize()
    assert spy.mx_grad.calls == 1                             # (the promoted call is the fp32 Function's)
    for n in ("f0", "k0"):
        assert m[n].grad.dtype == t[n].dtype and torch.equal(m[n].grad, want[n]), n
    if image_grad:
        assert m["x0"].grad.dtype == torch.float32
        image_gradients_agree(m["x0"].grad, want["x0"], DTYPES[tname], "layer frame gradient", (t["f0"], t["k0"], gout))
    else:
        assert m["x0"].grad is None


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("shape,taps", [((2, 3, 24, 23), 16), ((2, 5, 24, 32), 16), ((2, 3, 24, 32), 4)],
                         ids=["W23", "C5", "4taps"])
def test_uncovered_mixed_calls_keep_the_fp32_backward(monkeypatch, shape, taps, tname):
    _h, t = module_inputs(shape, taps, tname, "T", 97)
    names = ("f0", "k0")
    gout = signed_gradient(shape)
    spy = Spies(monkeypatch)
    m = layer_backward(t, names, gout)
    assert all(r == 1 for r in spy.mx_grad.returns), spy.mx_grad.returns      # no kernel of the new library
    assert spy.f32_bwd.calls == 1
    want = promoted_grads(warp_module, t, names, ("x0", "f0", "k0"), gout)
    for n in names:
        assert m[n].grad.dtype == t[n].dtype and torch.equal(m[n].grad, want[n]), n


@pytest.mark.parametrize("tname", TNAMES)
def test_a_declined_view_takes_the_promoted_backward(monkeypatch, tname):
    """A covered shape whose taps the library cannot read (a contiguous tensor two bytes off): return 1, then the casts and
    the fp32 kernel -- the promoted call's bits."""
    shape = (2, 3, 40, 64)
    _h, t = module_inputs(shape, 16, tname, "fp32", 101)
    k0 = shifted_by_one(t["k0"])
    assert k0.is_contiguous() and k0.data_ptr() % 8 == 2
    gout = signed_gradient(shape)
    spy = Spies(monkeypatch)
    f0, k0 = t["f0"].clone().requires_grad_(True), k0.detach().requires_grad_(True)
    assert k0.data_ptr() % 8 == 2
    warp_module(t["x0"], f0, k0).backward(gout)
    torch.cuda.synchronize()
    assert spy.mx_fwd.returns == [1]
    assert spy.mx_grad.returns == [1] and spy.f32_bwd.calls == 1
    want = promoted_grads(warp_module, t, ("f0", "k0"), ("x0", "f0", "k0"), gout)
    assert f0.grad.dtype == torch.float32 and torch.equal(f0.grad, want["f0"])
    assert k0.grad.dtype == DTYPES[tname] and torch.equal(k0.grad, want["k0"])


@pytest.mark.parametrize("tname", TNAMES)
def test_pure_calls_never_touch_the_mixed_backward(monkeypatch, tname):
    T = DTYPES[tname]
    shape = (2, 3, 40, 64)
    _h, t = module_inputs(shape, 16, tname, "fp32", 103)
    gout = signed_gradient(shape)
    spy = Spies(monkeypatch)
    for cast in (torch.float32, T):
        x, f, k = (t[n].detach().to(c).clone().requires_grad_(True) for n, c in (("x0", cast), ("f0", torch.float32), ("k0", cast)))
        warp_module(x, f, k).backward(gout.to(cast))
        assert x.grad.dtype == cast and k.grad.dtype == cast
    torch.cuda.synchronize()
    assert spy.mx_grad.calls == 0 and spy.mx_fwd.calls == 0 and spy.f32_bwd.calls == 1
