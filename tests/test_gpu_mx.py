"""The mixed-precision adaptive warp and blend (libmemc_hip_mx.so, include/memc_warp_mx.h): fp32 frames and output beside
fp16 / bf16 taps and occlusions, the flow in fp32 or that dtype -- what torch.autocast hands the operators -- and the
route FilterInterpolationLayer / FilterInterpolationBlendLayer take for such calls.

Inputs are the census table of tests/_lowp_paths.py (bands in both directions, capped tiles, slow sites, split and mixed
lanes, empty tiles, 4-column edge tiles, a ragged last tile row) plus the minimum width and a wide row of mostly invalid
sites, as in test_gpu_blend_grad.py.  Taps, occlusions and half flows are rounded to T first (P.rounded); images and
outputs are fp32.  Rules:
  against the oracle     tests/_parity.close(..., RTOL) on the widened inputs -- the project's one rule, nothing else;
  against the half twin  on images representable in T, the mixed result rounded to T is within one ulp_T of
                         libmemc_hip_lp.so's everywhere, with the same non-finite pattern: both evaluate one fp32 expression
                         and may differ in instruction fusion alone, which moves an fp32 value by a few fp32 ulps and so can
                         flip a rounding to T only at a tie.  The bit-equal fraction is printed, not asserted;
  gradients              bit for bit those of the explicitly promoted call (the image gradient apart: it takes atomics).
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
import _netutil                              # noqa: E402
from _parity import RTOL, close              # noqa: E402
from test_gpu_blend_grad import EXTRA, Spy, np_occlusion      # noqa: E402
from test_gpu_lowp_parity import DTYPES, ulp                  # noqa: E402
from tools import synth                      # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
TNAMES = sorted(DTYPES)
FLOWS = ["fp32", "T"]
WARP_CASES = P.CASES + EXTRA
WARP_IDS = P.CASE_IDS + ["2x37x8-min-width", "1x20x1280-far"]
BLEND_CASES = P.BLEND_CASES + EXTRA
BLEND_IDS = P.CASE_IDS[:len(P.BLEND_CASES)] + WARP_IDS[-2:]
FWD_PATH, BLEND_PATH = "fi_fwd_mx:tiled_c3", "fi_blend_mx:tiled_c3"


def MX():
    import my_package._ext.my_lib_mx as M
    return M


def LPLIB():
    import my_package._ext.my_lib_lp as M
    return M


def F32LIB():
    import my_package._ext.my_lib as M
    return M


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)


def N(t):
    return t.detach().float().cpu().numpy()


_HOST = {}


def host_case(case, tname, flow_t, image_in_T=False):
    """One direction pair of a case on the host, fp32 numpy, taps / occlusions rounded to T, flows to their dtype, the
    second direction from seed + 100; `want0` / `want` the oracle's warp of direction 0 and blend.  Computed once."""
    key = (case, tname, flow_t, image_in_T)
    if key not in _HOST:
        from oracle import memc_oracle as O
        B, H, W, kind, sigma, seed = case
        h = {}
        for d, (x, f, k, o) in enumerate((("x0", "f0", "k0", "o0"), ("x2", "f1", "k1", "o1"))):
            c = (B, H, W, kind, sigma, seed + 100 * d)
            xi, fl, kt, _ = P.case_inputs(c, 3)
            h[x] = P.rounded(xi, tname) if image_in_T else xi
            h[f] = P.rounded(fl, tname if flow_t == "T" else "fp32")
            h[k] = P.rounded(kt, tname)
            h[o] = P.rounded(np_occlusion(np.random.default_rng(seed + 100 * d + 7), B, H, W), tname)
        if not image_in_T:                                     # (the half-twin comparison needs no oracle)
            h["want0"] = O.filter_interpolation_forward(h["x0"], h["f0"], h["k0"])
            w2 = O.filter_interpolation_forward(h["x2"], h["f1"], h["k1"])
            h["want"] = ((h["o0"] * h["want0"]).astype(np.float32) + (h["o1"] * w2).astype(np.float32)).astype(np.float32)
        _HOST[key] = h
    return _HOST[key]


def device_case(h, tname, flow_t):
    T = DTYPES[tname]
    FT = T if flow_t == "T" else torch.float32
    return {"x0": dev(h["x0"]), "x2": dev(h["x2"]), "f0": dev(h["f0"], FT), "f1": dev(h["f1"], FT), "k0": dev(h["k0"], T),
            "k1": dev(h["k1"], T), "o0": dev(h["o0"], T), "o1": dev(h["o1"], T)}


BLEND_NAMES = ("x0", "x2", "f0", "f1", "k0", "k1", "o0", "o1")


def mx_warp(x, f, k, out=None):
    out = torch.full_like(x, NAN) if out is None else out
    status = MX().FilterInterpolationLayer_gpu_forward_mx(x, f, k, out)
    torch.cuda.synchronize()
    return status, out


def mx_blend(t, out=None, **over):
    t = dict(t, **over)
    out = torch.full_like(t["x0"], NAN) if out is None else out
    status = MX().FilterInterpolationBlendLayer_gpu_forward_mx(*[t[n] for n in BLEND_NAMES], out)
    torch.cuda.synchronize()
    return status, out


# --------------------------------------------------------------------------------------------------------------
# 1, 2: oracle parity on every in-kernel path
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("case", WARP_CASES, ids=WARP_IDS)
def test_warp_matches_the_oracle_on_every_tile_path(oracle, case, tname, flow_t):
    h = host_case(case, tname, flow_t)
    t = device_case(h, tname, flow_t)
    status, out = mx_warp(t["x0"], t["f0"], t["k0"])
    assert status == 0 and MX().last_kernel_path() == FWD_PATH
    assert out.dtype == torch.float32 and not torch.isnan(out).any(), "an element was not assigned"
    close(N(out), h["want0"], "mx warp %s flow %s" % (tname, flow_t), RTOL)


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("case", BLEND_CASES, ids=BLEND_IDS)
def test_blend_matches_the_oracle_on_every_tile_path(oracle, case, tname, flow_t):
    h = host_case(case, tname, flow_t)
    t = device_case(h, tname, flow_t)
    status, out = mx_blend(t)
    assert status == 0 and MX().last_kernel_path() == BLEND_PATH
    assert out.dtype == torch.float32 and not torch.isnan(out).any(), "an element was not assigned"
    close(N(out), h["want"], "mx blend %s flow %s" % (tname, flow_t), RTOL)


# --------------------------------------------------------------------------------------------------------------
# 3: the half kernels on images that T holds exactly
# --------------------------------------------------------------------------------------------------------------
def within_one_ulp(mixed, half, T, label):
    """mixed (fp32) rounded to T against the half library's T result"""
    got, want = mixed.to(T), half
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want)), label
    fin = torch.isfinite(want)
    g, w = got.float()[fin], want.float()[fin]
    equal = float((got == want)[fin].float().mean()) if bool(fin.any()) else 1.0
    worst = float(((g - w).abs() / ulp(w, T)).max()) if bool(fin.any()) else 0.0
    print("%s: bit-equal %.6f of %d, worst %.3g ulp_T" % (label, equal, int(fin.sum()), worst))
    assert worst <= 1.0, (label, worst)


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("case", BLEND_CASES, ids=BLEND_IDS)
def test_consistent_with_the_half_kernels(case, tname, flow_t):
    T = DTYPES[tname]
    h = host_case(case, tname, flow_t, image_in_T=True)
    t = device_case(h, tname, flow_t)
    x0h, x2h = t["x0"].to(T), t["x2"].to(T)
    assert torch.equal(x0h.float(), t["x0"])                       # the images are representable in T
    status, out = mx_warp(t["x0"], t["f0"], t["k0"])
    assert status == 0
    half = torch.full_like(x0h, NAN)
    assert LPLIB().FilterInterpolationLayer_gpu_forward_lp(x0h, t["f0"], t["k0"], half) == 0
    assert LPLIB().last_kernel_path() == "fi_fwd_lp:tiled_c3"
    torch.cuda.synchronize()
    within_one_ulp(out, half, T, "warp %s flow %s" % (tname, flow_t))
    status, out = mx_blend(t)
    assert status == 0
    half = torch.full_like(x0h, NAN)
    assert LPLIB().FilterInterpolationBlendLayer_gpu_forward_lp(x0h, x2h, t["f0"], t["f1"], t["k0"], t["k1"], t["o0"],
                                                                 t["o1"], half) == 0
    assert LPLIB().last_kernel_path() == "fi_blend_lp:tiled_c3"
    torch.cuda.synchronize()
    within_one_ulp(out, half, T, "blend %s flow %s" % (tname, flow_t))


# --------------------------------------------------------------------------------------------------------------
# 4: views and determinism
# --------------------------------------------------------------------------------------------------------------
def channel_slice_shifted(src, fill=None):
    """src's values (or `fill`) as channels 1..3 of a five-channel buffer that starts ONE element into its allocation"""
    B, C, H, W = src.shape
    buf = torch.full((B * 5 * H * W + 1,), 7.0 if fill is None else fill, device=src.device, dtype=src.dtype)
    view = buf[1:].view(B, 5, H, W)[:, 1:1 + C]
    if fill is None:
        view.copy_(src)
    return buf, view


def shifted_by_one(src):
    buf = torch.empty(src.numel() + 1, device=src.device, dtype=src.dtype)
    view = buf[1:].view(src.shape)
    view.copy_(src)
    return view


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
def test_views_and_run_to_run(tname, flow_t):
    case = P.CASES[1]
    t = device_case(host_case(case, tname, flow_t), tname, flow_t)
    s, warp0 = mx_warp(t["x0"], t["f0"], t["k0"])
    s2, blend0 = mx_blend(t)
    assert s == 0 and s2 == 0
    # a second identical call: no atomics
    assert torch.equal(mx_warp(t["x0"], t["f0"], t["k0"])[1], warp0) and torch.equal(mx_blend(t)[1], blend0)
    # every tensor row-padded by 64 elements, outputs included
    pad = {n: synth.padded_planes(v) for n, v in t.items()}
    assert pad["k0"].stride(2) == case[2] + 64 and not pad["k0"].is_contiguous()
    s, out = mx_warp(pad["x0"], pad["f0"], pad["k0"], synth.padded_planes(torch.full_like(t["x0"], NAN)))
    assert s == 0 and MX().last_kernel_path() == FWD_PATH and torch.equal(out, warp0)
    s, out = mx_blend(pad, synth.padded_planes(torch.full_like(t["x0"], NAN)))
    assert s == 0 and MX().last_kernel_path() == BLEND_PATH and torch.equal(out, blend0)
    # fp32 images and output as a channel slice of a larger buffer, one element off: dword alignment suffices
    _b0, x0v = channel_slice_shifted(t["x0"])
    _b2, x2v = channel_slice_shifted(t["x2"])
    obuf, ov = channel_slice_shifted(t["x0"], fill=NAN)
    assert x0v.data_ptr() % 8 == 4 and ov.data_ptr() % 8 == 4 and x0v.stride() == ov.stride()
    s, out = mx_warp(x0v, t["f0"], t["k0"], ov)
    assert s == 0 and torch.equal(out, warp0)
    assert torch.isnan(obuf[1:].view(x0v.size(0), 5, *x0v.shape[2:])[:, (0, 4)]).all()     # the neighbours were not touched
    obuf, ov = channel_slice_shifted(t["x0"], fill=NAN)
    s, out = mx_blend(t, ov, x0=x0v, x2=x2v)
    assert s == 0 and torch.equal(out, blend0)
    assert torch.isnan(obuf[1:].view(x0v.size(0), 5, *x0v.shape[2:])[:, (0, 4)]).all()
    # taps one half element off: declined, nothing touched
    s, out = mx_warp(t["x0"], t["f0"], shifted_by_one(t["k0"]))
    assert s == 1 and torch.isnan(out).all()
    s, out = mx_blend(t, k0=shifted_by_one(t["k0"]), k1=shifted_by_one(t["k1"]))
    assert s == 1 and torch.isnan(out).all()
    # the occlusions as channel 1 of a two-channel tensor (strides stay multiples of four elements)
    two = [torch.stack((torch.full_like(t[n][:, 0], 9.0), t[n][:, 0]), dim=1) for n in ("o0", "o1")]
    s, out = mx_blend(t, o0=two[0][:, 1:2], o1=two[1][:, 1:2])
    assert s == 0 and torch.equal(out, blend0)


# --------------------------------------------------------------------------------------------------------------
# 5: routing of the layers
# --------------------------------------------------------------------------------------------------------------
class Spies:
    def __init__(self, monkeypatch):
        self.mx_warp = Spy(monkeypatch, MX(), "FilterInterpolationLayer_gpu_forward_mx")
        self.mx_blend = Spy(monkeypatch, MX(), "FilterInterpolationBlendLayer_gpu_forward_mx")
        self.f32 = [Spy(monkeypatch, F32LIB(), n) for n in ("FilterInterpolationLayer_gpu_forward",
                                                             "FilterInterpolationBlendLayer_gpu_forward")]
        self.lp = [Spy(monkeypatch, LPLIB(), n) for n in ("FilterInterpolationLayer_gpu_forward_lp",
                                                          "FilterInterpolationBlendLayer_gpu_forward_lp")]

    def f32_calls(self):
        return sum(s.calls for s in self.f32)

    def lp_calls(self):
        return sum(s.calls for s in self.lp)

    def mx_calls(self):
        return self.mx_warp.calls + self.mx_blend.calls


def module_inputs(shape, taps, tname, flow_t, seed):
    """device dict of the blend's eight inputs at `shape` with `taps` taps: fp32 frames, T taps and occlusions"""
    B, C, H, W = shape
    T = DTYPES[tname]
    FT = T if flow_t == "T" else torch.float32
    fs = int(round(taps ** 0.5))
    h = {}
    for d, (x, f, k, o) in enumerate((("x0", "f0", "k0", "o0"), ("x2", "f1", "k1", "o1"))):
        rng = np.random.default_rng(seed + 100 * d)
        h[f] = P.rounded(synth.np_flow(rng, B, H, W, "smooth"), tname if flow_t == "T" else "fp32")
        h[x] = synth.np_image(rng, B, C, H, W)
        h[k] = P.rounded(synth.np_filter(rng, B, H, W, fs), tname)
        h[o] = P.rounded(np_occlusion(rng, B, H, W), tname)
    t = {n: dev(h[n], torch.float32 if n[0] == "x" else (FT if n[0] == "f" else T)) for n in BLEND_NAMES}
    return h, t


def warp_module(*a):
    from my_package.modules.FilterInterpolationModule import FilterInterpolationModule
    return FilterInterpolationModule()(*a)


def blend_module(*a):
    from my_package.modules.FilterInterpolationBlendModule import FilterInterpolationBlendModule
    return FilterInterpolationBlendModule()(*a)


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("shape", [(2, 3, 40, 64), (1, 3, 96, 256)], ids=["2x3x40x64", "1x3x96x256"])
def test_the_layers_take_the_mixed_route(oracle, monkeypatch, shape, tname, flow_t):
    h, t = module_inputs(shape, 16, tname, flow_t, 61)
    spy = Spies(monkeypatch)
    out = warp_module(t["x0"], t["f0"], t["k0"])
    torch.cuda.synchronize()
    assert spy.mx_warp.calls == 1 and spy.mx_warp.returns == [0] and spy.f32_calls() == 0 and spy.lp_calls() == 0
    assert out.dtype == torch.float32
    want0 = oracle.filter_interpolation_forward(h["x0"], h["f0"], h["k0"])
    close(N(out), want0, "layer mx warp", RTOL)
    out = blend_module(*[t[n] for n in BLEND_NAMES])
    torch.cuda.synchronize()
    assert spy.mx_blend.calls == 1 and spy.mx_blend.returns == [0] and spy.mx_warp.calls == 1
    assert spy.f32_calls() == 0 and spy.lp_calls() == 0
    assert out.dtype == torch.float32
    want2 = oracle.filter_interpolation_forward(h["x2"], h["f1"], h["k1"])
    want = ((h["o0"] * want0).astype(np.float32) + (h["o1"] * want2).astype(np.float32)).astype(np.float32)
    close(N(out), want, "layer mx blend", RTOL)


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("shape,taps", [((2, 3, 24, 23), 16), ((2, 5, 24, 32), 16), ((2, 3, 24, 32), 4)],
                         ids=["W23", "C5", "4taps"])
def test_uncovered_mixed_calls_keep_the_promoted_route(monkeypatch, shape, taps, tname):
    _h, t = module_inputs(shape, taps, tname, "T", 67)
    spy = Spies(monkeypatch)
    out = warp_module(t["x0"], t["f0"], t["k0"])
    promoted = warp_module(t["x0"], t["f0"].float(), t["k0"].float())
    assert out.dtype == torch.float32 and torch.equal(out, promoted)
    out = blend_module(*[t[n] for n in BLEND_NAMES])
    promoted = blend_module(*[t[n].float() for n in BLEND_NAMES])
    assert out.dtype == torch.float32 and torch.equal(out, promoted)
    torch.cuda.synchronize()
    assert all(r == 1 for r in spy.mx_warp.returns + spy.mx_blend.returns), (spy.mx_warp.returns, spy.mx_blend.returns)
    assert spy.lp_calls() == 0 and spy.f32_calls() > 0


@pytest.mark.parametrize("tname", TNAMES)
def test_a_declined_view_takes_the_promoted_route_inside_the_function(monkeypatch, tname):
    """A covered shape whose taps the library cannot read (a contiguous tensor two bytes off): return 1, then the casts and
    the fp32 kernels -- the promoted call's bits."""
    _h, t = module_inputs((2, 3, 40, 64), 16, tname, "fp32", 71)
    k0, k1 = shifted_by_one(t["k0"]), shifted_by_one(t["k1"])
    assert k0.is_contiguous() and k0.data_ptr() % 8 == 2
    spy = Spies(monkeypatch)
    out = warp_module(t["x0"], t["f0"], k0)
    assert spy.mx_warp.returns == [1] and spy.f32[0].calls == 1
    assert torch.equal(out, warp_module(t["x0"], t["f0"], t["k0"].float()))
    out = blend_module(*[dict(t, k0=k0, k1=k1)[n] for n in BLEND_NAMES])
    assert spy.mx_blend.returns == [1] and spy.f32[1].calls == 1
    assert torch.equal(out, blend_module(*[t[n].float() for n in BLEND_NAMES]))


@pytest.mark.parametrize("tname", TNAMES)
def test_pure_calls_never_touch_the_mixed_library(monkeypatch, tname):
    T = DTYPES[tname]
    _h, t = module_inputs((2, 3, 40, 64), 16, tname, "fp32", 73)
    spy = Spies(monkeypatch)
    for cast in (torch.float32, T):
        warp_module(t["x0"].to(cast), t["f0"], t["k0"].to(cast))
        blend_module(*[t[n] if n[0] == "f" else t[n].to(cast) for n in BLEND_NAMES])
    torch.cuda.synchronize()
    assert spy.mx_calls() == 0 and spy.f32_calls() == 2 and spy.lp_calls() == 2


# --------------------------------------------------------------------------------------------------------------
# 6: gradients are the promoted call's
# --------------------------------------------------------------------------------------------------------------
def leaves(t, names):
    return {n: (v.clone().requires_grad_(True) if n in names else v) for n, v in t.items()}


def promoted_grads(run, t, names, order, gout):
    """the same tensors promoted by hand: float32 leaves, the float32 Function, each gradient rounded to its input's dtype"""
    p = {n: (v.float().requires_grad_(True) if n in names else v.float()) for n, v in t.items()}
    run(*[p[n] for n in order]).backward(gout)
    return {n: p[n].grad.to(t[n].dtype) for n in names}


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("image_grad", [False, True], ids=["frames-are-data", "frame-gradient"])
def test_warp_gradients_are_the_promoted_calls(oracle, monkeypatch, tname, flow_t, image_grad):
    h, t = module_inputs((2, 3, 40, 64), 16, tname, flow_t, 79)
    names = ("f0", "k0") + (("x0",) if image_grad else ())
    gout_h = np.random.default_rng(5).standard_normal((2, 3, 40, 64)).astype(np.float32)
    gout = dev(gout_h)
    m = leaves(t, names)
    spy = Spies(monkeypatch)
    warp_module(m["x0"], m["f0"], m["k0"]).backward(gout)
    assert spy.mx_warp.returns == [0]
    want = promoted_grads(warp_module, t, names, ("x0", "f0", "k0"), gout)
    torch.cuda.synchronize()
    for n in ("f0", "k0"):
        assert m[n].grad.dtype == t[n].dtype and torch.equal(m[n].grad, want[n]), n
    if image_grad:                                           # atomics: the oracle, under the closeness rule
        assert m["x0"].grad.dtype == torch.float32
        g1, _g2, _g3 = oracle.filter_interpolation_backward(h["x0"], h["f0"], h["k0"], gout_h)
        close(N(m["x0"].grad), g1, "mx warp grad image", RTOL)
    else:
        assert m["x0"].grad is None


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("image_grad", [False, True], ids=["frames-are-data", "frame-gradient"])
def test_blend_gradients_are_the_promoted_calls(oracle, monkeypatch, tname, flow_t, image_grad):
    import my_package._ext.my_lib_blend_grad as BG
    from my_package.functions import FilterInterpolationBlendLayer as BL
    h, t = module_inputs((2, 3, 40, 64), 16, tname, flow_t, 83)
    names = BLEND_NAMES[2:] + (("x0",) if image_grad else ())
    gout_h = np.random.default_rng(6).standard_normal((2, 3, 40, 64)).astype(np.float32)
    gout = dev(gout_h)
    m = leaves(t, names)
    out = blend_module(*[m[n] for n in BLEND_NAMES])
    fused = Spy(monkeypatch, BG, "FilterInterpolationBlendLayer_gpu_backward")
    composed = Spy(monkeypatch, BL, "_direction_backward")
    out.backward(gout)
    torch.cuda.synchronize()
    if image_grad:                                           # direction 0 composed, direction 1 fused
        assert fused.calls == 1 and fused.returns == [0] and composed.calls == 1
    else:
        assert fused.calls == 2 and fused.returns == [0, 0] and composed.calls == 0
    want = promoted_grads(blend_module, t, names, BLEND_NAMES, gout)
    torch.cuda.synchronize()
    for n in BLEND_NAMES[2:]:
        assert m[n].grad.dtype == t[n].dtype and torch.equal(m[n].grad, want[n]), n
    assert m["x2"].grad is None
    if image_grad:
        assert m["x0"].grad.dtype == torch.float32
        g1, _g2, _g3 = oracle.filter_interpolation_backward(h["x0"], h["f0"], h["k0"], (gout_h * h["o0"]).astype(np.float32))
        close(N(m["x0"].grad), g1, "mx blend grad image", RTOL)
    else:
        assert m["x0"].grad is None


# --------------------------------------------------------------------------------------------------------------
# 7: the network under autocast
# --------------------------------------------------------------------------------------------------------------
def star(training):
    _netutil.purge_networks()
    import networks
    assert "memc-net_amd" in networks.__file__
    net = networks.MEMC_Net_star(channel=3, filter_size=4, training=training)
    net.load_state_dict(_netutil.named_weights(net.state_dict()), strict=True)
    return net.cuda().train() if training else net.cuda().eval()


def test_autocast_inference_blends_on_the_mixed_kernel(monkeypatch):
    net = star(False)
    x = _netutil.frames(7, 1, 128, 128).cuda()
    spy = Spy(monkeypatch, MX(), "FilterInterpolationBlendLayer_gpu_forward_mx")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        frames_out, _flows, filters, _occlusions = net(x)
    torch.cuda.synchronize()
    assert spy.calls >= 1 and all(r == 0 for r in spy.returns), (spy.calls, spy.returns)
    assert all(f.dtype in (torch.float16, torch.float32) for f in frames_out)
    assert frames_out[1].dtype == torch.float32 and frames_out[1].shape == (1, 3, 128, 128)
    assert all(bool(torch.isfinite(f.float()).all()) for f in frames_out)
    assert filters[0].dtype == torch.float16


def test_autocast_training_step_has_finite_gradients(monkeypatch):
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    net = star(True)
    spy = Spy(monkeypatch, MX(), "FilterInterpolationBlendLayer_gpu_forward_mx")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        losses, _f, _k, _o = net(_netutil.training_frames(5, 1, 128, 128).cuda())
        total = sum(l.float().abs().mean() for l in losses)
    total.backward()
    torch.cuda.synchronize()
    assert spy.calls >= 1 and all(r == 0 for r in spy.returns), (spy.calls, spy.returns)
    grads = [(n, p.grad) for n, p in net.named_parameters() if p.grad is not None]
    assert grads
    bad = [n for n, g in grads if not bool(torch.isfinite(g.float()).all())]
    assert not bad, bad
