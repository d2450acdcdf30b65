"""The mixed-precision fused blend backward (libmemc_hip_mx_blend_grad.so, include/memc_warp_mx_blend_grad.h): fp32 frames
and gradoutput beside fp16 / bf16 taps and occlusions, the flow in fp32 or that dtype -- the blend's backward of the call
torch.autocast makes -- and the route FilterInterpolationBlendLayer takes for it.

Inputs are the census table of tests/_lowp_paths.py (bands in both directions, capped tiles, slow sites, split and mixed
lanes, empty tiles, 4-column edge tiles, a ragged last tile row) plus the minimum width and a wide row of mostly invalid
sites, as in test_gpu_blend_grad.py.  Taps, occlusions and half flows are rounded to T first (P.rounded); the image and
gradoutput stay fp32 as generated (not on T's grid: a kernel that read them as T would show).  Rules:
  the C entry point      each output `torch.equal` to the fp32 library's (libmemc_hip_blend_grad.so) on the widened inputs
                         after one `.to(dtype)`: no tolerance.  The fp32 kernel is the reference; the existing tests hold it
                         to the oracle;
  exact inputs           tests/_exact.py's blend inputs (numbers of fp16 and bf16 by construction): `torch.equal` to the
                         oracle's expectation rounded once with `.to(T)` -- a check that does not go through the fp32 kernel;
  the layer              gradients `torch.equal` to those of the explicitly promoted call (test_gpu_mx.promoted_grads); an
                         image gradient (atomics) against the oracle under tests/_parity.close(..., RTOL).
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

import _exact as E                           # noqa: E402
import _lowp_paths as P                      # noqa: E402
import _netutil                              # noqa: E402
from _parity import RTOL, close              # noqa: E402
from test_gpu_blend_grad import ABI_CASES, ABI_IDS, Spy, np_occlusion                    # noqa: E402
from test_gpu_exact import DIRECTIONS, exact, lowp_cases, storage, want_direction        # noqa: E402
from test_gpu_mx import (BLEND_NAMES, DTYPES, FLOWS, TNAMES, blend_module, leaves, module_inputs, promoted_grads,   # noqa: E402
                         shifted_by_one, star)
from tools import synth                      # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
PATH, F32_PATH = "fi_blend_bwd_mx:tiled_c3", "fi_blend_bwd:tiled_c3"


def MXBG():
    import my_package._ext.my_lib_mx_blend_grad as M
    return M


def BG():
    import my_package._ext.my_lib_blend_grad as M
    return M


def BL():
    from my_package.functions import FilterInterpolationBlendLayer as M
    return M


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)


def N(t):
    return t.detach().float().cpu().numpy()


def nan_like(t):
    return torch.full_like(t, NAN)


_HOST = {}


def direction(case, tname, flow_t):
    """(x, flow, taps, occ, gout) of one direction on the host, fp32 numpy: taps and occlusion rounded to T, the flow to its
    storage, image and gradoutput as generated.  Computed once, never written."""
    key = (case, tname, flow_t)
    if key not in _HOST:
        x, flow, filt, gout = P.case_inputs(case, 3)
        B, H, W = case[:3]
        occ = np_occlusion(np.random.default_rng(case[5] + 7), B, H, W)
        _HOST[key] = (x, P.rounded(flow, tname if flow_t == "T" else "fp32"), P.rounded(filt, tname), P.rounded(occ, tname),
                      gout)
    return _HOST[key]


def on_device(host, tname, flow_t):
    T = DTYPES[tname]
    FT = T if flow_t == "T" else torch.float32
    x, flow, filt, occ, gout = host
    return [dev(x), dev(flow, FT), dev(filt, T), dev(occ, T), dev(gout)]


def mixed(x, flow, filt, occ, gout, outs=None):
    """the C entry point into NaN-filled outputs: (status, gflow, gtaps, gocc)"""
    g2, g3, g4 = outs if outs is not None else (nan_like(flow), nan_like(filt), nan_like(occ))
    status = MXBG().FilterInterpolationBlendLayer_gpu_backward_mx(x, flow, filt, occ, gout, g2, g3, g4)
    torch.cuda.synchronize()
    return status, g2, g3, g4


def widened_reference(x, flow, filt, occ, gout):
    """the fp32 library on the widened inputs, each result rounded once to its input's dtype"""
    wide = (flow.float(), filt.float(), occ.float())
    outs = tuple(nan_like(t) for t in wide)
    assert BG().FilterInterpolationBlendLayer_gpu_backward(x, *wide, gout, *outs) == 0
    assert BG().last_kernel_path() == F32_PATH
    torch.cuda.synchronize()
    return tuple(o.to(t.dtype) for o, t in zip(outs, (flow, filt, occ)))


# --------------------------------------------------------------------------------------------------------------
# 1: the C entry point on every in-kernel path, bit for bit the fp32 library's
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("case", ABI_CASES, ids=ABI_IDS)
def test_c_entry_point_is_the_fp32_kernel_rounded_once(case, tname, flow_t):
    host = direction(case, tname, flow_t)
    assert not np.array_equal(P.rounded(host[0], tname), host[0]), "the image is on T's grid"
    assert not np.array_equal(P.rounded(host[4], tname), host[4]), "gradoutput is on T's grid"
    t = on_device(host, tname, flow_t)
    status, g2, g3, g4 = mixed(*t)
    assert status == 0 and MXBG().last_kernel_path() == PATH
    want = widened_reference(*t)
    for g, w, src, what in zip((g2, g3, g4), want, t[1:4], ("grad flow", "grad taps", "grad occlusion")):
        assert g.dtype == src.dtype, what
        assert not torch.isnan(g).any(), (what, "an element was not assigned")
        assert torch.equal(g, w), (what, int((g != w).sum()), g.numel())


# --------------------------------------------------------------------------------------------------------------
# 2: exact inputs against the oracle, not through the fp32 kernel
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
def test_exact_inputs_match_the_oracle_rounded_once(oracle, tname, flow_t):
    T = DTYPES[tname]
    FT = T if flow_t == "T" else torch.float32
    st = storage(tname, flow_t)
    for ci in lowp_cases(flow_t):
        h = E.blend_inputs(E.TABLE[ci], st)
        gout = dev(h["gout"])
        for d in (0, 1):
            x, f, k, o = (h[n] for n in DIRECTIONS[d])
            status, g2, g3, g4 = mixed(dev(x), dev(f, FT), dev(k, T), dev(o, T), gout)
            assert status == 0 and MXBG().last_kernel_path() == PATH
            _w1, w2, w3, w4, _w = want_direction(oracle, ("table", ci, st), h, d)
            what = "mixed blend backward %s direction %d %s flow %s" % (E.TABLE_IDS[ci], d, tname, flow_t)
            assert g2.dtype == FT and g3.dtype == T and g4.dtype == T
            exact(g2, w2, what + " flow gradient")
            exact(g3, w3, what + " tap gradient")
            exact(g4, w4, what + " occlusion gradient")


# --------------------------------------------------------------------------------------------------------------
# 3: views
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
def test_strided_views_and_run_to_run(tname, flow_t):
    """Row-padded tensors (row stride W + 64), outputs included, and an occlusion that is channel 1 of a [B, 2, H, W] half
    tensor give the dense call's bits; so does a second identical call (no atomics)."""
    host = direction(P.CASES[1], tname, flow_t)
    dense = on_device(host, tname, flow_t)
    status, g2, g3, g4 = mixed(*dense)
    assert status == 0
    status, h2, h3, h4 = mixed(*dense)
    assert status == 0
    assert torch.equal(g2, h2) and torch.equal(g3, h3) and torch.equal(g4, h4)
    pad = [synth.padded_planes(t) for t in dense]
    assert pad[2].stride(2) == host[2].shape[3] + 64 and not pad[2].is_contiguous()
    outs = tuple(synth.padded_planes(nan_like(t)) for t in dense[1:4])
    status, p2, p3, p4 = mixed(*pad, outs=outs)
    assert status == 0 and MXBG().last_kernel_path() == PATH
    assert torch.equal(g2, p2) and torch.equal(g3, p3) and torch.equal(g4, p4)
    # the occlusion (and its gradient) as channel 1 of a two-channel half tensor
    two = torch.stack((torch.full_like(dense[3][:, 0], 9.0), dense[3][:, 0]), dim=1)
    gtwo = nan_like(two)
    for _ in range(2):
        status, v2, v3, v4 = mixed(dense[0], dense[1], dense[2], two[:, 1:2], dense[4],
                                   outs=(nan_like(dense[1]), nan_like(dense[2]), gtwo[:, 1:2]))
        assert status == 0
        assert torch.equal(g2, v2) and torch.equal(g3, v3) and torch.equal(g4, v4)
        assert torch.isnan(gtwo[:, 0]).all()                 # the neighbouring channel was not touched


# --------------------------------------------------------------------------------------------------------------
# 4 - 6: the layer
# --------------------------------------------------------------------------------------------------------------
class LayerSpies:
    def __init__(self, monkeypatch):
        self.mixed = Spy(monkeypatch, MXBG(), "FilterInterpolationBlendLayer_gpu_backward_mx")
        self.f32 = Spy(monkeypatch, BG()._SAT, "call")       # every call of the float32 library's C function
        self.composed = Spy(monkeypatch, BL(), "_direction_backward")


def backward_of(t, names, gout, monkeypatch):
    m = leaves(t, names)
    out = blend_module(*[m[n] for n in BLEND_NAMES])
    spy = LayerSpies(monkeypatch)
    out.backward(gout)
    torch.cuda.synchronize()
    return m, spy


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("shape", [(2, 3, 40, 64), (1, 3, 96, 256)], ids=["2x3x40x64", "1x3x96x256"])
def test_the_layer_takes_the_mixed_kernel(monkeypatch, shape, tname, flow_t):
    _h, t = module_inputs(shape, 16, tname, flow_t, 89)
    gout = dev(np.random.default_rng(9).standard_normal(shape).astype(np.float32))
    m, spy = backward_of(t, BLEND_NAMES[2:], gout, monkeypatch)
    # every dtype and flow-storage group takes the mixed kernel: none lost to the promoted route
    # (profiles/r16_mixed_blend_backward.txt)
    assert spy.mixed.calls == 2 and spy.mixed.returns == [0, 0], (spy.mixed.calls, spy.mixed.returns)
    assert spy.f32.calls == 0 and spy.composed.calls == 0, (spy.f32.calls, spy.composed.calls)
    want = promoted_grads(blend_module, t, BLEND_NAMES[2:], BLEND_NAMES, gout)
    torch.cuda.synchronize()
    for n in BLEND_NAMES[2:]:
        assert m[n].grad.dtype == t[n].dtype and torch.equal(m[n].grad, want[n]), n
    assert m["x0"].grad is None and m["x2"].grad is None


@pytest.mark.parametrize("tname", TNAMES)
def test_a_declined_view_takes_the_promoted_route(monkeypatch, tname):
    """taps that are contiguous but two bytes off a quad: the mixed function returns 1 for that direction, which is then
    widened and run on the float32 kernel -- the promoted call's bits"""
    _h, t = module_inputs((2, 3, 40, 64), 16, tname, "fp32", 97)
    gout = dev(np.random.default_rng(10).standard_normal((2, 3, 40, 64)).astype(np.float32))
    m = leaves(t, BLEND_NAMES[2:])
    k0 = shifted_by_one(m["k0"])                             # (a copy inside the graph: its gradient reaches the leaf)
    assert k0.is_contiguous() and k0.data_ptr() % 8 == 2
    out = blend_module(*[dict(m, k0=k0)[n] for n in BLEND_NAMES])
    spy = LayerSpies(monkeypatch)
    out.backward(gout)
    torch.cuda.synchronize()
    assert spy.mixed.returns == [1, 0], spy.mixed.returns
    assert spy.f32.calls == 1 and spy.f32.returns == [0] and spy.composed.calls == 0
    want = promoted_grads(blend_module, t, BLEND_NAMES[2:], BLEND_NAMES, gout)
    torch.cuda.synchronize()
    for n in BLEND_NAMES[2:]:
        assert m[n].grad.dtype == t[n].dtype and torch.equal(m[n].grad, want[n]), n


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
def test_a_direction_whose_image_wants_a_gradient_is_composed(oracle, monkeypatch, tname, flow_t):
    shape = (2, 3, 40, 64)
    h, t = module_inputs(shape, 16, tname, flow_t, 101)
    gout_h = np.random.default_rng(11).standard_normal(shape).astype(np.float32)
    gout = dev(gout_h)
    names = BLEND_NAMES[2:] + ("x0",)
    m, spy = backward_of(t, names, gout, monkeypatch)
    assert spy.composed.calls == 1                            # direction 0, on widened tensors
    assert spy.mixed.calls == 1 and spy.mixed.returns == [0] and spy.f32.calls == 0       # direction 1
    want = promoted_grads(blend_module, t, names, BLEND_NAMES, gout)
    torch.cuda.synchronize()
    for n in BLEND_NAMES[2:]:
        assert m[n].grad.dtype == t[n].dtype and torch.equal(m[n].grad, want[n]), n
    assert m["x2"].grad is None and m["x0"].grad.dtype == torch.float32
    g1, _g2, _g3 = oracle.filter_interpolation_backward(h["x0"], h["f0"], h["k0"], (gout_h * h["o0"]).astype(np.float32))
    close(N(m["x0"].grad), g1, "mixed blend grad image", RTOL)


# --------------------------------------------------------------------------------------------------------------
# 7: the network under autocast
# --------------------------------------------------------------------------------------------------------------
def test_autocast_training_step_runs_on_the_mixed_backward(monkeypatch):
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    net = star(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        losses, _f, _k, _o = net(_netutil.training_frames(5, 1, 128, 128).cuda())
        total = sum(l.float().abs().mean() for l in losses)
    new = Spy(monkeypatch, MXBG(), "FilterInterpolationBlendLayer_gpu_backward_mx")
    composed = Spy(monkeypatch, BL(), "_direction_backward")
    total.backward()
    torch.cuda.synchronize()
    assert new.calls >= 1 and all(r == 0 for r in new.returns), (new.calls, new.returns)
    assert composed.calls == 0
    grads = [(n, p.grad) for n, p in net.named_parameters() if p.grad is not None]
    assert grads
    bad = [n for n, g in grads if not bool(torch.isfinite(g.float()).all())]
    assert not bad, bad
