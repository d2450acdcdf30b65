"""Every route of the four projection entry points (FlowProjection / DepthFlowProjection, forward and backward) held to the
per-cell bounds of tests/_proj_bound.py -- a float64 restatement and a bound derived from the kernels' sources -- instead of
the 1e-4 of tests/_parity.py.  Through the C ABI, outputs pre-filled with NaN, the route asserted where the library reports
it (last_kernel_path) and, where it does not, the source condition that selects it asserted on the inputs in numpy.

Every largest err / bound is printed and appended to proj_bound_ratios.jsonl beside the parity record (the directory of
tests/_parity.log_path()); profiles/proj_bounds_observed.md keeps a copy of one run.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _parity as P          # noqa: E402
import _proj_bound as PB     # noqa: E402
from tools import synth      # noqa: E402

pytestmark = pytest.mark.gpu

K_REACH = 24                 # proj_owner5's scan reach (flow_projection.hip, launch_proj_owner5: kReach = 24)
CAP = 2496                   # proj_bwd_tiled's staged cells per 64 x 16 tile (launch_proj_bwd)


def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a GPU: the HIP path cannot be exercised (no fallback exists)")
    return torch.device("cuda:0")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def N(t):
    return t.detach().cpu().numpy()


def nan(*shape):
    return torch.full(shape, float("nan"), device=dev())


@pytest.fixture(scope="module")
def my_lib():
    import my_package._ext.my_lib as L
    return L


def held(what, r_ok, tail=0):
    """assert err / bound <= 1 over the compared cells; `tail`: the last columns first, on their own, so a failure names them"""
    r, ok = r_ok
    worst = float(r[ok].max()) if ok.any() else 0.0
    print("%-64s err / bound %.3f over %d cells" % (what, worst, int(ok.sum())))
    try:
        p = os.path.join(os.path.dirname(P.log_path()), "proj_bound_ratios.jsonl")
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "a") as f:
            f.write(json.dumps({"what": what, "ratio": worst, "cells": int(ok.sum())}) + "\n")
    except OSError:
        pass
    if tail:
        rt, okt = r[..., -tail:], ok[..., -tail:]
        assert not okt.any() or float(rt[okt].max()) <= 1.0, "%s: the last %d columns, err / bound %.3f" % (what, tail, float(rt[okt].max()))
    assert worst <= 1.0, "%s: err / bound %.3f" % (what, worst)
    return worst


_REFS = {}


def refs(d, key):
    """restatements and oracle planes of one input set: made once per module run, shared, never written"""
    if key not in _REFS:
        from oracle import memc_oracle as O
        r = {"fwd": {False: PB.Forward(d["flow"]), True: PB.Forward(d["flow"], d["depth"])}}
        assert r["fwd"][False].excluded == 0 and r["fwd"][True].excluded == 0
        out0, cnt0 = O.flow_projection_forward(d["flow"], 0)
        dout0, dcnt0 = O.depth_flow_projection_forward(d["flow"], d["depth"], 0)
        r["planes"] = {False: (cnt0, None), True: (dcnt0, dout0)}
        r["bwd"] = {False: PB.Backward(d["flow"], None, cnt0, None, d["gout"]),
                    True: PB.Backward(d["flow"], d["depth"], dcnt0, dout0, d["gout"])}
        _REFS[key] = r
    return _REFS[key]


def case_inputs(name):
    d = PB.make(PB.case(name))
    return d, refs(d, name)


def forward(my_lib, d, r, dep, fill, tag, path, tail=0, wrap=T):
    f = wrap(d["flow"])
    cnt, out = wrap(np.full_like(d["depth"], np.nan)), wrap(np.full_like(d["flow"], np.nan))
    if dep:
        assert my_lib.DepthFlowProjectionLayer_gpu_forward(f, wrap(d["depth"]), cnt, out, fill) == 0
    else:
        assert my_lib.FlowProjectionLayer_gpu_forward(f, cnt, out, fill) == 0
    got = my_lib.last_kernel_path()
    assert got == ("dproj_fwd:" if dep else "proj_fwd:") + path, got
    name = "%s %s fill %d (%s)" % (tag, "dproj" if dep else "proj", fill, got)
    held(name + " count", r["fwd"][dep].ratio_count(N(cnt)), tail)
    held(name + " out", r["fwd"][dep].ratio_out(N(out), fill), tail)
    return cnt, out


def backward(my_lib, d, r, dep, tag, path, tail=0, wrap=T):
    """the oracle's forward planes go in: the same planes the restatement got"""
    f, g = wrap(d["flow"]), wrap(d["gout"])
    cnt0, out0 = r["planes"][dep]
    gin = wrap(np.full_like(d["flow"], np.nan))
    if dep:
        gd = wrap(np.full_like(d["depth"], np.nan))
        assert my_lib.DepthFlowProjectionLayer_gpu_backward(f, wrap(d["depth"]), wrap(cnt0), wrap(out0), g, gin, gd) == 0
    else:
        assert my_lib.FlowProjectionLayer_gpu_backward(f, wrap(cnt0), g, gin) == 0
    got = my_lib.last_kernel_path()
    assert got == ("dproj_bwd:" if dep else "proj_bwd:") + path, got
    name = "%s %s (%s)" % (tag, "dproj" if dep else "proj", got)
    held(name + " gradinput1", r["bwd"][dep].ratio1(N(gin)), tail)
    if dep:
        held(name + " gradinput2", r["bwd"][dep].ratio2(N(gd)), tail)
        return gin, gd
    return gin, None


def everything(my_lib, d, r, tag, fwd_path, bwd_path, tail=0, wrap=T):
    for dep in (False, True):
        for fill in (0, 1):
            forward(my_lib, d, r, dep, fill, tag, fwd_path, tail, wrap)
        backward(my_lib, d, r, dep, tag, bwd_path, tail, wrap)


@pytest.mark.parametrize("name", ["smooth4", "smooth30"])
def test_owner_forward_and_tiled_backward(my_lib, name):
    d, r = case_inputs(name)
    everything(my_lib, d, r, name, "owner", "tiled")


def _motion(flow):
    """the image's dominant motion as proj_owner5 estimates it (motion_sample_issue / motion_round4): the mean of an 8 x 8
    grid of sites, 0 below 6 px"""
    B, _, H, W = flow.shape
    l = np.arange(64)
    xs, ys = ((2 * (l & 7) + 1) * W) >> 4, ((2 * (l >> 3) + 1) * H) >> 4
    mean = flow[:, :, ys, xs].astype(np.float64).mean(axis=2)            # [B, 2]
    return np.where(np.abs(mean) < 6.0, 0.0, 4.0 * np.rint(mean / 4.0))


def test_far_completion_of_the_owner_forward(my_lib):
    """proj_owner5 scans the sources within kReach = 24 px (relative to the image's motion m) of a tile; a valid source
    with |f - m| >= 24 on an axis is found by its home tile only, which flags the image, and proj_owner_far recomputes the
    tiles it lands in (FarTile: three float64 planes, the same readout).  The library reports `owner` for both, so the
    condition is asserted here: m == 0 for every image and some valid site of every image moves 24 px or more."""
    d = PB.make(PB.case("smooth30"))
    rng = np.random.default_rng(41)
    d["flow"] = synth.np_flow(rng, 2, 48, 96, "smooth", 3.0)
    d["flow"][:, 0, 20:30, 8:24] += np.float32(40.0)                    # a block of sites panned 40 px to the right
    assert not _motion(d["flow"]).any()
    valid = PB.locate32(d["flow"])[0]
    far = valid & (np.abs(d["flow"]).max(axis=1) >= K_REACH)
    assert far.reshape(2, -1).any(axis=1).all()
    r = refs(d, "far block")
    for dep in (False, True):
        for fill in (0, 1):
            forward(my_lib, d, r, dep, fill, "far block", "owner")


def _largest_corner_box(flow):
    """cells of the largest corner box [min L, max R] x [min T, max Bm] over the valid sites of one 64 x 16 site tile"""
    B, _, H, W = flow.shape
    valid, L, R, Tt, Bm = PB.locate32(flow)
    best = 0
    for b in range(B):
        for y0 in range(0, H, 16):
            for x0 in range(0, W & ~3, 64):
                s = (b, slice(y0, y0 + 16), slice(x0, min(x0 + 64, W & ~3)))
                v = valid[s]
                if v.any():
                    best = max(best, int((R[s][v].max() - L[s][v].min() + 1) * (Bm[s][v].max() - Tt[s][v].min() + 1)))
    return best


@pytest.mark.parametrize("name", ["iid3", "iid160"])
def test_ragged_widths_holes_and_corners_outside_the_staged_box(my_lib, name):
    """W % 4 != 0, W >= 8: the owner kernels' ragged instantiation forward; backward the tiled kernel over the whole quads and
    proj_bwd (one lane per site) over the W % 4 columns behind them -- those columns are checked on their own first.
    iid160 (flow of +-160 px on 2 x 90 x 130, the cancellation case on record) also has 77 % holes (hole filling on the
    owner route's masks), corner boxes beyond proj_bwd_tiled's CAP = 2496 staged cells (the `else` branch at
    flow_projection.hip:1238 reads such corners from global memory; the library reports `tiled` either way, so the box is
    computed here), and gradinput2 is held to its per-cell bound with no per-tensor term."""
    d, r = case_inputs(name)
    W = d["flow"].shape[3]
    assert W % 4 != 0 and W >= 8
    if name == "iid160":
        assert r["fwd"][True].holes() > 0.2
        assert _largest_corner_box(d["flow"]) > CAP
    everything(my_lib, d, r, name, "owner", "tiled", tail=W % 4)


def test_scalar_width(my_lib):
    d, r = case_inputs("scalar")
    everything(my_lib, d, r, "scalar", "scalar", "scalar")


@pytest.mark.parametrize("name", ["special", "two rows", "two columns"])
def test_special_values_and_folded_corners(my_lib, name):
    """NaN / Inf flows at a few sites (invalid: exactly zero gradients, no term anywhere); images of two rows / two columns
    with whole-pixel flows, where R == L or Bm == T hands a cell the same term twice."""
    d, r = case_inputs(name)
    W = d["flow"].shape[3]
    if name != "special":
        assert r["bwd"][True].r["touches"].any()
    path = "scalar" if W < 8 else "owner"
    everything(my_lib, d, r, name, path, "scalar" if W < 8 else "tiled", tail=W % 4 if W >= 8 else 0)


def test_a_view_two_elements_into_its_buffer(my_lib):
    """A 64-wide view that starts two elements into rows of 66: no row is 16-byte aligned.  Until round 5 such views took
    the scalar kernels; vec4_ok (memc_tile.hpp) now asks for W % 4 == 0 only and the quads are loaded with dword alignment,
    so the routes are `owner` and `tiled` (tests/test_gpu_parity.py::test_shapes_take_the_documented_kernel_paths) -- the
    unaligned staging of those kernels is what this holds to the bound."""
    rng = np.random.default_rng(77)
    B, H, W = 2, 20, 64
    d = dict(flow=synth.np_flow(rng, B, H, W, "iid", 3.0), depth=synth.np_depth(rng, B, H, W),
             gout=rng.random((B, 2, H, W), dtype=np.float32))
    r = refs(d, "view + 2")
    bufs = []

    def wrap(a):
        buf = torch.full(a.shape[:3] + (W + 2,), -3.0, device=dev())
        v = buf[..., 2:]
        v.copy_(T(a))
        assert v.data_ptr() % 16 != 0
        bufs.append(buf)
        return v
    everything(my_lib, d, r, "view + 2", "owner", "tiled", wrap=wrap)
    assert all(bool((b[..., :2] == -3.0).all()) for b in bufs)


def test_row_padded_views_leave_their_margins_alone(my_lib):
    """every tensor a window of a larger buffer (one more channel, rows and columns around it): batch, channel and row
    strides unrelated to the sizes; what surrounds a window must not change"""
    d, r = case_inputs("iid10")                                         # 2 x 33 x 131: ragged as well
    B, _, H, W = d["flow"].shape
    made = []

    def wrap(a):
        ch = a.shape[1]
        buf = torch.full((B, ch + 1, H + 3, W + 9), -3.0, device=dev())
        v = buf[:, 1:1 + ch, 2:2 + H, 5:5 + W]
        v.copy_(T(a))
        made.append((buf, ch))
        return v
    everything(my_lib, d, r, "padded views", "owner", "tiled", tail=W % 4, wrap=wrap)
    for buf, ch in made:
        inner = torch.zeros_like(buf, dtype=torch.bool)
        inner[:, 1:1 + ch, 2:2 + H, 5:5 + W] = True
        assert bool((buf[~inner] == -3.0).all())


def test_scratch_free_general_route_in_a_captured_graph(my_lib):
    """Inside a stream capture the reference-signature entry points have no scratch block (run_proj_fwd: r.flag == nullptr)
    and take the general route: zero, proj_scatter_tiled (fp32 LDS planes and fp32 atomics), proj_average_v4, and the literal
    hole walker proj_fillhole_v4.  One capture on a single stream, no parallel branches, replayed once."""
    rng = np.random.default_rng(43)
    B, H, W = 2, 48, 96
    d = dict(flow=synth.np_flow(rng, B, H, W, "iid", 40.0), depth=synth.np_depth(rng, B, H, W),
             gout=rng.random((B, 2, H, W), dtype=np.float32))
    r = refs(d, "general")
    assert r["fwd"][True].holes() > 0.2
    f, dep = T(d["flow"]), T(d["depth"])
    cnt, out, dcnt, dout = nan(B, 1, H, W), nan(B, 2, H, W), nan(B, 1, H, W), nan(B, 2, H, W)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert my_lib.FlowProjectionLayer_gpu_forward(f, cnt, out, 1) == 0
        p1 = my_lib.last_kernel_path()
        assert my_lib.DepthFlowProjectionLayer_gpu_forward(f, dep, dcnt, dout, 1) == 0
        p2 = my_lib.last_kernel_path()
    assert (p1, p2) == ("proj_fwd:general", "dproj_fwd:general"), (p1, p2)
    graph.replay()
    torch.cuda.synchronize()
    held("general proj fill 1 count", r["fwd"][False].ratio_count(N(cnt)))
    held("general proj fill 1 out", r["fwd"][False].ratio_out(N(out), 1))
    held("general dproj fill 1 count", r["fwd"][True].ratio_count(N(dcnt)))
    held("general dproj fill 1 out", r["fwd"][True].ratio_out(N(dout), 1))


def test_the_layers_with_the_library_s_own_forward_planes(my_lib):
    """FlowProjectionLayer / DepthFlowProjectionLayer forward and backward: the count and output the library's forward made
    are read back from the autograd node, and the backward's restatement is made from THOSE planes."""
    from my_package.functions.DepthFlowProjectionLayer import DepthFlowProjectionLayer
    from my_package.functions.FlowProjectionLayer import FlowProjectionLayer
    d, r = case_inputs("smooth30")
    g = T(d["gout"])
    f = T(d["flow"]).requires_grad_(True)
    out = FlowProjectionLayer(True)(f)
    _f, cnt = out.grad_fn.saved_tensors
    held("layer proj count", r["fwd"][False].ratio_count(N(cnt)))
    held("layer proj out", r["fwd"][False].ratio_out(N(out), 0))
    out.backward(g)
    held("layer proj gradinput1", PB.Backward(d["flow"], None, N(cnt), None, d["gout"]).ratio1(N(f.grad)))
    f = T(d["flow"]).requires_grad_(True)
    dep = T(d["depth"]).requires_grad_(True)
    out = DepthFlowProjectionLayer(True)(f, dep)
    _f, _d, cnt, saved = out.grad_fn.saved_tensors
    assert torch.equal(saved, out.detach())
    held("layer dproj count", r["fwd"][True].ratio_count(N(cnt)))
    held("layer dproj out", r["fwd"][True].ratio_out(N(out), 0))
    out.backward(g)
    own = PB.Backward(d["flow"], d["depth"], N(cnt), N(out), d["gout"])
    held("layer dproj gradinput1", own.ratio1(N(f.grad)))
    held("layer dproj gradinput2", own.ratio2(N(dep.grad)))
