"""The fp16 / bf16 depth projection backward (libmemc_hip_lp_dproj_grad.so, my_lib_lp_dproj_grad,
_DepthFlowProjectionLpFunction) on the GPU.

  * bit for bit against the float32 library: both gradients == fp32_backward(widened inputs).to(T), outputs pre-filled with
    NaN, count and forward output from the float32 forward on the widened flow and depth (fillhole = 0) -- the claim of the
    header;
  * the exact-arithmetic cases (tests/_lp_dproj_cases.py; premises: tests/test_lp_dproj_grad_cases.py) against the oracle,
    `torch.equal`: synthetic counts +-2^e and exactly 0 elsewhere, so a wrong read is inf or NaN; the cases outside the
    coverage return 1 and leave sentinel-filled outputs untouched;
  * ordinary inputs against the oracle under tests/_netcalls.rule_rounded, both gradients (the reference alone passes it
    there: tests/test_lp_dproj_grad_cases.py);
  * padded views (row stride W + 64) of every T tensor -- and of the float32 forward output, which the layout rule holds
    to the flow's element strides -- : the dense results, twice, nothing written behind a row; a view two elements into
    its buffer is declined, for each of the five T tensors;
  * the layer: dtype, bit-equality with the widened route, the route through the two bindings, what autograd keeps, the
    declined width, the switch, float32 calls and a half flow beside a float32 depth on their old routes.
Every case is milliseconds of GPU time; expectations are computed once per session.
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

import _exact as E             # noqa: E402
import _lp_dproj_cases as C    # noqa: E402
import _netcalls as NC         # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
PATH = "dproj_bwd_lp:tiled"
ENTRY = "DepthFlowProjectionLayer_gpu_backward_lp"
ENTRY32 = "DepthFlowProjectionLayer_gpu_backward"
T_NAMES = ("flow", "depth", "gout", "gin1", "gin2")


def F32():
    import my_package._ext.my_lib as M
    return M


def LPD():
    import my_package._ext.my_lib_lp_dproj_grad as M
    return M


def D(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)


def differing(got, want):
    g, w = got.detach().float().cpu(), want.detach().float().cpu()
    bad = ~((g == w) | (torch.isnan(g) & torch.isnan(w)))
    if not bool(bad.any()):
        return "equal"
    first = tuple(int(i) for i in torch.nonzero(bad)[0])
    return "%d of %d elements differ (%d NaN in got); first at %s: got %r, want %r" % (
        int(bad.sum()), bad.numel(), int(torch.isnan(g).sum()), first, float(g[first]), float(w[first]))


def lp_call(flow, depth, count, out, gout, gin1, gin2, ret=0):
    """the new entry point; asserts its return code and, for an enqueued call, the kernel family"""
    assert LPD().DepthFlowProjectionLayer_gpu_backward_lp(flow, depth, count, out, gout, gin1, gin2) == ret
    if ret == 0:
        assert LPD().last_kernel_path() == PATH
    return gin1, gin2


def fp32_forward(flow32, depth32):
    """(count, output) of the float32 forward (fillhole = 0) on a float32 flow and depth"""
    count = flow32.new_empty((flow32.size(0), 1, flow32.size(2), flow32.size(3)))
    out = torch.empty_like(flow32)
    ws = F32().flow_projection_workspace(flow32, 0, depth=True)
    assert F32().DepthFlowProjectionLayer_gpu_forward_ws(flow32, depth32, count, out, 0, ws) == 0
    return count, out


def fp32_backward(flow32, depth32, count, out, gout32):
    gin1, gin2 = torch.full_like(flow32, NAN), torch.full_like(depth32, NAN)
    assert F32().DepthFlowProjectionLayer_gpu_backward(flow32, depth32, count, out, gout32, gin1, gin2) == 0
    assert F32().last_kernel_path() == "dproj_bwd:tiled"
    return gin1, gin2


_ONCE = {}


def once(key, make):
    if key not in _ONCE:
        _ONCE[key] = make()
    return _ONCE[key]


# ==================================================================================================================
# bit for bit against the float32 library
# ==================================================================================================================
@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("case", C.RANDOM, ids=C.RANDOM_IDS)
def test_bit_for_bit_against_the_float32_library(case, tname):
    T = DTYPES[tname]
    flow, depth, gout = (D(a, T) for a in C.random_inputs(case, tname))
    count, out = fp32_forward(flow.float(), depth.float())
    want = [w.to(T) for w in fp32_backward(flow.float(), depth.float(), count, out, gout.float())]
    got = lp_call(flow, depth, count, out, gout, torch.full_like(flow, NAN), torch.full_like(depth, NAN))
    torch.cuda.synchronize()
    for g, w, n in zip(got, want, ("gradinput1", "gradinput2")):
        assert g.dtype == T and not bool(torch.isnan(w).any())
        assert torch.equal(g, w), "%s: %s" % (n, differing(g, w))


# ==================================================================================================================
# exact-arithmetic inputs against the oracle
# ==================================================================================================================
def want_exact(oracle, name, tname):
    def make():
        h = C.exact_inputs(name, tname)
        return tuple(torch.from_numpy(g) for g in
                     oracle.depth_flow_projection_backward(h["flow"], h["depth"], h["count"], h["fwd_out"], h["gout"]))
    return once(("exact", name, tname), make)


@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("name", C.COVERED)
def test_exact_inputs_against_the_oracle(oracle, name, tname):
    """which branches a case reaches: tests/test_lp_dproj_grad_cases.py::test_the_exact_cases_reach_every_branch_of_the_kernel"""
    T = DTYPES[tname]
    h = C.exact_inputs(name, tname)
    flow, depth, gout = D(h["flow"], T), D(h["depth"], T), D(h["gout"], T)
    assert torch.equal(flow.float().cpu(), torch.from_numpy(h["flow"]))      # the half tensor IS the case's flow
    got = lp_call(flow, depth, D(h["count"]), D(h["fwd_out"]), gout, torch.full_like(flow, NAN), torch.full_like(depth, NAN))
    torch.cuda.synchronize()
    for g, w, n in zip(got, want_exact(oracle, name, tname), ("gradinput1", "gradinput2")):
        assert torch.equal(g.cpu(), w.to(T)), "%s %s %s: %s" % (name, tname, n, differing(g, w.to(T)))


@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("name", C.DECLINED)
def test_cases_outside_the_coverage_are_declined_untouched(name, tname):
    T = DTYPES[tname]
    h = E.proj_bwd_inputs(name, True)
    flow, depth, gout = D(h["flow"], T), D(h["depth"], T), D(h["gout"], T)
    before = LPD().last_kernel_path()
    gin1, gin2 = lp_call(flow, depth, D(h["count"]), D(h["fwd_out"]), gout, torch.full_like(flow, 7.0),
                         torch.full_like(depth, 7.0), ret=1)
    torch.cuda.synchronize()
    assert bool((gin1 == 7.0).all()) and bool((gin2 == 7.0).all()), "a declined call wrote its output"
    assert LPD().last_kernel_path() == before


# ==================================================================================================================
# ordinary inputs against the oracle
# ==================================================================================================================
@pytest.mark.parametrize("tname", C.TNAMES)
def test_ordinary_inputs_against_the_oracle(oracle, tname):
    T = DTYPES[tname]
    flow, depth, gout = C.random_inputs(C.ORDINARY, tname)
    wout, wcount = oracle.depth_flow_projection_forward(flow, depth, 0)
    want = oracle.depth_flow_projection_backward(flow, depth, wcount, wout, gout)
    tf, td = D(flow, T), D(depth, T)
    count, out = fp32_forward(tf.float(), td.float())
    got = lp_call(tf, td, count, out, D(gout, T), torch.full_like(tf, NAN), torch.full_like(td, NAN))
    torch.cuda.synchronize()
    for g, w, n in zip(got, want, ("gradinput1", "gradinput2")):
        print(NC.rule_rounded(g, w, T, "DepthFlowProjection backward %s 2x2x20x72 %s" % (tname, n)))


# ==================================================================================================================
# views
# ==================================================================================================================
def padded(t, value=None):
    """t's values (or `value`) in rows 64 elements longer, in a buffer of t's dtype filled with 7: (view, buffer)"""
    B, Ch, H, W = t.shape
    buf = torch.full((B, Ch, H, W + 64), 7.0, dtype=t.dtype, device="cuda")
    view = buf[:, :, :, :W]
    if value is None:
        view.copy_(t)
    else:
        view.fill_(value)
    assert not view.is_contiguous() and view.stride(2) == W + 64
    return view, buf


@pytest.mark.parametrize("tname", C.TNAMES)
def test_padded_views_and_run_to_run(oracle, tname):
    """every T tensor in rows 64 elements longer; so is the float32 forward output, which must have the flow's element
    strides (a dense one beside a padded flow is malformed: -1, asserted here); the count keeps its own dense layout"""
    name, T = "2x100x132-smooth8", DTYPES[tname]
    h = C.exact_inputs(name, tname)
    W = h["flow"].shape[3]
    dense = {"flow": D(h["flow"], T), "depth": D(h["depth"], T), "gout": D(h["gout"], T), "out": D(h["fwd_out"])}
    views = {k: padded(v) for k, v in dense.items()}
    count = D(h["count"])
    want = [w.to(T) for w in want_exact(oracle, name, tname)]
    v = {k: views[k][0] for k in views}
    runs = []
    for rnd in range(2):
        (g1, g1buf), (g2, g2buf) = padded(dense["flow"], NAN), padded(dense["depth"], NAN)
        lp_call(v["flow"], v["depth"], count, v["out"], v["gout"], g1, g2)
        torch.cuda.synchronize()
        for g, w, n in ((g1, want[0], "gradinput1"), (g2, want[1], "gradinput2")):
            assert torch.equal(g.cpu(), w), "round %d, %s: %s" % (rnd, n, differing(g, w))
        for k, buf in [(k, b) for k, (_v, b) in views.items()] + [("gradinput1", g1buf), ("gradinput2", g2buf)]:
            assert bool((buf[:, :, :, W:] == 7.0).all()), "round %d: the bytes behind a row of %s were written" % (rnd, k)
        runs.append((g1.clone(), g2.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in dense:                                       # the inputs themselves are untouched
        assert torch.equal(views[k][0], dense[k])
    assert torch.equal(count.cpu(), torch.from_numpy(h["count"]))
    # the dense call gives the same bits
    d1, d2 = lp_call(dense["flow"], dense["depth"], count, dense["out"], dense["gout"], torch.full_like(dense["flow"], NAN),
                     torch.full_like(dense["depth"], NAN))
    assert torch.equal(d1, runs[0][0]) and torch.equal(d2, runs[0][1])
    # a dense forward output beside a padded flow is not of the flow's layout: rejected before the device, nothing written
    g1, _b1 = padded(dense["flow"], 7.0)
    g2, _b2 = padded(dense["depth"], 7.0)
    lp_call(v["flow"], v["depth"], count, dense["out"], v["gout"], g1, g2, ret=-1)
    torch.cuda.synchronize()
    assert bool((g1 == 7.0).all()) and bool((g2 == 7.0).all())


@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("which", T_NAMES)
def test_a_view_two_elements_into_its_buffer_is_declined(which, tname):
    T = DTYPES[tname]
    B, H, W = 1, 8, 16
    ch = {"flow": 2, "depth": 1, "gout": 2, "gin1": 2, "gin2": 1}

    def shifted(c):
        buf = torch.full((B * c * H * W + 8,), 7.0, dtype=T, device="cuda")
        v = buf[2:2 + B * c * H * W].view(B, c, H, W)
        assert v.data_ptr() % 8 == 4 and v.is_contiguous()
        return v, buf
    t = {k: (torch.zeros((B, ch[k], H, W), dtype=T, device="cuda"), None) for k in T_NAMES}
    t[which] = shifted(ch[which])
    t["gin1"][0].fill_(7.0)
    t["gin2"][0].fill_(7.0)
    count = torch.ones((B, 1, H, W), device="cuda")
    out = torch.zeros((B, 2, H, W), device="cuda")
    lp_call(t["flow"][0], t["depth"][0], count, out, t["gout"][0], t["gin1"][0], t["gin2"][0], ret=1)
    torch.cuda.synchronize()
    assert bool((t["gin1"][0] == 7.0).all()) and bool((t["gin2"][0] == 7.0).all())
    if which in ("gin1", "gin2"):
        assert bool((t[which][1] == 7.0).all())
    else:
        assert bool((t[which][1][:2] == 7.0).all()) and bool((t[which][1][-6:] == 7.0).all())


# ==================================================================================================================
# the layer
# ==================================================================================================================
class Spy:
    """records (binding, entry, return code, kernel path) of the two depth projection backward entry points"""

    def __init__(self, monkeypatch):
        self.calls = []
        for lib_name, module, entry in (("my_lib", F32(), ENTRY32), ("my_lib_lp_dproj_grad", LPD(), ENTRY)):
            monkeypatch.setattr(module, entry, self._wrap(lib_name, module, getattr(module, entry), entry))

    def _wrap(self, lib_name, module, real, entry):
        def spy(*args):
            ret = real(*args)
            self.calls.append((lib_name, entry, ret, module.last_kernel_path()))
            return ret
        return spy


def layer_classes():
    from my_package.functions import DepthFlowProjectionLayer as L
    from my_package.functions._common import host_widened
    from my_package.modules.DepthFlowProjectionModule import DepthFlowProjectionModule
    return L, host_widened, DepthFlowProjectionModule


def layer_inputs(W, tname):
    """(flow, depth, gout) on the device, in T"""
    case = (2, 20, W, "smooth", 4.0, 410 + W)
    return tuple(D(a, DTYPES[tname]) for a in C.random_inputs(case, tname))


def widened_route(flow, depth, gout):
    """host_widened around the float32 Function, called directly: the route of the switch turned off"""
    L, host_widened, _ = layer_classes()
    f, d = flow.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    out = host_widened(L._DepthFlowProjectionFunction.apply, f, f, d, 0)
    out.backward(gout)
    return out.detach(), f.grad, d.grad


def run_module(Module, flow, depth, gout):
    f, d = flow.clone().requires_grad_(True), depth.clone().requires_grad_(True)
    out = Module(True)(f, d)
    saved = tuple(out.grad_fn.saved_tensors) if hasattr(out.grad_fn, "saved_tensors") else None
    out.backward(gout)
    torch.cuda.synchronize()
    return out, f.grad, d.grad, saved


def same_as(got, want, T):
    for g, w, n in zip(got, want, ("output", "gradinput1", "gradinput2")):
        assert g.dtype == T, (n, g.dtype)
        assert torch.equal(g.detach(), w), "%s: %s" % (n, differing(g, w))


@pytest.mark.parametrize("tname", C.TNAMES)
def test_layer_takes_the_half_kernel_and_equals_the_widened_route(monkeypatch, tname):
    L, _hw, Module = layer_classes()
    T = DTYPES[tname]
    flow, depth, gout = layer_inputs(72, tname)
    want = widened_route(flow, depth, gout)
    assert L.DepthFlowProjectionLayer.native_half_backward is True      # the default (profiles/r23_half_depth_projection_backward.txt)
    spy = Spy(monkeypatch)
    out, g1, g2, saved = run_module(Module, flow, depth, gout)
    assert type(out.grad_fn).__name__.startswith("_DepthFlowProjectionLpFunction")
    same_as((out, g1, g2), want, T)
    # what autograd keeps: the flow and the depth as they are, the float32 count and forward output -- no float32 copies
    assert tuple(t.dtype for t in saved) == (T, T, torch.float32, torch.float32)
    B, _, H, W = flow.shape
    assert [tuple(t.shape) for t in saved] == [(B, 2, H, W), (B, 1, H, W), (B, 1, H, W), (B, 2, H, W)]
    assert spy.calls == [("my_lib_lp_dproj_grad", ENTRY, 0, PATH)], spy.calls


@pytest.mark.parametrize("tname", C.TNAMES)
def test_layer_falls_back_to_the_widened_arithmetic_where_the_kernel_declines(monkeypatch, tname):
    L, _hw, Module = layer_classes()
    T = DTYPES[tname]
    flow, depth, gout = layer_inputs(10, tname)
    want = widened_route(flow, depth, gout)
    monkeypatch.setattr(L.DepthFlowProjectionLayer, "native_half_backward", True)
    spy = Spy(monkeypatch)
    out, g1, g2, _saved = run_module(Module, flow, depth, gout)
    same_as((out, g1, g2), want, T)
    assert [c[:3] for c in spy.calls] == [("my_lib_lp_dproj_grad", ENTRY, 1), ("my_lib", ENTRY32, 0)], spy.calls
    assert spy.calls[1][3] == "dproj_bwd:tiled"


@pytest.mark.parametrize("tname", C.TNAMES)
def test_layer_switch_off_takes_the_float32_entry_point_only(monkeypatch, tname):
    L, _hw, Module = layer_classes()
    T = DTYPES[tname]
    flow, depth, gout = layer_inputs(72, tname)
    want = widened_route(flow, depth, gout)
    monkeypatch.setattr(L.DepthFlowProjectionLayer, "native_half_backward", False)
    spy = Spy(monkeypatch)
    out, g1, g2, _saved = run_module(Module, flow, depth, gout)
    same_as((out, g1, g2), want, T)
    assert spy.calls == [("my_lib", ENTRY32, 0, "dproj_bwd:tiled")], spy.calls


def test_float32_inputs_take_the_float32_function_unchanged(monkeypatch):
    L, _hw, Module = layer_classes()
    flow, depth, gout = (t.float() for t in layer_inputs(72, "fp16"))
    monkeypatch.setattr(L.DepthFlowProjectionLayer, "native_half_backward", True)
    spy = Spy(monkeypatch)
    out, g1, g2, _saved = run_module(Module, flow, depth, gout)
    assert type(out.grad_fn).__name__.startswith("_DepthFlowProjectionFunction")
    assert out.dtype == g1.dtype == g2.dtype == torch.float32
    assert spy.calls == [("my_lib", ENTRY32, 0, "dproj_bwd:tiled")], spy.calls


@pytest.mark.parametrize("tname", C.TNAMES)
def test_a_half_flow_beside_a_float32_depth_takes_the_widened_route_unchanged(monkeypatch, tname):
    L, _hw, Module = layer_classes()
    T = DTYPES[tname]
    flow, depth, gout = layer_inputs(72, tname)
    depth = depth.float()
    want = widened_route(flow, depth, gout)
    monkeypatch.setattr(L.DepthFlowProjectionLayer, "native_half_backward", True)
    spy = Spy(monkeypatch)
    out, g1, g2, _saved = run_module(Module, flow, depth, gout)
    assert not type(out.grad_fn).__name__.startswith("_DepthFlowProjectionLpFunction")
    assert out.dtype == T and g1.dtype == T and g2.dtype == torch.float32
    for g, w, n in zip((out, g1, g2), want, ("output", "gradinput1", "gradinput2")):
        assert torch.equal(g.detach(), w), "%s: %s" % (n, differing(g, w))
    assert spy.calls == [("my_lib", ENTRY32, 0, "dproj_bwd:tiled")], spy.calls
