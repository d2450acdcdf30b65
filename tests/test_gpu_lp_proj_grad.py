"""The fp16 / bf16 projection backward (libmemc_hip_lp_proj_grad.so, my_lib_lp_proj_grad, _FlowProjectionLpFunction) on the GPU.

  * bit for bit against the float32 library: got == fp32_backward(flow.float(), count, gout.float()).to(T), output pre-filled
    with NaN, counts from the float32 forward on the widened flow (fillhole = 0) -- the claim of the header;
  * the exact-arithmetic cases (tests/_lp_proj_cases.py; premises: tests/test_lp_proj_grad_cases.py) against the oracle,
    `torch.equal`: synthetic counts 2^e and exactly 0 elsewhere, so a wrong read is inf or NaN; the cases outside the
    coverage return 1 and leave a sentinel-filled output untouched;
  * ordinary inputs against the oracle under tests/_netcalls.rule_rounded, the bound the network tests hold this operator to;
  * padded views (row stride W + 64) of flow, gradoutput and gradient: the dense results, twice, nothing written behind a
    row; a view two elements into its buffer is declined;
  * the layer: dtype, bit-equality with the widened route, the route through the two bindings, what autograd keeps, the
    declined width, the switch;
  * one bfloat16 training step of MEMC_Net_star: both projection backward calls take the new entry point and meet the oracle.
Every case is milliseconds of GPU time; expectations are computed once per session.
"""
import copy
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

import _exact as E            # noqa: E402
import _lp_proj_cases as C    # noqa: E402
import _netcalls as NC        # noqa: E402
import _netutil               # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
PATH = "proj_bwd_lp:tiled"
ENTRY = "FlowProjectionLayer_gpu_backward_lp"


def F32():
    import my_package._ext.my_lib as M
    return M


def LPP():
    import my_package._ext.my_lib_lp_proj_grad as M
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


def lp_call(flow, count, gout, gin, ret=0):
    """the new entry point; asserts its return code and, for an enqueued call, the kernel family"""
    assert LPP().FlowProjectionLayer_gpu_backward_lp(flow, count, gout, gin) == ret
    if ret == 0:
        assert LPP().last_kernel_path() == PATH
    return gin


def fp32_forward_count(flow32):
    """count of the float32 forward (fillhole = 0) on a float32 flow"""
    count = flow32.new_empty((flow32.size(0), 1, flow32.size(2), flow32.size(3)))
    out = torch.empty_like(flow32)
    ws = F32().flow_projection_workspace(flow32, 0)
    assert F32().FlowProjectionLayer_gpu_forward_ws(flow32, count, out, 0, ws) == 0
    return count


def fp32_backward(flow32, count, gout32):
    gin = torch.full_like(flow32, NAN)
    assert F32().FlowProjectionLayer_gpu_backward(flow32, count, gout32, gin) == 0
    assert F32().last_kernel_path() == "proj_bwd:tiled"
    return gin


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
    flow, gout = (D(a, T) for a in C.random_inputs(case, tname))
    count = fp32_forward_count(flow.float())
    want = fp32_backward(flow.float(), count, gout.float()).to(T)
    got = lp_call(flow, count, gout, torch.full_like(flow, NAN))
    torch.cuda.synchronize()
    assert got.dtype == T and not bool(torch.isnan(want).any())
    assert torch.equal(got, want), differing(got, want)


# ==================================================================================================================
# exact-arithmetic inputs against the oracle
# ==================================================================================================================
def want_exact(oracle, name, tname):
    def make():
        h = C.exact_inputs(name, tname)
        return torch.from_numpy(oracle.flow_projection_backward(h["flow"], h["count"], h["gout"]))
    return once(("exact", name, tname), make)


@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("name", C.COVERED)
def test_exact_inputs_against_the_oracle(oracle, name, tname):
    """which branches a case reaches: tests/test_lp_proj_grad_cases.py::test_the_exact_cases_reach_every_branch_of_the_kernel"""
    T = DTYPES[tname]
    h = C.exact_inputs(name, tname)
    flow, gout = D(h["flow"], T), D(h["gout"], T)
    assert torch.equal(flow.float().cpu(), torch.from_numpy(h["flow"]))      # the half tensor IS the case's flow
    got = lp_call(flow, D(h["count"]), gout, torch.full_like(flow, NAN))
    torch.cuda.synchronize()
    want = want_exact(oracle, name, tname).to(T)
    assert torch.equal(got.cpu(), want), "%s %s: %s" % (name, tname, differing(got, want))


@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("name", C.DECLINED)
def test_cases_outside_the_coverage_are_declined_untouched(name, tname):
    T = DTYPES[tname]
    h = E.proj_bwd_inputs(name, False)
    flow, gout = D(h["flow"], T), D(h["gout"], T)
    before = LPP().last_kernel_path()
    gin = lp_call(flow, D(h["count"]), gout, torch.full_like(flow, 7.0), ret=1)
    torch.cuda.synchronize()
    assert bool((gin == 7.0).all()), "a declined call wrote its output"
    assert LPP().last_kernel_path() == before


# ==================================================================================================================
# ordinary inputs against the oracle
# ==================================================================================================================
@pytest.mark.parametrize("tname", C.TNAMES)
def test_ordinary_inputs_against_the_oracle(oracle, tname):
    T = DTYPES[tname]
    flow, gout = C.random_inputs(C.ORDINARY, tname)
    count = oracle.flow_projection_forward(flow, 0)[1]
    want = oracle.flow_projection_backward(flow, count, gout)
    tf = D(flow, T)
    got = lp_call(tf, fp32_forward_count(tf.float()), D(gout, T), torch.full_like(tf, NAN))
    torch.cuda.synchronize()
    print(NC.rule_rounded(got, want, T, "FlowProjection backward %s 2x2x20x72" % tname))


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
    name, T = "2x100x132-smooth8", DTYPES[tname]
    h = C.exact_inputs(name, tname)
    W = h["flow"].shape[3]
    dense = {k: D(h[k], T) for k in ("flow", "gout")}
    views = {k: padded(v) for k, v in dense.items()}
    count = D(h["count"])
    want = want_exact(oracle, name, tname).to(T)
    runs = []
    for rnd in range(2):
        g, gbuf = padded(dense["flow"], NAN)
        lp_call(views["flow"][0], count, views["gout"][0], g)
        torch.cuda.synchronize()
        assert torch.equal(g.cpu(), want), "round %d: %s" % (rnd, differing(g, want))
        for k, buf in [(k, b) for k, (_v, b) in views.items()] + [("gradinput1", gbuf)]:
            assert bool((buf[:, :, :, W:] == 7.0).all()), "round %d: the bytes behind a row of %s were written" % (rnd, k)
        runs.append(g.clone())
    assert torch.equal(runs[0], runs[1])
    for k in dense:                                       # the inputs themselves are untouched
        assert torch.equal(views[k][0], dense[k])
    # the dense call gives the same bits
    assert torch.equal(lp_call(dense["flow"], count, dense["gout"], torch.full_like(dense["flow"], NAN)), runs[0])


@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("which", ["flow", "gout", "gin"])
def test_a_view_two_elements_into_its_buffer_is_declined(which, tname):
    T = DTYPES[tname]
    B, H, W = 1, 8, 16

    def shifted():
        buf = torch.full((B * 2 * H * W + 8,), 7.0, dtype=T, device="cuda")
        v = buf[2:2 + B * 2 * H * W].view(B, 2, H, W)
        assert v.data_ptr() % 8 == 4 and v.is_contiguous()
        return v, buf
    t = {k: (torch.zeros((B, 2, H, W), dtype=T, device="cuda"), None) for k in ("flow", "gout", "gin")}
    t[which] = shifted()
    t["gin"][0].fill_(7.0)
    count = torch.ones((B, 1, H, W), device="cuda")
    lp_call(t["flow"][0], count, t["gout"][0], t["gin"][0], ret=1)
    torch.cuda.synchronize()
    assert bool((t["gin"][0] == 7.0).all())
    if t[which][1] is not None:
        assert bool((t[which][1][:2] == 7.0).all()) and bool((t[which][1][-6:] == 7.0).all())


# ==================================================================================================================
# the layer
# ==================================================================================================================
class Spy:
    """records (binding, entry, return code, kernel path) of the two projection backward entry points"""

    def __init__(self, monkeypatch):
        self.calls = []
        for lib_name, module, entry in (("my_lib", F32(), "FlowProjectionLayer_gpu_backward"), ("my_lib_lp_proj_grad", LPP(), ENTRY)):
            monkeypatch.setattr(module, entry, self._wrap(lib_name, module, getattr(module, entry), entry))

    def _wrap(self, lib_name, module, real, entry):
        def spy(*args):
            ret = real(*args)
            self.calls.append((lib_name, entry, ret, module.last_kernel_path()))
            return ret
        return spy


def layer_classes():
    from my_package.functions import FlowProjectionLayer as L
    from my_package.functions._common import host_widened
    from my_package.modules.FlowProjectionModule import FlowProjectionModule
    return L, host_widened, FlowProjectionModule


def layer_inputs(W, tname):
    case = (2, 20, W, "smooth", 4.0, 310 + W)
    return tuple(D(a, DTYPES[tname]) for a in C.random_inputs(case, tname))


def widened_route(flow, gout):
    """host_widened around the float32 Function, called directly: today's route"""
    L, host_widened, _ = layer_classes()
    leaf = flow.clone().requires_grad_(True)
    out = host_widened(L._FlowProjectionFunction.apply, leaf, leaf, 0)
    out.backward(gout)
    return out.detach(), leaf.grad


@pytest.mark.parametrize("tname", C.TNAMES)
def test_layer_takes_the_half_kernel_and_equals_the_widened_route(monkeypatch, tname):
    L, _hw, Module = layer_classes()
    assert L.FlowProjectionLayer.native_half_backward is True
    T = DTYPES[tname]
    flow, gout = layer_inputs(72, tname)
    want_out, want_grad = widened_route(flow, gout)
    spy = Spy(monkeypatch)
    leaf = flow.clone().requires_grad_(True)
    out = Module(True)(leaf)
    assert out.dtype == T and torch.equal(out.detach(), want_out)
    assert tuple(t.dtype for t in out.grad_fn.saved_tensors) == (T, torch.float32)      # no float32 flow is kept
    assert [tuple(t.shape) for t in out.grad_fn.saved_tensors] == [tuple(flow.shape), (flow.size(0), 1) + tuple(flow.shape[2:])]
    out.backward(gout)
    torch.cuda.synchronize()
    assert leaf.grad.dtype == T
    assert torch.equal(leaf.grad, want_grad), differing(leaf.grad, want_grad)
    assert spy.calls == [("my_lib_lp_proj_grad", ENTRY, 0, PATH)], spy.calls


@pytest.mark.parametrize("tname", C.TNAMES)
def test_layer_falls_back_to_the_widened_arithmetic_where_the_kernel_declines(monkeypatch, tname):
    _L, _hw, Module = layer_classes()
    T = DTYPES[tname]
    flow, gout = layer_inputs(10, tname)
    want_out, want_grad = widened_route(flow, gout)
    spy = Spy(monkeypatch)
    leaf = flow.clone().requires_grad_(True)
    out = Module(True)(leaf)
    out.backward(gout)
    torch.cuda.synchronize()
    assert out.dtype == T and torch.equal(out.detach(), want_out)
    assert leaf.grad.dtype == T and torch.equal(leaf.grad, want_grad), differing(leaf.grad, want_grad)
    assert [c[:3] for c in spy.calls] == [("my_lib_lp_proj_grad", ENTRY, 1), ("my_lib", "FlowProjectionLayer_gpu_backward", 0)], spy.calls
    assert spy.calls[1][3] == "proj_bwd:tiled"


@pytest.mark.parametrize("tname", C.TNAMES)
def test_layer_switch_off_takes_the_float32_entry_point_only(monkeypatch, tname):
    L, _hw, Module = layer_classes()
    T = DTYPES[tname]
    flow, gout = layer_inputs(72, tname)
    want_out, want_grad = widened_route(flow, gout)
    monkeypatch.setattr(L.FlowProjectionLayer, "native_half_backward", False)
    spy = Spy(monkeypatch)
    leaf = flow.clone().requires_grad_(True)
    out = Module(True)(leaf)
    out.backward(gout)
    torch.cuda.synchronize()
    assert out.dtype == T and torch.equal(out.detach(), want_out)
    assert leaf.grad.dtype == T and torch.equal(leaf.grad, want_grad)
    assert spy.calls == [("my_lib", "FlowProjectionLayer_gpu_backward", 0, "proj_bwd:tiled")], spy.calls


def test_float32_flows_take_the_float32_function_unchanged(monkeypatch):
    L, _hw, Module = layer_classes()
    flow, gout = (t.float() for t in layer_inputs(72, "fp16"))
    spy = Spy(monkeypatch)
    leaf = flow.clone().requires_grad_(True)
    out = Module(True)(leaf)
    assert type(out.grad_fn).__name__.startswith("_FlowProjectionFunction")
    out.backward(gout)
    assert leaf.grad.dtype == torch.float32
    assert spy.calls == [("my_lib", "FlowProjectionLayer_gpu_backward", 0, "proj_bwd:tiled")], spy.calls


# ==================================================================================================================
# the network
# ==================================================================================================================
def test_a_bfloat16_training_step_takes_the_half_kernel_for_both_projections(oracle, monkeypatch):
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    _netutil.purge_networks()
    import networks
    assert "memc-net_amd" in networks.__file__
    m = networks.MEMC_Net_star(channel=3, filter_size=4, training=False)
    m.load_state_dict(_netutil.named_weights(m.state_dict()), strict=True, warn_align_corners=False)
    net = copy.deepcopy(m).cuda().to(torch.bfloat16)
    x = _netutil.training_frames(5, 1, 128, 128).cuda().to(torch.bfloat16)
    with NC.Recorder() as rec:
        spy = Spy(monkeypatch)                           # over the recorder's own spy on my_lib
        net.train()
        net.zero_grad(set_to_none=True)
        losses, _f, _k, _o = net(x)
        sum(l.abs().sum() for l in losses).backward()
        torch.cuda.synchronize()
        monkeypatch.undo()
    projections = rec.of(NC.PROJECTION)
    assert len(projections) == 2
    assert spy.calls == [("my_lib_lp_proj_grad", ENTRY, 0, PATH)] * 2, spy.calls
    assert not rec.lib("my_lib", "FlowProjectionLayer_gpu_backward")
    for call in projections:
        assert call.inputs[0].dtype == torch.bfloat16 and call.inputs[0].grad.dtype == torch.bfloat16
        NC.check_gradoutput(call)
        for s in NC.check_backward(call):
            print(s)
