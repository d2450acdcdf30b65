"""The fp16 / bf16 bilinear warp (libmemc_hip_lp_bl.so, my_lib_lp_bl, the `native_half` route of InterpolationLayer /
InterpolationChLayer) on the GPU.  The cases: tests/_lp_bl_cases.py; their premises: tests/test_lp_bl_cases.py.

  * forward, bit for bit against the float32 library: got == fp32_forward(x.float(), flow.float()).to(T) for both dtypes,
    both flow storages, every random case and channel count, the output pre-filled with NaN, the kernel family named;
  * forward against the oracle: the exact-arithmetic cases `torch.equal` to the oracle rounded once; one ordinary case
    under tests/_netcalls.rule_rounded;
  * widths 6 and 10 and a view two elements into its buffer take bl_fwd_lp:direct with the same bit-equality;
  * padded views (row stride W + 64) of image, flow and output: the dense result, twice, nothing written behind a row;
  * backward: gradinput2 `torch.equal` to the float32 library's on the widened inputs rounded once to the flow's dtype, from
    a NaN-filled buffer; gradinput1 (a float32 buffer, added into) against the oracle under tests/_parity.close, on the
    exact cases `torch.equal`; a buffer of ones comes back as ones plus the gradient; C = 8, width 10 and a misaligned view
    return 1 and leave sentinel-filled outputs untouched;
  * the layers: dtypes, bit-equality of the two routes, the route through the bindings, what autograd keeps, the declined
    C = 8 backward, float32 calls.
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

import _lp_bl_cases as C      # noqa: E402
import _netcalls as NC        # noqa: E402
import _parity as P           # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
FLOWS = ("flowT", "flow32")               # the flow stored in T, or in float32
TILED_C3, TILED_CHUNKS, DIRECT, BWD = "bl_fwd_lp:tiled_c3", "bl_fwd_lp:tiled_chunks", "bl_fwd_lp:direct", "bl_bwd_lp:tiled_c3"


def F32():
    import my_package._ext.my_lib as M
    return M


def LPB():
    import my_package._ext.my_lib_lp_bl as M
    return M


def D(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)


def flow_dtype(T, fl):
    return T if fl == "flowT" else torch.float32


def differing(got, want):
    g, w = got.detach().float().cpu(), want.detach().float().cpu()
    bad = ~((g == w) | (torch.isnan(g) & torch.isnan(w)))
    if not bool(bad.any()):
        return "equal"
    first = tuple(int(i) for i in torch.nonzero(bad)[0])
    return "%d of %d elements differ (%d NaN in got); first at %s: got %r, want %r" % (
        int(bad.sum()), bad.numel(), int(torch.isnan(g).sum()), first, float(g[first]), float(w[first]))


def entry(kind, channels):
    """the Interpolation entry point for RGB, the InterpolationCh one otherwise"""
    return ("InterpolationLayer" if channels == 3 else "InterpolationChLayer") + "_gpu_" + kind


def lp_forward(x, flow, out, path, name=None):
    assert getattr(LPB(), (name or entry("forward", x.size(1))) + "_lp")(x, flow, out) == 0
    assert LPB().last_kernel_path() == path
    return out


def fp32_forward(x32, flow32):
    out = torch.full_like(x32, NAN)
    assert getattr(F32(), entry("forward", x32.size(1)))(x32, flow32, out) == 0
    return out


def lp_backward(x, flow, gout, gin1, gin2, ret=0, name=None):
    assert getattr(LPB(), (name or entry("backward", x.size(1))) + "_lp")(x, flow, gout, gin1, gin2) == ret
    if ret == 0:
        assert LPB().last_kernel_path() == BWD
    return gin1, gin2


def fp32_backward(x32, flow32, gout32):
    g1, g2 = torch.zeros_like(x32), torch.full_like(flow32, NAN)
    assert getattr(F32(), entry("backward", x32.size(1)))(x32, flow32, gout32, g1, g2) == 0
    return g1, g2


_ONCE = {}


def once(key, make):
    if key not in _ONCE:
        _ONCE[key] = make()
    return _ONCE[key]


def tiled_path(channels):
    return TILED_C3 if channels == 3 else TILED_CHUNKS


# ==================================================================================================================
# forward
# ==================================================================================================================
@pytest.mark.parametrize("fl", FLOWS)
@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("channels", C.FWD_CHANNELS)
@pytest.mark.parametrize("case", C.RANDOM, ids=C.RANDOM_IDS)
def test_forward_bit_for_bit_against_the_float32_library(case, channels, tname, fl):
    T = DTYPES[tname]
    xn, fn, _g = C.random_inputs(case, channels, tname)
    x, flow = D(xn, T), D(fn, flow_dtype(T, fl))
    want = fp32_forward(x.float(), flow.float()).to(T)
    got = lp_forward(x, flow, torch.full_like(x, NAN), tiled_path(channels))
    torch.cuda.synchronize()
    assert got.dtype == T and not bool(torch.isnan(want).any())
    assert torch.equal(got, want), differing(got, want)


@pytest.mark.parametrize("fl", FLOWS)
@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("name", C.EXACT_IDS + [C.EXACT_C8])
def test_forward_exact_inputs_against_the_oracle(oracle, name, tname, fl):
    T = DTYPES[tname]
    xn, fn, _g = C.exact_inputs(name, tname)
    x, flow = D(xn, T), D(fn, flow_dtype(T, fl))
    assert torch.equal(x.float().cpu(), torch.from_numpy(xn)) and torch.equal(flow.float().cpu(), torch.from_numpy(fn))
    fwd = oracle.interpolation_forward if xn.shape[1] == 3 else oracle.interpolation_ch_forward
    want = once(("fwd", name, tname), lambda: torch.from_numpy(fwd(xn, fn))).to(T)
    got = lp_forward(x, flow, torch.full_like(x, NAN), tiled_path(xn.shape[1]))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want), "%s %s: %s" % (name, tname, differing(got, want))


@pytest.mark.parametrize("tname", C.TNAMES)
def test_forward_ordinary_inputs_against_the_oracle(oracle, tname):
    T = DTYPES[tname]
    xn, fn, _g = C.random_inputs(C.ORDINARY, 3, tname)
    got = lp_forward(D(xn, T), D(fn, T), torch.full((2, 3, 20, 72), NAN, dtype=T, device="cuda"), TILED_C3)
    torch.cuda.synchronize()
    print(NC.rule_rounded(got, oracle.interpolation_forward(xn, fn), T, "Interpolation forward %s 2x3x20x72" % tname))


def narrow_inputs(W, channels, tname):
    return C.random_inputs((2, 12, W, "smooth", 2.0, 320 + W), channels, tname)


@pytest.mark.parametrize("fl", FLOWS)
@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("channels", [3, 5])
@pytest.mark.parametrize("W", [6, 10])
def test_forward_other_widths_take_the_direct_kernel(W, channels, tname, fl):
    T = DTYPES[tname]
    xn, fn, _g = narrow_inputs(W, channels, tname)
    x, flow = D(xn, T), D(fn, flow_dtype(T, fl))
    want = fp32_forward(x.float(), flow.float()).to(T)
    got = lp_forward(x, flow, torch.full_like(x, NAN), DIRECT)
    torch.cuda.synchronize()
    assert torch.equal(got, want), differing(got, want)


def shifted(t, fill=None):
    """t's values (or `fill`) in a contiguous view two elements into a buffer filled with 7: (view, buffer)"""
    buf = torch.full((t.numel() + 8,), 7.0, dtype=t.dtype, device="cuda")
    v = buf[2:2 + t.numel()].view(t.shape)
    if fill is None:
        v.copy_(t)
    else:
        v.fill_(fill)
    assert v.data_ptr() % 8 == 2 * t.element_size() and v.is_contiguous()
    return v, buf


@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("which", ["image", "flow", "output"])
def test_forward_a_view_two_elements_into_its_buffer_takes_the_direct_kernel(which, tname):
    T = DTYPES[tname]
    xn, fn, _g = C.random_inputs(C.ORDINARY, 3, tname)
    x, flow = D(xn, T), D(fn, T)
    want = fp32_forward(x.float(), flow.float()).to(T)
    out, obuf = torch.full_like(x, NAN), None
    if which == "image":
        x, _ = shifted(x)
    elif which == "flow":
        flow, _ = shifted(flow)
    else:
        out, obuf = shifted(x, NAN)
    lp_forward(x, flow, out, DIRECT)
    torch.cuda.synchronize()
    assert torch.equal(out, want), differing(out, want)
    if obuf is not None:
        assert bool((obuf[:2] == 7.0).all()) and bool((obuf[-6:] == 7.0).all())


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


@pytest.mark.parametrize("fl", FLOWS)
@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("channels", [3, 5])
def test_forward_padded_views_and_run_to_run(channels, tname, fl):
    T = DTYPES[tname]
    xn, fn, _g = C.random_inputs(C.ORDINARY, channels, tname)
    W = xn.shape[3]
    x, flow = D(xn, T), D(fn, flow_dtype(T, fl))
    dense = lp_forward(x, flow, torch.full_like(x, NAN), tiled_path(channels))
    (xv, xbuf), (fv, fbuf) = padded(x), padded(flow)
    runs = []
    for rnd in range(2):
        ov, obuf = padded(x, NAN)
        lp_forward(xv, fv, ov, tiled_path(channels))
        torch.cuda.synchronize()
        assert torch.equal(ov, dense), "round %d: %s" % (rnd, differing(ov, dense))
        for k, buf in (("image", xbuf), ("flow", fbuf), ("output", obuf)):
            assert bool((buf[:, :, :, W:] == 7.0).all()), "round %d: the bytes behind a row of %s were written" % (rnd, k)
        runs.append(ov.clone())
    assert torch.equal(runs[0], runs[1])
    assert torch.equal(xv, x) and torch.equal(fv, flow)


# ==================================================================================================================
# backward
# ==================================================================================================================
def oracle_backward(oracle, key, xn, fn, gn):
    return once(("bwd",) + key, lambda: tuple(torch.from_numpy(np.asarray(a)) for a in oracle.interpolation_backward(xn, fn, gn)))


@pytest.mark.parametrize("fl", FLOWS)
@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("case", C.RANDOM, ids=C.RANDOM_IDS)
def test_backward_ordinary_inputs(oracle, case, tname, fl):
    """the flow gradient bit for bit against the float32 library, the image gradient (float32) against the oracle"""
    T = DTYPES[tname]
    FT = flow_dtype(T, fl)
    xn, fn, gn = C.random_inputs(case, 3, tname)
    x, flow, gout = D(xn, T), D(fn, FT), D(gn, T)
    _w1, w2 = fp32_backward(x.float(), flow.float(), gout.float())
    assert F32().last_kernel_path() == "bl_bwd:tiled_c3"
    g1, g2 = lp_backward(x, flow, gout, torch.zeros_like(x, dtype=torch.float32), torch.full_like(flow, NAN))
    torch.cuda.synchronize()
    assert g2.dtype == FT and not bool(torch.isnan(w2).any())
    assert torch.equal(g2, w2.to(FT)), differing(g2, w2.to(FT))
    o1, o2 = oracle_backward(oracle, (case, tname), xn, fn, gn)
    P.close(g1, o1.cuda(), "half Interpolation gradinput1 %s %s" % (tname, fl))
    print(NC.by_dtype(g2, o2, FT, "half Interpolation gradinput2 %s %s" % (tname, fl), 3 * P.RTOL))


@pytest.mark.parametrize("fl", FLOWS)
@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("name", C.EXACT_IDS)
def test_backward_exact_inputs_against_the_oracle(oracle, name, tname, fl):
    """any order of the sums gives the same bits on these inputs (tests/_exact.py): both gradients `torch.equal`; a buffer
    holding ones comes back as ones plus the gradient, exactly"""
    T = DTYPES[tname]
    FT = flow_dtype(T, fl)
    xn, fn, gn = C.exact_inputs(name, tname)
    x, flow, gout = D(xn, T), D(fn, FT), D(gn, T)
    o1, o2 = oracle_backward(oracle, (name, tname), xn, fn, gn)
    _w1, w2 = fp32_backward(x.float(), flow.float(), gout.float())
    g1, g2 = lp_backward(x, flow, gout, torch.zeros_like(x, dtype=torch.float32), torch.full_like(flow, NAN))
    h1, h2 = lp_backward(x, flow, gout, torch.ones_like(x, dtype=torch.float32), torch.full_like(flow, NAN))
    torch.cuda.synchronize()
    assert torch.equal(g2, w2.to(FT)), differing(g2, w2.to(FT))
    assert torch.equal(g2.cpu(), o2.to(FT)), differing(g2, o2.to(FT))
    assert torch.equal(g1.cpu(), o1), differing(g1, o1)
    assert torch.equal(h1.cpu(), o1 + 1.0), differing(h1, o1 + 1.0)
    assert torch.equal(h2, g2)


@pytest.mark.parametrize("tname", C.TNAMES)
def test_backward_adds_into_the_image_gradient(oracle, tname):
    """ordinary inputs: ones plus the gradient, within the image gradient's own rule (one fp32 rounding of the sum, 6e-8 of
    it, lies far inside)"""
    T = DTYPES[tname]
    xn, fn, gn = C.random_inputs(C.IID_BWD, 3, tname)
    x, flow, gout = D(xn, T), D(fn, T), D(gn, T)
    o1, _o2 = oracle_backward(oracle, (C.IID_BWD, tname), xn, fn, gn)
    h1, _h2 = lp_backward(x, flow, gout, torch.ones_like(x, dtype=torch.float32), torch.full_like(flow, NAN))
    torch.cuda.synchronize()
    P.close(h1, (o1 + 1.0).cuda(), "half Interpolation gradinput1 += %s" % tname)


def _declined(x, flow, gout, name=None):
    g1 = torch.full_like(x, 7.0, dtype=torch.float32)
    g2 = torch.full_like(flow, 7.0)
    before = LPB().last_kernel_path()
    lp_backward(x, flow, gout, g1, g2, ret=1, name=name)
    torch.cuda.synchronize()
    assert bool((g1 == 7.0).all()) and bool((g2 == 7.0).all()), "a declined call wrote its outputs"
    assert LPB().last_kernel_path() == before


@pytest.mark.parametrize("fl", FLOWS)
@pytest.mark.parametrize("tname", C.TNAMES)
def test_backward_declines_what_it_does_not_cover(tname, fl):
    T = DTYPES[tname]
    FT = flow_dtype(T, fl)
    # eight channels through InterpolationCh
    xn, fn, gn = C.random_inputs(C.ORDINARY, C.DECLINED_CHANNELS, tname)
    _declined(D(xn, T), D(fn, FT), D(gn, T))
    # width 10
    xn, fn, gn = narrow_inputs(10, 3, tname)
    _declined(D(xn, T), D(fn, FT), D(gn, T))
    _declined(D(xn, T), D(fn, FT), D(gn, T), name="InterpolationChLayer_gpu_backward")
    # a view two elements into its buffer: the image, gradoutput, a half flow
    xn, fn, gn = C.random_inputs(C.ORDINARY, 3, tname)
    x, flow, gout = D(xn, T), D(fn, FT), D(gn, T)
    _declined(shifted(x)[0], flow, gout)
    _declined(x, flow, shifted(gout)[0])
    if FT == T:
        _declined(x, shifted(flow)[0], gout)


# ==================================================================================================================
# the layers
# ==================================================================================================================
ENTRIES = [k + "_gpu_" + d for k in ("InterpolationLayer", "InterpolationChLayer") for d in ("forward", "backward")]


class Spy:
    """records (binding, entry, return code, kernel path) of the bilinear entry points of the two bindings"""

    def __init__(self, monkeypatch):
        self.calls = []
        for lib_name, module, suffix in (("my_lib", F32(), ""), ("my_lib_lp_bl", LPB(), "_lp")):
            for e in ENTRIES:
                monkeypatch.setattr(module, e + suffix, self._wrap(lib_name, module, getattr(module, e + suffix), e + suffix))

    def _wrap(self, lib_name, module, real, name):
        def spy(*args):
            ret = real(*args)
            self.calls.append((lib_name, name, ret, module.last_kernel_path()))
            return ret
        return spy


def layer_classes(channels):
    from my_package.functions import InterpolationChLayer as LC
    from my_package.functions import InterpolationLayer as L3
    from my_package.modules.InterpolationChModule import InterpolationChModule
    from my_package.modules.InterpolationModule import InterpolationModule
    if channels == 3:
        return L3.InterpolationLayer, InterpolationModule, "InterpolationLayer"
    return LC.InterpolationChLayer, InterpolationChModule, "InterpolationChLayer"


def run_layer(Module, x, flow, gout):
    xl, fl_ = x.clone().requires_grad_(True), flow.clone().requires_grad_(True)
    out = Module()(xl, fl_)
    saved = tuple(out.grad_fn.saved_tensors) if hasattr(out.grad_fn, "saved_tensors") else None
    out.backward(gout)
    torch.cuda.synchronize()
    return out.detach(), xl.grad, fl_.grad, saved, out.grad_fn


@pytest.mark.parametrize("fl", FLOWS)
@pytest.mark.parametrize("tname", C.TNAMES)
def test_layer_takes_the_half_kernels_and_equals_the_widened_route(oracle, monkeypatch, tname, fl):
    Layer, Module, label = layer_classes(3)
    assert Layer.native_half is True and layer_classes(8)[0].native_half is True      # profiles/r22_half_bilinear.txt
    T = DTYPES[tname]
    FT = flow_dtype(T, fl)
    xn, fn, gn = C.random_inputs(C.ORDINARY, 3, tname)
    x, flow, gout = D(xn, T), D(fn, FT), D(gn, T)
    o1, o2 = oracle_backward(oracle, (C.ORDINARY, tname), xn, fn, gn)
    # the widened route: the switch off
    monkeypatch.setattr(Layer, "native_half", False)
    spy = Spy(monkeypatch)
    w_out, w_g1, w_g2, _saved, w_fn = run_layer(Module, x, flow, gout)
    assert [c[:3] for c in spy.calls] == [("my_lib", label + "_gpu_forward", 0), ("my_lib", label + "_gpu_backward", 0)], spy.calls
    monkeypatch.undo()
    # the native route
    monkeypatch.setattr(Layer, "native_half", True)
    spy = Spy(monkeypatch)
    out, g1, g2, saved, fn_ = run_layer(Module, x, flow, gout)
    assert spy.calls == [("my_lib_lp_bl", label + "_gpu_forward_lp", 0, TILED_C3),
                         ("my_lib_lp_bl", label + "_gpu_backward_lp", 0, BWD)], spy.calls
    assert "LpFunction" in type(fn_).__name__ and "LpFunction" not in type(w_fn).__name__
    assert (out.dtype, g1.dtype, g2.dtype) == (T, T, FT) and (w_out.dtype, w_g1.dtype, w_g2.dtype) == (T, T, FT)
    assert tuple(t.dtype for t in saved) == (T, FT)                         # as the network holds them: no float32 copy
    assert [tuple(t.shape) for t in saved] == [tuple(x.shape), tuple(flow.shape)]
    assert torch.equal(out, w_out), differing(out, w_out)
    assert torch.equal(g2, w_g2), differing(g2, w_g2)
    for what, g in (("native", g1), ("widened", w_g1)):
        print(NC.rule_rounded(g, o1, T, "%s image gradient, %s route %s %s" % (label, what, tname, fl)))
    print(NC.by_dtype(g2, o2, FT, "%s flow gradient %s %s" % (label, tname, fl), 3 * P.RTOL))


@pytest.mark.parametrize("tname", C.TNAMES)
def test_layer_falls_back_where_the_backward_declines(oracle, monkeypatch, tname):
    """eight channels through InterpolationCh: the half forward (chunks), the declined backward, the float32 backward on the
    widened saved tensors -- and the oracle's gradients"""
    Layer, Module, label = layer_classes(8)
    T = DTYPES[tname]
    xn, fn, gn = C.random_inputs(C.ORDINARY, 8, tname)
    x, flow, gout = D(xn, T), D(fn, T), D(gn, T)
    spy = Spy(monkeypatch)
    out, g1, g2, saved, _fn = run_layer(Module, x, flow, gout)
    assert [c[:3] for c in spy.calls] == [("my_lib_lp_bl", label + "_gpu_forward_lp", 0),
                                          ("my_lib_lp_bl", label + "_gpu_backward_lp", 1),
                                          ("my_lib", label + "_gpu_backward", 0)], spy.calls
    assert spy.calls[0][3] == TILED_CHUNKS
    assert tuple(t.dtype for t in saved) == (T, T) and (out.dtype, g1.dtype, g2.dtype) == (T, T, T)
    want = fp32_forward(x.float(), flow.float()).to(T)
    assert torch.equal(out, want), differing(out, want)
    o1, o2 = (torch.from_numpy(np.asarray(a)) for a in oracle.interpolation_ch_backward(xn, fn, gn))
    print(NC.rule_rounded(g1, o1, T, "InterpolationCh C8 image gradient %s" % tname))
    print(NC.rule_rounded(g2, o2, T, "InterpolationCh C8 flow gradient %s" % tname, 3 * P.RTOL))


@pytest.mark.parametrize("channels", [3, 8])
def test_float32_calls_and_mixed_calls_never_touch_the_half_binding(monkeypatch, channels):
    Layer, Module, label = layer_classes(channels)
    xn, fn, gn = C.random_inputs(C.ORDINARY, channels, "fp16")
    spy = Spy(monkeypatch)
    out, g1, g2, _saved, fn_ = run_layer(Module, D(xn), D(fn), D(gn))
    assert "Function" in type(fn_).__name__ and "LpFunction" not in type(fn_).__name__
    assert (out.dtype, g1.dtype, g2.dtype) == (torch.float32,) * 3
    # a float32 image beside a half flow: host_widened
    out, g1, g2, _saved, _fn = run_layer(Module, D(xn), D(fn, torch.float16), D(gn))
    assert (out.dtype, g1.dtype, g2.dtype) == (torch.float32, torch.float32, torch.float16)
    assert len(spy.calls) == 4 and all(c[0] == "my_lib" and c[2] == 0 for c in spy.calls), spy.calls
