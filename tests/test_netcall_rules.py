"""The rules of tests/_netcalls.py have teeth (CPU only: this is what shows that tests/test_gpu_lowp_network_calls.py can fail).

Records are made by hand, one small case per operator (B = 1, 3 or 8 channels, 16 x 24): seeded inputs rounded to T, the
oracle's own outputs and gradients rounded to T (or left in float32 where the mixed routes return float32).  The rules must
pass on these, and fail on: a result moved by 2 ulp_T at one element, the two directions of a blend swapped, a flow gradient
in the tap gradient's place, a gradient of zeros, a gradient that is None, and a tensor whose max |want| is below 1e-2."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _netcalls as NC       # noqa: E402
from tools import synth      # noqa: E402

H, W_ = 16, 24
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
F32 = torch.float32


def T_(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def occlusion(rng):
    return (0.25 + 0.5 * rng.random((1, 1, H, W_), dtype=np.float32)).astype(np.float32)


def record(cls, options, tensors, out_dtype, gout=None):
    """a Call as the recorder would leave it, had the operator returned the oracle's values rounded once;
    tensors: (name, tensor, requires_grad)"""
    call = NC.Call(0, cls, options, gout is not None)
    for name, t, grad in tensors:
        call.inputs.append(NC.Input(name, t.clone().requires_grad_(grad)))
    values = [i.value for i in call.inputs]
    call.outputs = [torch.from_numpy(w).to(out_dtype) for w in NC.expected_forward(cls, options, values)]
    call.out_requires_grad, call.gradoutputs = [gout is not None], [gout]
    if gout is not None:
        for rec, g in zip(call.inputs, NC.expected_backward(cls, options, values, gout)):
            if rec.requires_grad:
                rec.grad = torch.from_numpy(g).to(rec.dtype)
    return call


def warp_call(T, mixed, C=3, train=True, seed=3):
    rng = np.random.default_rng(seed)
    x = T_(synth.np_image(rng, 1, C, H, W_), F32 if mixed else T)
    flow, taps = T_(synth.np_flow(rng, 1, H, W_, "smooth"), T), T_(synth.np_filter(rng, 1, H, W_), T)
    gout = T_(rng.standard_normal((1, C, H, W_)).astype(np.float32), F32 if mixed else T) if train else None
    return record(NC.WARP, {}, [("input1", x, False), ("input2", flow, train), ("input3", taps, train)],
                  F32 if mixed else T, gout)


def blend_call(T, mixed, train=True, seed=4):
    rng = np.random.default_rng(seed)
    t = []
    for name in NC.BLEND_NAMES:
        if name.startswith("input"):
            t.append((name, T_(synth.np_image(rng, 1, 3, H, W_), F32 if mixed else T), False))
        elif name.startswith("flow"):
            t.append((name, T_(synth.np_flow(rng, 1, H, W_, "smooth"), T), train))
        elif name.startswith("filter"):
            t.append((name, T_(synth.np_filter(rng, 1, H, W_), T), train))
        else:
            t.append((name, T_(occlusion(rng), T), train))
    gout = T_(rng.standard_normal((1, 3, H, W_)).astype(np.float32), F32 if mixed else T) if train else None
    return record(NC.BLEND, {}, t, F32 if mixed else T, gout)


def projection_call(T, train, seed=5):
    rng = np.random.default_rng(seed)
    flow = T_(synth.np_flow(rng, 1, H, W_, "smooth"), T)
    gout = T_(rng.standard_normal((1, 2, H, W_)).astype(np.float32), T) if train else None
    return record(NC.PROJECTION, {"requires_grad": train}, [("input1", flow, train)], T, gout)


def cases(T):
    return {"warp mixed": warp_call(T, True), "warp half": warp_call(T, False), "context warp": warp_call(T, False, C=8, train=False),
            "blend mixed": blend_call(T, True), "blend half": blend_call(T, False),
            "projection train": projection_call(T, True), "projection infer (holes filled)": projection_call(T, False)}


def check(call):
    NC.check_forward(call)
    if NC.wants_gradients(call):
        NC.check_gradoutput(call)
        NC.check_backward(call)


def fails(call, match=None):
    with pytest.raises(AssertionError, match=match):
        check(call)


def nudge(t, ulps):
    """`t` with its largest element moved by `ulps` units of t's own format (2 ulp_T of a T tensor; for a float32 tensor the
    step that breaks the float32 rule is stated by the caller)"""
    out = t.clone()
    k = int(out.abs().argmax())
    flat = out.view(-1)
    step = NC.ulp(flat[k:k + 1].float(), t.dtype)[0] if t.dtype in NC.MANT else 0.0
    flat[k] = (flat[k].float() + ulps * step).to(t.dtype)
    return out


@pytest.mark.parametrize("tname", sorted(DTYPES))
def test_the_rules_pass_on_the_oracles_own_values_rounded_once(oracle, tname):
    for name, call in cases(DTYPES[tname]).items():
        check(call)
    assert NC.check_forward(cases(DTYPES[tname])["projection infer (holes filled)"])[0]["rule"] == "rounded"
    assert NC.check_forward(cases(DTYPES[tname])["blend half"])[0]["rule"] == "lp forward"
    assert NC.check_forward(cases(DTYPES[tname])["blend mixed"])[0]["rule"] == "float32"


def test_ulp_is_the_half_parity_modules():
    import test_gpu_lowp_parity as LP
    x = torch.tensor([0.0, 1e-8, 6.1e-5, 0.3, 1.0, 1.5, 2.0, 1000.0, 60000.0])
    for T in DTYPES.values():
        assert torch.equal(NC.ulp(x, T), LP.ulp(x, T))
    assert float(NC.ulp(torch.tensor([1.0]), torch.float16)) == 2.0 ** -10
    assert float(NC.ulp(torch.tensor([1.0]), torch.bfloat16)) == 2.0 ** -7


@pytest.mark.parametrize("tname", sorted(DTYPES))
def test_two_ulp_at_one_element_fail(oracle, tname):
    T = DTYPES[tname]
    for name in ("warp half", "context warp", "blend half", "projection train", "projection infer (holes filled)"):
        call = cases(T)[name]
        call.outputs[0] = nudge(call.outputs[0], 2)
        fails(call, "beyond the bound")
    for name, which in (("warp half", "input2"), ("warp mixed", "input3"), ("blend mixed", "occlusion1"),
                        ("blend half", "flow0"), ("projection train", "input1")):
        call = cases(T)[name]
        rec = [i for i in call.inputs if i.name == which][0]
        rec.grad = nudge(rec.grad, 2)
        fails(call, "beyond the bound")
    # float32 results: 2 ulp_T of the value is far beyond 1e-4
    call = cases(T)["blend mixed"]
    k = int(call.outputs[0].abs().argmax())
    call.outputs[0].view(-1)[k] += 2 * float(NC.ulp(call.outputs[0].view(-1)[k:k + 1], T))
    fails(call, "max abs err")


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("mixed", [True, False], ids=["mixed", "half"])
def test_swapped_blend_directions_fail(oracle, tname, mixed):
    T = DTYPES[tname]
    call = blend_call(T, mixed)
    swapped = {"flow0": "flow1", "flow1": "flow0"}
    values = {i.name: i.value for i in call.inputs}
    wrong = NC.expected_forward(NC.BLEND, {}, [values[swapped.get(n, n)] for n in NC.BLEND_NAMES])[0]
    call.outputs[0] = torch.from_numpy(wrong).to(call.outputs[0].dtype)
    fails(call)
    # the tap gradient of direction 0 handed to both directions (same shape and dtype: only the values tell)
    call = blend_call(T, mixed)
    grads = {i.name: i for i in call.inputs}
    grads["filter1"].grad = grads["filter0"].grad.clone()
    fails(call, "filter1")


@pytest.mark.parametrize("tname", sorted(DTYPES))
def test_wrong_missing_and_zero_gradients_fail(oracle, tname):
    T = DTYPES[tname]
    call = warp_call(T, True)
    call.inputs[2].grad = call.inputs[1].grad.clone()            # the flow gradient in the tap gradient's place
    fails(call, "shape")
    for name in ("warp mixed", "warp half", "blend mixed", "blend half", "projection train"):
        for k, rec in enumerate(cases(T)[name].inputs):
            if not rec.requires_grad:
                continue
            call = cases(T)[name]
            call.inputs[k].grad = torch.zeros_like(call.inputs[k].grad)
            fails(call, rec.name)
            call = cases(T)[name]
            call.inputs[k].grad = None
            fails(call, "got None")
            call = cases(T)[name]
            call.inputs[k].grad = call.inputs[k].grad.to(F32 if rec.dtype != F32 else T)
            fails(call, "dtype")
    call = warp_call(T, True)                                    # a gradient for a frame
    call.inputs[0].grad = torch.zeros_like(call.inputs[0].value)
    fails(call, "asked for none")


@pytest.mark.parametrize("tname", sorted(DTYPES))
def test_tensors_too_small_to_tell_fail(oracle, tname):
    """1e-5-sized gradients (what a .mean() loss gives): zeros would pass the absolute rule, so the rules refuse the tensor"""
    T = DTYPES[tname]
    for make in (lambda: warp_call(T, True), lambda: blend_call(T, False), lambda: projection_call(T, True)):
        call = make()
        small = (call.gradoutputs[0].float() * 1e-5).to(call.gradoutputs[0].dtype)
        tensors = [(i.name, i.value, i.requires_grad) for i in call.inputs]
        tiny = record(call.cls, call.options, tensors, call.outputs[0].dtype, small)
        NC.check_forward(tiny)
        with pytest.raises(AssertionError, match="gradoutput"):
            NC.check_gradoutput(tiny)
        with pytest.raises(AssertionError, match="100 x ATOL"):
            NC.check_backward(tiny)
        for rec in tiny.inputs:                                  # ... and indeed zeros are within 1e-4 of them
            if rec.requires_grad:
                assert float(rec.grad.float().abs().max()) < 1e-4
    with pytest.raises(AssertionError, match="100 x ATOL"):
        NC.rule_float32(torch.full((4,), 5e-3), np.full((4,), 5e-3, np.float32), "a small float32 tensor")
    with pytest.raises(AssertionError, match="100 x ATOL"):
        NC.rule_lp_forward(torch.full((4,), 5e-3, dtype=T), np.full((4,), 5e-3, np.float32), T, "a small half tensor")


def test_the_recorder_keeps_each_calls_own_gradient(hip_lib_path):
    """a tensor with three consumers: the record of a call holds what THAT call returned for it, not the sum"""
    from my_package.modules._operator_module import OperatorModule
    import my_package._ext.my_lib as my_lib

    class _Mul:
        def __call__(self, a, b):
            return a * b

    class MulModule(OperatorModule):
        layer, tensors, options = _Mul, ("a", "b"), ()

        def forward(self, a, b):
            return self.f(a, b)

    x = torch.arange(6.0).reshape(1, 1, 2, 3).requires_grad_(True)
    y = torch.full((1, 1, 2, 3), 2.0, requires_grad=True)[:, :, :, 1:]
    real, binding = MulModule.forward, my_lib.FilterInterpolationLayer_gpu_forward
    with NC.Recorder() as rec:
        assert MulModule.forward is not real and my_lib.FilterInterpolationLayer_gpu_forward is not binding
        out = MulModule()(x[:, :, :, 1:], y) + MulModule()(x, x)[:, :, :, 1:] + 3 * x[:, :, :, 1:]
        out.sum().backward()
        with torch.no_grad():
            MulModule()(x, x)
    assert MulModule.forward is real and my_lib.FilterInterpolationLayer_gpu_forward is binding
    first, second, third = rec.calls
    assert [i.strides for i in first.inputs] == [(6, 6, 3, 1)] * 2 and first.inputs[0].shape == (1, 1, 2, 2)
    assert first.inputs[0].align16 == x[:, :, :, 1:].data_ptr() % 16
    assert torch.equal(first.inputs[0].grad, y.detach()) and torch.equal(first.inputs[1].grad, x.detach()[:, :, :, 1:])
    assert torch.equal(second.inputs[0].grad, second.inputs[1].grad) and second.inputs[0].grad.shape == x.shape
    assert torch.equal(second.inputs[0].grad[:, :, :, 1:], x.detach()[:, :, :, 1:]) and not second.inputs[0].grad[:, :, :, 0].any()
    assert torch.equal(first.gradoutputs[0], torch.ones(1, 1, 2, 2)) and torch.equal(first.outputs[0], (x[:, :, :, 1:] * y).detach())
    assert not torch.equal(x.grad[:, :, :, 1:], first.inputs[0].grad)         # the network's tensor holds the sum
    assert third.grad_mode is False and third.out_requires_grad == [False] and third.gradoutputs == [None]
    assert not rec.lib_calls


def test_the_gradoutput_conditions():
    call = warp_call(torch.float16, True)
    NC.check_gradoutput(call)
    for bad in (call.gradoutputs[0] * 1000.0, call.gradoutputs[0] * 1e-3):
        call.gradoutputs[0] = bad
        with pytest.raises(AssertionError, match="outside"):
            NC.check_gradoutput(call)
    call.gradoutputs[0] = torch.full_like(bad, float("nan"))
    with pytest.raises(AssertionError, match="not finite"):
        NC.check_gradoutput(call)
