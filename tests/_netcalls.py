"""tests/_netcalls.py -- what a NETWORK hands the operators, recorded call by call, and the rules the records are held to.

`Recorder` is a context manager.  For the duration of one network run it wraps `forward` of every
`my_package.modules._operator_module.OperatorModule` subclass and records, per call: the module class and its constructor
options; per input the dtype, shape, strides, `data_ptr() % 16`, `requires_grad` and a detached clone; the outputs as
detached clones; and, where an output requires grad, the gradoutput autograd delivers to this call and the gradient this
call returns for each input.  The per-input gradient is taken by a hook on a private alias of the input (`t.view_as(t)`:
same dtype, strides and data_ptr) that only this call consumes -- a hook on the network's own tensor would see the sum over
all its consumers.  It also replaces every `*_gpu_*` entry point of the bindings in LIBS by a spy that forwards to it and
keeps the entry point's name, its return code, the library's `last_kernel_path()` right after the call and which tensor
arguments were None.

The rules (`check_call`) compare a record with oracle/memc_oracle (fp32) on the recorded inputs widened exactly to float32;
a blend is (o0 * w0) + (o1 * w2) formed in float32.  By result dtype:

    float32                                tests/_parity.close, rtol = RTOL (3 x RTOL for image gradients)
    T from the half forward kernels        |got - want| <= ulp_T(want) / 2 + 2e-5 * max(1, |want|), same non-finite pattern
                                           (tests/test_gpu_lowp_parity.check); the bit-equal share is reported, not asserted
    any other T (gradients, host_widened)  |got - want| <= B + ulp_T(|want| + B) / 2, B = _parity's bound for the element:
                                           one rounding of an fp32 value that meets the project's rule

Every tensor compared must have max |want| >= 100 x ATOL (`not_vacuous`): below that the absolute rule would pass zeros.
tests/test_netcall_rules.py shows on the CPU that these rules fail when they should.
"""
import importlib
import os
import pkgutil
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from _parity import ATOL, BIG, RTOL, close      # noqa: E402

MANT = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}      # (mantissa bits, smallest normal exponent)
LOWP = tuple(MANT)
MIN_WANT = 100 * ATOL
LIBS = ("my_lib", "my_lib_lp", "my_lib_lp_grad", "my_lib_mx", "my_lib_mx_grad", "my_lib_blend_grad", "my_lib_mx_blend_grad")
WARP, BLEND, PROJECTION = "FilterInterpolationModule", "FilterInterpolationBlendModule", "FlowProjectionModule"
BLEND_NAMES = ("input0", "input2", "flow0", "flow1", "filter0", "filter1", "occlusion0", "occlusion1")


# ---- the records ------------------------------------------------------------------------------------------------------
class Input:
    def __init__(self, name, t):
        self.name, self.dtype, self.shape, self.strides = name, t.dtype, tuple(t.shape), tuple(t.stride())
        self.align16, self.requires_grad = t.data_ptr() % 16, t.requires_grad
        self.value = t.detach().clone()
        self.grad = None                        # what THIS call returned for the input (set by the alias's hook)


class Call:
    def __init__(self, index, cls, options, grad_mode):
        self.index, self.cls, self.options, self.grad_mode = index, cls, options, grad_mode
        self.inputs, self.outputs, self.out_requires_grad, self.gradoutputs, self.lib_calls = [], [], [], [], []

    def label(self):
        return "call %d %s" % (self.index, self.cls)

    def describe(self):
        ins = ", ".join("%s %s%s" % (i.name, str(i.dtype).replace("torch.", ""), " grad" if i.requires_grad else "")
                        for i in self.inputs)
        outs = ", ".join(str(o.dtype).replace("torch.", "") for o in self.outputs)
        return "%s%r (%s) -> %s via %s" % (self.cls, tuple(self.options.values()), ins, outs,
                                          ", ".join("%s=%d %s" % (c.entry, c.ret, c.path) for c in self.lib_calls) or "-")


class LibCall:
    def __init__(self, lib, entry, ret, path, none_args, call):
        self.lib, self.entry, self.ret, self.path, self.none_args = lib, entry, ret, path, none_args
        self.call = call                        # index of the operator call whose forward made it; None: a backward pass

    def __repr__(self):
        return "%s.%s=%d %r%s" % (self.lib, self.entry, self.ret, self.path, "" if self.call is not None else " (backward)")


def operator_classes():
    """every OperatorModule subclass of my_package.modules (one per file; the package's __init__ imports none)"""
    import my_package.modules as pkg
    from my_package.modules._operator_module import OperatorModule
    for info in pkgutil.iter_modules(pkg.__path__):
        if info.name.endswith("Module"):
            importlib.import_module("my_package.modules." + info.name)
    return list(OperatorModule.__subclasses__())


class Recorder:
    def __init__(self):
        self.calls, self.lib_calls, self._undo, self._current = [], [], [], None

    # -- the bindings
    def _spy(self, lib_name, module, entry):
        real = getattr(module, entry)

        def spy(*args, **kwargs):
            ret = real(*args, **kwargs)
            rec = LibCall(lib_name, entry, ret, module.last_kernel_path(), tuple(i for i, a in enumerate(args) if a is None),
                          None if self._current is None else self._current.index)
            self.lib_calls.append(rec)
            if self._current is not None:
                self._current.lib_calls.append(rec)
            return ret
        setattr(module, entry, spy)
        self._undo.append((module, entry, real))

    # -- the operator modules
    def _wrap(self, cls):
        real = cls.forward
        recorder = self

        def forward(module, *args, **kwargs):
            if kwargs or recorder._current is not None:          # (the networks call positionally, and never nest)
                return real(module, *args, **kwargs)
            call = Call(len(recorder.calls), cls.__name__, {name: getattr(module, name) for name, _ in cls.options},
                        torch.is_grad_enabled())
            recorder.calls.append(call)
            aliases = []
            for name, t in zip(cls.tensors, args):
                rec = Input(name, t)
                call.inputs.append(rec)
                if t.requires_grad and call.grad_mode:
                    alias = t.view_as(t)
                    assert (alias.dtype, alias.stride(), alias.data_ptr()) == (t.dtype, t.stride(), t.data_ptr())
                    alias.register_hook(lambda g, rec=rec: setattr(rec, "grad", g.detach().clone()))
                    aliases.append(alias)
                else:
                    aliases.append(t)
            recorder._current = call
            try:
                out = real(module, *aliases)
            finally:
                recorder._current = None
            for k, o in enumerate(out if isinstance(out, (tuple, list)) else (out,)):
                call.outputs.append(o.detach().clone())
                call.out_requires_grad.append(o.requires_grad)
                call.gradoutputs.append(None)
                if o.requires_grad:
                    o.register_hook(lambda g, k=k: call.gradoutputs.__setitem__(k, g.detach().clone()))
            return out
        cls.forward = forward
        self._undo.append((cls, "forward", real))

    def __enter__(self):
        try:
            for name in LIBS:
                module = importlib.import_module("my_package._ext." + name)
                for entry in dir(module):
                    if "_gpu_" in entry and callable(getattr(module, entry)):
                        self._spy(name, module, entry)
            for cls in operator_classes():
                self._wrap(cls)
        except BaseException:
            self.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, *exc):
        while self._undo:
            owner, name, real = self._undo.pop()
            setattr(owner, name, real)
        return False

    def lib(self, lib=None, entry=None, backward=None):
        """the spied calls, filtered: by binding, by entry point, by pass (backward=True: made outside every forward)"""
        return [c for c in self.lib_calls if (lib is None or c.lib == lib) and (entry is None or c.entry == entry)
                and (backward is None or (c.call is None) == backward)]

    def of(self, cls):
        return [c for c in self.calls if c.cls == cls]


# ---- the rules --------------------------------------------------------------------------------------------------------
def ulp(want, dtype):
    """the spacing of `dtype` at |want| (tests/test_gpu_lowp_parity.ulp)"""
    mant, emin = MANT[dtype]
    _, e = torch.frexp(want)                                   # |want| in [2^(e-1), 2^e)
    e = torch.clamp(e - 1, min=emin)
    return torch.ldexp(torch.ones_like(want), e - mant)


def _host(a):
    if isinstance(a, torch.Tensor):
        return a.detach().float().cpu().contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def widen(t):
    """a recorded tensor as the oracle takes it: float32 numpy, every value exact"""
    return _host(t).numpy()


def not_vacuous(want, what):
    w = _host(want)
    w = torch.where(torch.isfinite(w), w.abs(), torch.zeros_like(w))
    top = float(w.max()) if w.numel() else 0.0
    assert top >= MIN_WANT, ("%s: max |want| = %.3g is below %.0e (100 x ATOL): under the absolute rule a tensor of zeros would "
                             "pass -- scale the inputs (loss constant, frames), not the tolerance" % (what, top, MIN_WANT))
    return top


def parity_bound(want, rtol):
    """_parity's bound per element: ATOL up to |want| = 10, max(ATOL, rtol * |want|) beyond"""
    aw = want.abs()
    return torch.where(aw <= BIG, torch.full_like(aw, ATOL), torch.clamp(rtol * aw, min=ATOL))


def _same_layout(got, want, dtype, what):
    assert isinstance(got, torch.Tensor), "%s: no tensor (got %r)" % (what, got)
    assert got.dtype == dtype, "%s: dtype %s, expected %s" % (what, got.dtype, dtype)
    assert tuple(got.shape) == tuple(want.shape), "%s: shape %s, expected %s" % (what, tuple(got.shape), tuple(want.shape))


def _stats(rule, what, err, bound, want, got, dtype):
    ratio = torch.where(bound > 0, err / bound, torch.zeros_like(err))
    k = int(ratio.argmax()) if ratio.numel() else 0
    exact = float((got == want.to(dtype).float()).float().mean()) if dtype in MANT else None
    return {"rule": rule, "what": what, "max_err": float(err.max()), "err_over_bound": float(ratio.reshape(-1)[k]),
            "max_want": float(want.abs().max()), "bit_equal": exact}


def rule_float32(got, want, what, rtol=RTOL):
    want = _host(want)
    _same_layout(got, want, torch.float32, what)
    not_vacuous(want, what)
    got = _host(got)
    close(got.numpy(), want.numpy(), what, rtol)
    fin = torch.isfinite(want) & torch.isfinite(got)
    return _stats("float32", what, (got - want).abs()[fin], parity_bound(want, rtol)[fin], want[fin], got[fin], torch.float32)


def _finite_pairs(got, want, what):
    fin = torch.isfinite(want)
    assert torch.equal(torch.isinf(got) & ~fin, torch.isinf(want) & ~fin), "%s: other infinities than the oracle's" % what
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "%s: other NaNs than the oracle's" % what
    return got[fin], want[fin]


def _within(rule, got, want, bound, dtype, what):
    err = (got - want).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        k = int(torch.where(bad, err - bound, torch.full_like(err, -1.0)).argmax())
        raise AssertionError("%s: %d element(s) beyond the bound; worst: got %.9g, want %.9g, err %.3g, bound %.3g"
                             % (what, int(bad.sum()), float(got[k]), float(want[k]), float(err[k]), float(bound[k])))
    return _stats(rule, what, err, bound, want, got, dtype)


def rule_lp_forward(got, want, dtype, what):
    """a result in T from the half forward kernels"""
    want = _host(want)
    _same_layout(got, want, dtype, what)
    not_vacuous(want, what)
    g, w = _finite_pairs(_host(got), want, what)
    return _within("lp forward", g, w, 0.5 * ulp(w, dtype) + 2e-5 * torch.clamp(w.abs(), min=1.0), dtype, what)


def rule_rounded(got, want, dtype, what, rtol=RTOL):
    """any other result in T: an fp32 value within _parity's bound of the oracle, rounded once"""
    want = _host(want)
    _same_layout(got, want, dtype, what)
    not_vacuous(want, what)
    g, w = _finite_pairs(_host(got), want, what)
    b = parity_bound(w, rtol)
    return _within("rounded", g, w, b + 0.5 * ulp(w.abs() + b, dtype), dtype, what)


def by_dtype(got, want, dtype, what, rtol=RTOL):
    if dtype == torch.float32:
        return rule_float32(got, want, what, rtol)
    return rule_rounded(got, want, dtype, what, rtol)


# ---- expected values: the fp32 oracle on the widened record -----------------------------------------------------------------
def _oracle():
    from oracle import memc_oracle
    memc_oracle.build()
    return memc_oracle


def expected_forward(cls, options, inputs):
    """the outputs of one operator call, float32 numpy; inputs: the recorded values (any dtype)"""
    O, a = _oracle(), [widen(t) for t in inputs]
    if cls == WARP:
        return [O.filter_interpolation_forward(*a)]
    if cls == BLEND:
        w0 = O.filter_interpolation_forward(a[0], a[2], a[4])
        w2 = O.filter_interpolation_forward(a[1], a[3], a[5])
        return [((a[6] * w0).astype(np.float32) + (a[7] * w2).astype(np.float32)).astype(np.float32)]
    if cls == PROJECTION:
        return [O.flow_projection_forward(a[0], 1 if options["requires_grad"] == False else 0)[0]]     # noqa: E712
    raise AssertionError("no oracle route for %s: a reduced-precision network is not expected to call it" % cls)


def expected_backward(cls, options, inputs, gradoutput):
    """the gradient of one operator call for each input, float32 numpy"""
    O, a, g = _oracle(), [widen(t) for t in inputs], widen(gradoutput)
    if cls == WARP:
        return list(O.filter_interpolation_backward(a[0], a[1], a[2], g))
    if cls == BLEND:
        grads = [None] * 8
        for d in (0, 1):
            x, flow, filt, occ = a[d::2]
            gx, gflow, gfilt = O.filter_interpolation_backward(x, flow, filt, (g * occ).astype(np.float32))
            gocc = (g * O.filter_interpolation_forward(x, flow, filt)).sum(axis=1, keepdims=True)
            grads[d::2] = gx, gflow, gfilt, gocc
        return grads
    if cls == PROJECTION:
        count = O.flow_projection_forward(a[0], 0)[1]
        return [O.flow_projection_backward(a[0], count, g)]
    raise AssertionError("no oracle route for %s" % cls)


IMAGE_INPUTS = {WARP: (0,), BLEND: (0, 1), PROJECTION: ()}
GRADOUT_RANGE = (0.1, 100.0)


def check_forward(call):
    """the outputs of a recorded call against the oracle; returns the figures per tensor"""
    want = expected_forward(call.cls, call.options, [i.value for i in call.inputs])
    assert len(want) == len(call.outputs), "%s: %d outputs" % (call.label(), len(call.outputs))
    stats = []
    for k, (got, w) in enumerate(zip(call.outputs, want)):
        what = "%s output %d" % (call.label(), k)
        if got.dtype == torch.float32:
            stats.append(rule_float32(got, w, what, RTOL))
        elif call.cls in (WARP, BLEND):
            stats.append(rule_lp_forward(got, w, got.dtype, what))
        else:
            stats.append(rule_rounded(got, w, got.dtype, what, RTOL))
    return stats


def wants_gradients(call):
    """a call whose backward pass ran: some output received a gradoutput"""
    return any(g is not None for g in call.gradoutputs)


def check_gradoutput(call):
    """the conditions the loss constant is chosen for: finite, max |g| within GRADOUT_RANGE"""
    g = call.gradoutputs[0]
    assert g is not None, "%s: no gradoutput was delivered" % call.label()
    assert g.dtype == call.outputs[0].dtype and g.shape == call.outputs[0].shape, call.label()
    assert bool(torch.isfinite(g).all()), "%s: the gradoutput is not finite" % call.label()
    top = float(g.float().abs().max())
    assert GRADOUT_RANGE[0] <= top <= GRADOUT_RANGE[1], "%s: max |gradoutput| = %.3g outside %s" % (call.label(), top, GRADOUT_RANGE)
    return top


def check_backward(call):
    """every gradient a recorded call returned against the oracle, and the structure: frames (an input without
    requires_grad) got none, every input with requires_grad got one of its own dtype and shape"""
    want = expected_backward(call.cls, call.options, [i.value for i in call.inputs], call.gradoutputs[0])
    stats = []
    for k, (rec, w) in enumerate(zip(call.inputs, want)):
        what = "%s grad %s" % (call.label(), rec.name)
        if not rec.requires_grad:
            assert rec.grad is None, "%s: a gradient for an input that asked for none" % what
            continue
        assert rec.grad is not None, "%s: autograd wanted a gradient and got None" % what
        assert tuple(rec.grad.shape) == rec.shape, "%s: shape %s, the input's is %s" % (what, tuple(rec.grad.shape), rec.shape)
        stats.append(by_dtype(rec.grad, w, rec.dtype, what, 3 * RTOL if k in IMAGE_INPUTS[call.cls] else RTOL))
    return stats


# ---- the promoted call, replayed -----------------------------------------------------------------------------------------
def promoted_gradients(call, composed=False):
    """The explicitly promoted call on clones of the record: every tensor widened, the float32 layer, each gradient cast to
    its input's dtype.  composed: ask for the image gradients too, so that a float32 blend composes each direction from the
    warp's entry points (the arithmetic the pure-half blend's docstring names) instead of taking its fused kernel."""
    import my_package.modules as pkg     # noqa: F401
    cls = getattr(importlib.import_module("my_package.modules." + call.cls), call.cls)
    leaves = []
    for k, rec in enumerate(call.inputs):
        t = rec.value.clone().float()
        leaves.append(t.requires_grad_(rec.requires_grad or (composed and k in IMAGE_INPUTS[call.cls])))
    out = cls(*call.options.values())(*leaves)
    out.backward(call.gradoutputs[0].clone().float())
    torch.cuda.synchronize()
    return [None if not rec.requires_grad else t.grad.to(rec.dtype) for rec, t in zip(call.inputs, leaves)]
