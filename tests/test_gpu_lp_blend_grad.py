"""The pure fp16 / bf16 fused blend backward (libmemc_hip_lp_blend_grad.so, include/memc_warp_lp_blend_grad.h): a half image,
half taps and occlusions, the flow and gradoutput in fp32 or that dtype -- the blend's backward of a model cast to bf16 /
fp16 -- and the opt-in route FilterInterpolationBlendLayer(fused_half_backward=True) takes for it.

Inputs are the census table of tests/_lowp_paths.py (bands in both directions, capped tiles, slow sites, split and mixed
lanes, empty tiles, 4-column edge tiles, a ragged last tile row) plus the minimum width and a wide row of mostly invalid
sites, as in test_gpu_blend_grad.py.  The image, taps and occlusions and, where they are stored in T, the flow and
gradoutput are rounded to T on the host first (P.rounded); an fp32 flow or gradoutput stays as generated (not on T's grid:
a kernel that read it as T would show).  Rules:
  the C entry point      each output `torch.equal` to the fp32 library's (libmemc_hip_blend_grad.so) on the `.float()` inputs
                         after one `.to(dtype)`: no tolerance -- both sides run the same fp32 arithmetic on exactly widened
                         values.  The fp32 kernel is the reference; the existing tests hold it to the oracle;
  exact inputs           tests/_exact.py's blend inputs (numbers of fp16 and bf16 by construction): `torch.equal` to the
                         oracle's expectation rounded once with `.to(T)` -- a check that does not go through the fp32 kernel;
  the layer, switch on   flow, tap and occlusion gradients `torch.equal` to those of the fp32 layer's fused route on the widened
                         leaves, cast once (test_gpu_mx.promoted_grads); a composed direction against the oracle under
                         tests/_netcalls.py's rounded rule; a declined direction and the switch off: the default layer's bits;
  the network            tests/_netcalls.py's recorder and rules on one bf16 training step of MEMC_Net_star.
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
import _netcalls as NC                       # noqa: E402
import _netutil                              # noqa: E402
from _parity import RTOL                     # noqa: E402
from test_gpu_blend_grad import ABI_CASES, ABI_IDS, Spy, np_occlusion                    # noqa: E402
from test_gpu_exact import DIRECTIONS, exact, lowp_cases, storage, want_direction        # noqa: E402
from test_gpu_mx import BLEND_NAMES, DTYPES, FLOWS, TNAMES, leaves, module_inputs, promoted_grads, star   # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
PATH, F32_PATH = "fi_blend_bwd_lp:tiled_c3", "fi_blend_bwd:tiled_c3"
ENTRY = "FilterInterpolationBlendLayer_gpu_backward_lp"
GOUTS = ["fp32", "T"]


def LPBG():
    import my_package._ext.my_lib_lp_blend_grad as M
    return M


def BG():
    import my_package._ext.my_lib_blend_grad as M
    return M


def LPG():
    import my_package._ext.my_lib_lp_grad as M
    return M


def F32LIB():
    import my_package._ext.my_lib as M
    return M


def BL():
    from my_package.functions import FilterInterpolationBlendLayer as M
    return M


def blend_module(*a, **options):
    from my_package.modules.FilterInterpolationBlendModule import FilterInterpolationBlendModule
    return FilterInterpolationBlendModule(**options)(*a)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)


def nan_like(t):
    return torch.full_like(t, NAN)


_HOST = {}


def direction(case, tname, flow_t, gout_t):
    """(x, flow, taps, occ, gout) of one direction on the host, fp32 numpy: image, taps and occlusion rounded to T, the flow
    and gradoutput to their storage.  Computed once, never written."""
    key = (case, tname, flow_t, gout_t)
    if key not in _HOST:
        x, flow, filt, gout = P.case_inputs(case, 3)
        B, H, W = case[:3]
        occ = np_occlusion(np.random.default_rng(case[5] + 7), B, H, W)
        _HOST[key] = (P.rounded(x, tname), P.rounded(flow, tname if flow_t == "T" else "fp32"), P.rounded(filt, tname),
                      P.rounded(occ, tname), P.rounded(gout, tname if gout_t == "T" else "fp32"))
    return _HOST[key]


def on_device(host, tname, flow_t, gout_t):
    T = DTYPES[tname]
    FT = T if flow_t == "T" else torch.float32
    GT = T if gout_t == "T" else torch.float32
    x, flow, filt, occ, gout = host
    return [dev(x, T), dev(flow, FT), dev(filt, T), dev(occ, T), dev(gout, GT)]


def half(x, flow, filt, occ, gout, outs=None):
    """the C entry point into NaN-filled outputs: (status, gflow, gtaps, gocc)"""
    g2, g3, g4 = outs if outs is not None else (nan_like(flow), nan_like(filt), nan_like(occ))
    status = LPBG().FilterInterpolationBlendLayer_gpu_backward_lp(x, flow, filt, occ, gout, g2, g3, g4)
    torch.cuda.synchronize()
    return status, g2, g3, g4


def widened_reference(x, flow, filt, occ, gout):
    """the fp32 library on the widened inputs, each result rounded once to its input's dtype"""
    wide = (flow.float(), filt.float(), occ.float())
    outs = tuple(nan_like(t) for t in wide)
    assert BG().FilterInterpolationBlendLayer_gpu_backward(x.float(), *wide, gout.float(), *outs) == 0
    assert BG().last_kernel_path() == F32_PATH
    torch.cuda.synchronize()
    return tuple(o.to(t.dtype) for o, t in zip(outs, (flow, filt, occ)))


# --------------------------------------------------------------------------------------------------------------
# 1: the C entry point on every in-kernel path, bit for bit the fp32 library's
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("gout_t", GOUTS)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("case", ABI_CASES, ids=ABI_IDS)
def test_c_entry_point_is_the_fp32_kernel_rounded_once(case, tname, flow_t, gout_t):
    host = direction(case, tname, flow_t, gout_t)
    if gout_t == "fp32":
        assert not np.array_equal(P.rounded(host[4], tname), host[4]), "an fp32 gradoutput is on T's grid"
    t = on_device(host, tname, flow_t, gout_t)
    for got, h in zip(t, host):
        assert np.array_equal(got.float().cpu().numpy(), h), "the host rounding is not the storage's"
    status, g2, g3, g4 = half(*t)
    assert status == 0 and LPBG().last_kernel_path() == PATH
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
        for n in ("x0", "x2", "gout"):
            assert np.array_equal(P.rounded(h[n], tname), h[n]), (n, "not a number of T")
        for GT in (torch.float32, T):
            gout = dev(h["gout"], GT)
            for d in (0, 1):
                x, f, k, o = (h[n] for n in DIRECTIONS[d])
                status, g2, g3, g4 = half(dev(x, T), dev(f, FT), dev(k, T), dev(o, T), gout)
                assert status == 0 and LPBG().last_kernel_path() == PATH
                _w1, w2, w3, w4, _w = want_direction(oracle, ("table", ci, st), h, d)
                what = "half blend backward %s direction %d %s flow %s gradoutput %s" % (E.TABLE_IDS[ci], d, tname, flow_t, GT)
                assert g2.dtype == FT and g3.dtype == T and g4.dtype == T
                exact(g2, w2, what + " flow gradient")
                exact(g3, w3, what + " tap gradient")
                exact(g4, w4, what + " occlusion gradient")


# --------------------------------------------------------------------------------------------------------------
# 3: views
# --------------------------------------------------------------------------------------------------------------
def padded(src, fill=None):
    """(buffer, view): src's values (or `fill`) in rows 64 elements longer, the padding NaN"""
    b, c, h, w = src.shape
    buf = torch.full((b, c, h, w + 64), NAN, device=src.device, dtype=src.dtype)
    view = buf[:, :, :, :w]
    if fill is None:
        view.copy_(src)
    else:
        view.fill_(fill)
    return buf, view


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
def test_strided_views_and_run_to_run(tname, flow_t):
    """Row-padded tensors (row stride W + 64), outputs included, and an occlusion that is channel 0 of a [B, 4, H, W] half
    tensor give the dense call's bits; so does a second identical call (no atomics).  Nothing outside the views is written."""
    host = direction(P.CASES[1], tname, flow_t, "T")
    W = host[0].shape[3]
    dense = on_device(host, tname, flow_t, "T")
    status, g2, g3, g4 = half(*dense)
    assert status == 0
    status, h2, h3, h4 = half(*dense)
    assert status == 0
    assert torch.equal(g2, h2) and torch.equal(g3, h3) and torch.equal(g4, h4)
    pad = [padded(t)[1] for t in dense]
    assert pad[0].stride(2) == W + 64 and pad[2].stride(2) == W + 64 and not pad[2].is_contiguous()
    bufs, outs = zip(*(padded(t, fill=NAN) for t in dense[1:4]))
    status, p2, p3, p4 = half(*pad, outs=outs)
    assert status == 0 and LPBG().last_kernel_path() == PATH
    assert torch.equal(g2, p2) and torch.equal(g3, p3) and torch.equal(g4, p4)
    for buf in bufs:
        assert torch.isnan(buf[:, :, :, W:]).all()           # the padding was not touched
    # the occlusion (and its gradient) as channel 0 of a four-channel half tensor: the 8-byte quads stay
    four = torch.cat((dense[3], torch.full_like(dense[3], 9.0).expand(-1, 3, -1, -1)), dim=1).contiguous()
    gfour = nan_like(four)
    for _ in range(2):
        status, v2, v3, v4 = half(dense[0], dense[1], dense[2], four[:, 0:1], dense[4],
                                  outs=(nan_like(dense[1]), nan_like(dense[2]), gfour[:, 0:1]))
        assert status == 0
        assert torch.equal(g2, v2) and torch.equal(g3, v3) and torch.equal(g4, v4)
        assert torch.isnan(gfour[:, 1:]).all()               # the neighbouring channels were not touched
    assert bool((four[:, 1:] == 9.0).all())


# --------------------------------------------------------------------------------------------------------------
# 4 - 6: the layer
# --------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 3, 40, 64), (1, 3, 96, 256)]
SHAPE_IDS = ["2x3x40x64", "1x3x96x256"]


def half_inputs(shape, tname, flow_t, seed):
    """(host dict, device dict) of the blend's eight inputs: frames, taps and occlusions of T, the frames rounded on the host
    as well"""
    h, t = module_inputs(shape, 16, tname, flow_t, seed)
    T = DTYPES[tname]
    for n in ("x0", "x2"):
        h[n] = P.rounded(h[n], tname)
        t[n] = dev(h[n], T)
    return h, t


def half_gout(shape, tname, seed):
    g = P.rounded(np.random.default_rng(seed).standard_normal(shape).astype(np.float32), tname)
    return g, dev(g, DTYPES[tname])


class LayerSpies:
    def __init__(self, monkeypatch):
        self.new = Spy(monkeypatch, LPBG(), ENTRY)
        self.door = Spy(monkeypatch, BG(), "FilterInterpolationBlendLayer_gpu_backward")
        self.recompute = Spy(monkeypatch, F32LIB(), "FilterInterpolationLayer_gpu_forward")
        self.f32_backward = Spy(monkeypatch, F32LIB(), "FilterInterpolationLayer_gpu_backward")
        self.lp_grad = Spy(monkeypatch, LPG(), "FilterInterpolationLayer_gpu_backward_lp")
        self.composed = Spy(monkeypatch, BL(), "_direction_backward")
        self.widened = []                                    # (dtype, data_ptr) of every tensor .float() was called on
        real = torch.Tensor.float

        def spy_float(t, *a, **k):
            self.widened.append((t.dtype, t.data_ptr()))
            return real(t, *a, **k)
        monkeypatch.setattr(torch.Tensor, "float", spy_float)


def backward_of(t, names, gout, monkeypatch, **options):
    m = leaves(t, names)
    out = blend_module(*[m[n] for n in BLEND_NAMES], **options)
    assert out.dtype == gout.dtype
    spy = LayerSpies(monkeypatch)
    out.backward(gout)
    torch.cuda.synchronize()
    monkeypatch.undo()
    return m, spy


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_layer_takes_the_half_kernel_when_asked(monkeypatch, shape, tname, flow_t):
    _h, t = half_inputs(shape, tname, flow_t, 89)
    _g, gout = half_gout(shape, tname, 9)
    m, spy = backward_of(t, BLEND_NAMES[2:], gout, monkeypatch, fused_half_backward=True)
    assert spy.new.calls == 2 and spy.new.returns == [0, 0], (spy.new.calls, spy.new.returns)
    assert spy.recompute.calls == 0 and spy.lp_grad.calls == 0 and spy.f32_backward.calls == 0 and spy.door.calls == 0
    assert spy.composed.calls == 0
    saved = {m[n].data_ptr() for n in BLEND_NAMES} | {gout.data_ptr()}
    assert not [w for w in spy.widened if w[1] in saved], spy.widened
    assert m["x0"].grad is None and m["x2"].grad is None
    want = promoted_grads(blend_module, t, BLEND_NAMES[2:], BLEND_NAMES, gout.float())
    torch.cuda.synchronize()
    for n in BLEND_NAMES[2:]:
        assert m[n].grad.dtype == t[n].dtype and torch.equal(m[n].grad, want[n]), (n, int((m[n].grad != want[n]).sum()))


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
def test_a_direction_whose_image_wants_a_gradient_is_composed(oracle, monkeypatch, tname, flow_t):
    shape = SHAPES[0]
    h, t = half_inputs(shape, tname, flow_t, 101)
    gout_h, gout = half_gout(shape, tname, 11)
    names = BLEND_NAMES[2:] + ("x0",)
    m, spy = backward_of(t, names, gout, monkeypatch, fused_half_backward=True)
    assert spy.composed.calls == 1 and spy.recompute.calls == 1 and spy.lp_grad.calls == 1      # direction 0, as today
    assert spy.new.calls == 1 and spy.new.returns == [0]                                         # direction 1
    assert m["x2"].grad is None
    want = NC.expected_backward(NC.BLEND, {}, [h[n] for n in BLEND_NAMES], gout_h)
    for k, n in enumerate(BLEND_NAMES):
        if n in names:
            NC.by_dtype(m[n].grad, want[k], t[n].dtype, "half blend, x0 wants a gradient: grad %s" % n,
                        3 * RTOL if n == "x0" else RTOL)
    # direction 1 is the fused kernel's: the fp32 layer's fused route on the widened leaves, cast once
    fused = promoted_grads(blend_module, t, BLEND_NAMES[2:], BLEND_NAMES, gout.float())
    torch.cuda.synchronize()
    for n in ("f1", "k1", "o1"):
        assert torch.equal(m[n].grad, fused[n]), n


@pytest.mark.parametrize("tname", TNAMES)
def test_a_declined_direction_takes_the_composed_route(monkeypatch, tname):
    """the binding answers 1 (not covered, nothing touched): both directions are composed -- the default layer's bits"""
    shape = SHAPES[0]
    _h, t = half_inputs(shape, tname, "fp32", 97)
    _g, gout = half_gout(shape, tname, 10)
    default, _spy = backward_of(t, BLEND_NAMES[2:], gout, monkeypatch)
    asked = []
    monkeypatch.setattr(LPBG(), ENTRY, lambda *a: asked.append(a) or 1)
    m = leaves(t, BLEND_NAMES[2:])
    out = blend_module(*[m[n] for n in BLEND_NAMES], fused_half_backward=True)
    composed = Spy(monkeypatch, BL(), "_direction_backward")
    out.backward(gout)
    torch.cuda.synchronize()
    assert len(asked) == 2 and composed.calls == 2
    for n in BLEND_NAMES[2:]:
        assert m[n].grad.dtype == t[n].dtype and torch.equal(m[n].grad, default[n].grad), n
    assert m["x0"].grad is None and m["x2"].grad is None


def recorded_backward(t, names, gout, **options):
    m = leaves(t, names)
    out = blend_module(*[m[n] for n in BLEND_NAMES], **options)
    with NC.Recorder() as rec:
        out.backward(gout)
        torch.cuda.synchronize()
    return m, [(c.lib, c.entry, c.ret, c.path, c.none_args) for c in rec.lib_calls]


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
def test_switch_off_is_the_layer_without_the_keyword(monkeypatch, tname, flow_t):
    monkeypatch.setattr(NC, "LIBS", NC.LIBS + ("my_lib_lp_blend_grad",))
    shape = SHAPES[0]
    _h, t = half_inputs(shape, tname, flow_t, 103)
    _g, gout = half_gout(shape, tname, 12)
    plain, plain_calls = recorded_backward(t, BLEND_NAMES[2:], gout)
    off, off_calls = recorded_backward(t, BLEND_NAMES[2:], gout, fused_half_backward=False)
    assert off_calls == plain_calls and len(plain_calls) == 4, (off_calls, plain_calls)
    assert not [c for c in off_calls if c[0] == "my_lib_lp_blend_grad"]
    for n in BLEND_NAMES[2:]:
        assert off[n].grad.dtype == t[n].dtype and torch.equal(off[n].grad, plain[n].grad), n
    assert off["x0"].grad is None and off["x2"].grad is None


# --------------------------------------------------------------------------------------------------------------
# 7: the network cast to bf16
# --------------------------------------------------------------------------------------------------------------
def test_bf16_training_step_runs_on_the_half_blend_backward(monkeypatch):
    monkeypatch.setattr(NC, "LIBS", NC.LIBS + ("my_lib_lp_blend_grad",))
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    net = star(True).to(torch.bfloat16)
    assert net.fused_half_blend_backward is False            # off by default
    net.fused_half_blend_backward = True
    x = _netutil.training_frames(5, 1, 128, 128).cuda().to(torch.bfloat16)
    with NC.Recorder() as rec:
        net.zero_grad(set_to_none=True)
        losses, _f, _k, _o = net(x)
        total = sum(l.abs().sum() for l in losses)
        total.backward()
        torch.cuda.synchronize()
    blends = rec.of(NC.BLEND)
    assert len(blends) == 1 and blends[0].options == {"fused_half_backward": True}
    call = blends[0]
    assert all(i.dtype == torch.bfloat16 for i in call.inputs) and call.outputs[0].dtype == torch.bfloat16
    assert [i.requires_grad for i in call.inputs] == [False, False] + [True] * 6
    new = rec.lib("my_lib_lp_blend_grad", ENTRY, backward=True)
    assert len(new) == 2 and all(c.ret == 0 and c.path == PATH for c in new), new
    assert not rec.lib("my_lib_lp_blend_grad", backward=False)
    assert not rec.lib("my_lib", "FilterInterpolationLayer_gpu_forward", backward=True)      # no fp32 recomputation
    assert not rec.lib("my_lib_lp_grad", backward=True)
    assert not [c for c in rec.lib_calls if c.ret != 0], rec.lib_calls
    # every recorded gradient against the fp32 oracle
    checked = 0
    for c in rec.calls:
        if NC.wants_gradients(c):
            NC.check_gradoutput(c)
            checked += len(NC.check_backward(c))
    assert checked >= 6
    # the fused kernel's three gradients per direction: the fp32 layer's fused route on the widened record, cast once
    want = NC.promoted_gradients(call, composed=False)
    for rec_in, w in zip(call.inputs[2:], want[2:]):
        assert rec_in.grad.dtype == torch.bfloat16 and torch.equal(rec_in.grad, w), rec_in.name
    assert call.inputs[0].grad is None and call.inputs[1].grad is None
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g.float()).all()) for g in grads)
