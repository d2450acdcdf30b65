"""Every warp kernel, the context warp, the projection forward and backward and the x4 upsampling on the exact-arithmetic
inputs of tests/_exact.py: bit for bit against the fp32 oracle on the same bytes.

On those inputs every product and every partial sum is a number of fp32 (tests/test_exact_inputs.py proves it on the CPU,
with a float64 build of the oracle and a bound on the sum of absolute terms), so the result is the same bits whatever the
order, the contraction, the packed fixed-point planes or the atomics do -- and the oracle's answer is an exact
expectation.  Rules, for every test:
  * expectation = the fp32 oracle on the same bytes; `torch.equal` on the whole tensor: no tolerance, no allowance for a
    fraction of elements, nothing masked;
  * a result stored in fp16 / bf16 must equal want.to(T); an fp32 image gradient or mixed-precision output is exact in fp32;
  * outputs are pre-filled with NaN (7.0 where the fp32 tests pre-fill what a kernel stores); a gradinput1 that is added
    into starts at 0.5 and must come back as want + 0.5 (a multiple of the quantum as well);
  * last_kernel_path() is asserted for every call that records one (the fp32 blend forward records none).
The projection forward divides: count must be exact, cells with count <= 0 must hold float32(s) -- the raw sum nothing
divided, exactly 0 where nothing landed --, elsewhere |got - s / c| <= 2^-22 |s / c| for the exact sums s and c
(tests/_exact.project_sums, float64 quotient).  The bound is derived: the kernels multiply by v_rcp_f32 (<= 1 ulp) or by
1.0f / c (<= 1/2 ulp) and round once more: <= 3 * 2^-24 relative; 2^-22 leaves a third over that.
With hole filling (fillhole = 1) counts and sums are still exact, so the SIGN of every count is certain -- also under signed
depths k / 8, k = -9 .. 9, whose sums are negative or cancel to exactly zero over a non-zero flow sum -- and which hole is
filled from which cells is decided, not ambiguous: a kept hole holds float32(s) bit for bit, a filled one is within
2^-21 * S of tests/_exact.fill_expectation (oracle/memc_oracle.c project_fillhole in float64) applied to the kernel's own
output and count, bit-equal to its neighbour where only one contributes; the bound is derived at the test.  The cases
reach the owner kernels and their in-tile fill, proj_owner_far (a patch of sources that leave the image pulls the motion
estimate away: such an image is redone there), proj_fill_pending with walks over 12 tile columns and 9 tile rows, the
ragged-row instantiations and the one-lane-per-site kernels with proj_fillhole; last_kernel_path() comes from the CPU
restatement of launch_proj_fwd.  The _ws entry points (workspaces full of 0xFF and 0x01), row-padded and misaligned views
and the two modules are held to the plain entry point's result with `torch.equal`.  What each case reaches is counted in
tests/test_exact_inputs.py::test_projection_fill_census.  The general path and proj_fillhole_v4 (a stream capture without a
workspace only) stay under test_gpu_workspace_and_streams.py.

The projection backward divides as well, by a count that its ABI takes as an INPUT: the cases hand it synthetic counts,
+-2^e where the true scatter puts anything and exactly 0 elsewhere, so that every quotient is exact and the comparison is
`torch.equal` like the warps' (the tiled kernel stages 1 / 0 = inf for the empty cells: a wrong read is inf or NaN).
Which case reaches the uncovered-site branch, a box clipped in x or y, the ragged staging, the tail columns' launch and
the one-lane-per-site route is counted on the CPU (tests/test_exact_inputs.py::test_projection_backward_census).  Real
counts stay under the 1e-4 tests of tests/test_gpu_parity.py, which remain as they are.
The context warp (fi_fwd_ctx_img) records no kernel path: its status is asserted.  The x4 upsampling without
align_corners has dyadic weights and torch's CPU result in float64 as its expectation; with align_corners it has none and
runs the same shapes under the rule of test_gpu_parity.test_flow_upsample4.

What this module cannot see: a difference in rounding order (exact inputs have none).  The bit-equality tests between
the libraries (test_gpu_lowp_paths.py, test_gpu_mx_grad.py) stay for that.  What it sees that they and the 1e-4 rule of
tests/_parity.py do not: any dropped, doubled or misweighted contribution, down to one part in 2^20 and below, on the
paths that only atomics reach as well, and sites exactly on the `<=` / `<` edges of the validity test.
profiles/exact_inputs_observed.md keeps the runs' times, what six 2^-20 mutations did to it, and what five mutations of the
hole filling did.
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

import _exact as E                         # noqa: E402
from tools import synth                    # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
TNAMES = sorted(DTYPES)
FLOWS = ["fp32", "T"]
NAMES = ("x0", "x2", "f0", "f1", "k0", "k1", "o0", "o1")
DIRECTIONS = (("x0", "f0", "k0", "o0"), ("x2", "f1", "k1", "o1"))


def F32():
    import my_package._ext.my_lib as M
    return M


def BG():
    import my_package._ext.my_lib_blend_grad as M
    return M


def LP():
    import my_package._ext.my_lib_lp as M
    return M


def LPG():
    import my_package._ext.my_lib_lp_grad as M
    return M


def MX():
    import my_package._ext.my_lib_mx as M
    return M


def MXG():
    import my_package._ext.my_lib_mx_grad as M
    return M


def D(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)


def filled(shape_of, value, dtype=None):
    return torch.full(shape_of.shape, value, dtype=dtype or shape_of.dtype, device="cuda")


def exact(got, want, what):
    """got (device tensor) == want (fp32 numpy) rounded to got's dtype, every element, bit for bit"""
    w = torch.from_numpy(np.ascontiguousarray(want, dtype=np.float32)).to(got.dtype)
    g = got.detach().cpu()
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not torch.equal(g, w):
        bad = ~((g == w) | (torch.isnan(g) & torch.isnan(w)))
        idx = torch.nonzero(bad)
        first = tuple(int(i) for i in idx[0])
        raise AssertionError("%s: %d of %d elements differ (%d NaN); first at %s: got %r, want %r; max |diff| %g" % (
            what, int(bad.sum()), bad.numel(), int(torch.isnan(g).sum()), first, float(g[first]), float(w[first]),
            float((g.float() - w.float())[bad & ~torch.isnan(g)].abs().max()) if bool((bad & ~torch.isnan(g)).any()) else NAN))


_WANT = {}


def once(key, make):
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


def want_fi(oracle, key, x, flow, filt, gout=None):
    """the oracle's (forward,) or (image, flow, tap gradients) of a case, computed once per session"""
    if gout is None:
        return once(("fwd",) + key, lambda: oracle.filter_interpolation_forward(x, flow, filt))
    return once(("bwd",) + key, lambda: oracle.filter_interpolation_backward(x, flow, filt, gout))


def want_direction(oracle, key, h, d):
    """(image, flow, tap, occlusion) gradients and the warp of direction d of a blend case h"""
    def make():
        x, f, k, o = (h[n] for n in DIRECTIONS[d])
        g1, g2, g3 = oracle.filter_interpolation_backward(x, f, k, (h["gout"] * o).astype(np.float32))
        w = oracle.filter_interpolation_forward(x, f, k)
        return g1, g2, g3, (h["gout"] * w).sum(axis=1, keepdims=True, dtype=np.float32), w
    return once(("dir", d) + key, make)


def want_blend(oracle, key, h):
    return once(("blend",) + key, lambda: (h["o0"] * want_direction(oracle, key, h, 0)[4] +
                                           h["o1"] * want_direction(oracle, key, h, 1)[4]).astype(np.float32))


def fwd_path(C, W, taps=16):
    if taps != 16:
        return "fi_fwd:generic"
    if (W & ~3) < 8 and W % 4 != 0:
        return "fi_fwd:direct"
    return "fi_fwd:tiled_c3" if C == 3 else "fi_fwd:tiled_c4n" if C % 4 == 0 and C >= 8 and W % 4 == 0 else \
        "fi_fwd:tiled_c4n_ragged" if C >= 4 else "fi_fwd:tiled_chunks"


def bwd_path(C, W, taps=16):
    if taps != 16:
        return "fi_bwd:generic"
    if C == 3:
        return "fi_bwd:tiled_c3" if (W & ~3) >= 4 else "fi_bwd:direct"
    return "fi_bwd:owner" if (W & ~3) >= 8 else "fi_bwd:direct"


# ==================================================================================================================
# libmemc_hip.so
# ==================================================================================================================
def f32_forward(oracle, key, x, flow, filt, what):
    C, W = x.shape[1], x.shape[3]
    tx = D(x)
    out = filled(tx, NAN)
    assert F32().FilterInterpolationLayer_gpu_forward(tx, D(flow), D(filt), out) == 0
    assert F32().last_kernel_path() == fwd_path(C, W, filt.shape[1]), what
    exact(out, want_fi(oracle, key, x, flow, filt), what)


def f32_backward(oracle, key, x, flow, filt, gout, what, image=True):
    """the C entry point from pre-filled buffers.  gradinput1 is ADDED into by the RGB tiled kernel (0.5 -> want + 0.5), STORED
    by the owner kernels (7.0, as test_filter_interpolation_backward_many_channels); the one-lane-per-site kernels get zeros"""
    C, W = x.shape[1], x.shape[3]
    path = bwd_path(C, W, filt.shape[1])
    fill = {"fi_bwd:tiled_c3": 0.5, "fi_bwd:owner": 7.0}.get(path, 0.0)
    tx, tf, tk = D(x), D(flow), D(filt)
    g1 = filled(tx, fill) if image else None
    g2, g3 = filled(tf, NAN), filled(tk, NAN)
    assert F32().FilterInterpolationLayer_gpu_backward(tx, tf, tk, D(gout), g1, g2, g3) == 0
    assert F32().last_kernel_path() == path, what
    w1, w2, w3 = want_fi(oracle, key, x, flow, filt, gout)
    if image:
        exact(g1, w1 + np.float32(fill if path == "fi_bwd:tiled_c3" else 0.0), what + " image gradient")
    exact(g2, w2, what + " flow gradient")
    exact(g3, w3, what + " tap gradient")


@pytest.mark.parametrize("ci", range(len(E.TABLE)), ids=E.TABLE_IDS)
def test_fp32_forward_on_the_table(oracle, ci):
    for C in E.FWD_CHANNELS[ci]:
        x, flow, filt, _ = E.table_inputs(E.TABLE[ci], C)
        f32_forward(oracle, ("table", ci, C, "fp32"), x, flow, filt, "fp32 forward %s C%d" % (E.TABLE_IDS[ci], C))


@pytest.mark.parametrize("name", sorted(E.SHAPES))
def test_fp32_forward_and_backward_on_other_shapes(oracle, name):
    """ragged widths (the tiled kernel on the whole quads, one lane per site behind them), the minimum width, the generic
    kernels of other filter sizes"""
    x, flow, filt, gout = E.shaped_inputs(*E.SHAPES[name])
    f32_forward(oracle, ("shape", name), x, flow, filt, "fp32 forward " + name)
    f32_backward(oracle, ("shape", name), x, flow, filt, gout, "fp32 backward " + name)


@pytest.mark.parametrize("image", [True, False], ids=["image", "noimage"])
@pytest.mark.parametrize("ci", range(len(E.TABLE)), ids=E.TABLE_IDS)
def test_fp32_rgb_backward_on_the_table(oracle, ci, image):
    x, flow, filt, gout = E.table_inputs(E.TABLE[ci], 3)
    f32_backward(oracle, ("table", ci, 3, "fp32"), x, flow, filt, gout, "fp32 backward %s" % E.TABLE_IDS[ci], image)


MANY = E.many_rows()
MANY_IDS = ["%dx%dx%dx%d-%s" % r for r in MANY]


@pytest.mark.parametrize("row", MANY, ids=MANY_IDS)
def test_fp32_many_channel_backward(oracle, row):
    x, flow, filt, gout = E.many_inputs(row)
    f32_forward(oracle, ("many", row), x, flow, filt, "fp32 forward %s" % (row,))
    f32_backward(oracle, ("many", row), x, flow, filt, gout, "fp32 backward %s" % (row,))


def bilinear(oracle, key, x, flow, gout, what, three_only=False):
    """InterpolationCh (and Interpolation, RGB only) forward and backward"""
    C, W = x.shape[1], x.shape[3]
    tx, tf, tg = D(x), D(flow), D(gout)
    ops = [("InterpolationChLayer", oracle.interpolation_ch_forward, oracle.interpolation_ch_backward)]
    if three_only:
        ops.append(("InterpolationLayer", oracle.interpolation_forward, oracle.interpolation_backward))
    owner = C != 3 and (W & ~3) >= 8
    for name, fwd, bwd in ops:
        out = filled(tx, NAN)
        assert getattr(F32(), name + "_gpu_forward")(tx, tf, out) == 0
        assert F32().last_kernel_path() == ("bl_fwd:tiled_c3" if C == 3 else "bl_fwd:tiled_chunks"), what
        exact(out, once((name, "fwd") + key, lambda: fwd(x, flow)), "%s %s forward" % (what, name))
        # gradinput1: added into by the RGB kernels, stored by the owner kernels; gradinput2 is stored
        fill = 0.5 if C == 3 else 7.0 if owner else 0.0
        g1, g2 = filled(tx, fill), filled(tf, 7.0)
        assert getattr(F32(), name + "_gpu_backward")(tx, tf, tg, g1, g2) == 0
        assert F32().last_kernel_path() == ("bl_bwd:tiled_c3" if C == 3 else "bl_bwd:owner" if owner else "bl_bwd:direct"), what
        w1, w2 = once((name, "bwd") + key, lambda: bwd(x, flow, gout))
        exact(g1, w1 + np.float32(0.5 if C == 3 else 0.0), "%s %s image gradient" % (what, name))
        exact(g2, w2, "%s %s flow gradient" % (what, name))


def test_fp32_bilinear_rgb(oracle):
    for name, x, flow, gout in E.bilinear_rgb_cases():
        bilinear(oracle, ("rgb", name), x, flow, gout, "bilinear " + name, three_only=True)


@pytest.mark.parametrize("row", MANY, ids=MANY_IDS)
def test_fp32_bilinear_many_channels(oracle, row):
    x, flow, _filt, gout = E.many_inputs(row)
    bilinear(oracle, ("many", row), x, flow, gout, "bilinear %s" % (row,))


PARITY_BLEND = E.parity_blend_cases()


@pytest.mark.parametrize("case", PARITY_BLEND, ids=["%dx%dx%dx%d-%s" % c[:5] for c in PARITY_BLEND])
def test_fp32_blend_forward(oracle, case):
    """the fused kernel through the C entry point where it takes the shape (RGB, W % 4 == 0), and the layer for every case
    (the last two compose the blend from two warps: two exact products and one exact sum as well)"""
    from my_package.modules.FilterInterpolationBlendModule import FilterInterpolationBlendModule
    h = E.parity_blend_inputs(case)
    want = want_blend(oracle, ("pblend", case), h)
    t = {n: D(h[n]) for n in NAMES}
    if case[1] == 3 and case[3] % 4 == 0:
        out = filled(t["x0"], NAN)
        assert F32().FilterInterpolationBlendLayer_gpu_forward(*[t[n] for n in NAMES], out) == 0
        exact(out, want, "fp32 blend, C entry point")
    with torch.no_grad():
        exact(FilterInterpolationBlendModule()(*[t[n] for n in NAMES]), want, "fp32 blend, layer")


# ==================================================================================================================
# libmemc_hip_blend_grad.so
# ==================================================================================================================
def blend_grad_call(t, d, outs=None):
    x, f, k, o = (t[n] for n in DIRECTIONS[d])
    g2, g3, g4 = outs if outs is not None else (filled(f, NAN), filled(k, NAN), filled(o, NAN))
    assert BG().FilterInterpolationBlendLayer_gpu_backward(x, f, k, o, t["gout"], g2, g3, g4) == 0
    assert BG().last_kernel_path() == "fi_blend_bwd:tiled_c3"
    return g2, g3, g4


@pytest.mark.parametrize("ci", range(len(E.TABLE)), ids=E.TABLE_IDS)
def test_blend_backward_fused(oracle, ci):
    """flow, tap and occlusion gradient of both directions; the occlusion gradient at invalid sites is
    sum_c gradoutput_c * input_c, exact as well"""
    h = E.blend_inputs(E.TABLE[ci])
    t = {n: D(h[n]) for n in NAMES + ("gout",)}
    for d in (0, 1):
        g2, g3, g4 = blend_grad_call(t, d)
        _w1, w2, w3, w4, _w = want_direction(oracle, ("table", ci, "fp32"), h, d)
        what = "fused blend backward %s direction %d" % (E.TABLE_IDS[ci], d)
        exact(g2, w2, what + " flow gradient")
        exact(g3, w3, what + " tap gradient")
        exact(g4, w4, what + " occlusion gradient")


# ==================================================================================================================
# libmemc_hip_lp.so / libmemc_hip_lp_grad.so and libmemc_hip_mx.so / libmemc_hip_mx_grad.so
# ==================================================================================================================
def storage(tname, flow_t):
    return tname if flow_t == "T" else "fp32"


def lowp_cases(flow_t):
    """table cases a flow storage runs: 1x20x1280-far keeps its paths only unclipped, in fp32"""
    return [ci for ci, c in enumerate(E.TABLE) if flow_t == "fp32" or c != E.FAR]


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("lib", ["lp", "mx"])
def test_lowp_forward(oracle, lib, tname, flow_t):
    T = DTYPES[tname]
    FT = T if flow_t == "T" else torch.float32
    st = storage(tname, flow_t)
    for ci in lowp_cases(flow_t):
        for C in (E.FWD_CHANNELS[ci] if lib == "lp" else [3]):
            x, flow, filt, _ = E.table_inputs(E.TABLE[ci], C, st)
            what = "%s forward %s C%d %s flow %s" % (lib, E.TABLE_IDS[ci], C, tname, flow_t)
            want = want_fi(oracle, ("table", ci, C, st), x, flow, filt)
            if lib == "lp":
                tx = D(x, T)
                out = filled(tx, NAN)
                assert LP().FilterInterpolationLayer_gpu_forward_lp(tx, D(flow, FT), D(filt, T), out) == 0
                assert LP().last_kernel_path() == ("fi_fwd_lp:tiled_c3" if C == 3 else "fi_fwd_lp:tiled_c4n"), what
                assert out.dtype == T
            else:
                tx = D(x)
                out = filled(tx, NAN)
                assert MX().FilterInterpolationLayer_gpu_forward_mx(tx, D(flow, FT), D(filt, T), out) == 0
                assert MX().last_kernel_path() == "fi_fwd_mx:tiled_c3", what
                assert out.dtype == torch.float32
            exact(out, want, what)


def lowp_blend_tensors(h, lib, T, FT):
    img = T if lib == "lp" else torch.float32
    return {n: D(h[n], img if n[0] == "x" else FT if n[0] == "f" else T) for n in NAMES}


def lowp_blend_call(lib, t, out):
    if lib == "lp":
        assert LP().FilterInterpolationBlendLayer_gpu_forward_lp(*[t[n] for n in NAMES], out) == 0
        assert LP().last_kernel_path() == "fi_blend_lp:tiled_c3"
    else:
        assert MX().FilterInterpolationBlendLayer_gpu_forward_mx(*[t[n] for n in NAMES], out) == 0
        assert MX().last_kernel_path() == "fi_blend_mx:tiled_c3"
    return out


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("lib", ["lp", "mx"])
def test_lowp_blend(oracle, lib, tname, flow_t):
    T = DTYPES[tname]
    FT = T if flow_t == "T" else torch.float32
    st = storage(tname, flow_t)
    for ci in lowp_cases(flow_t):
        h = E.blend_inputs(E.TABLE[ci], st)
        t = lowp_blend_tensors(h, lib, T, FT)
        out = lowp_blend_call(lib, t, filled(t["x0"], NAN))
        exact(out, want_blend(oracle, ("table", ci, st), h), "%s blend %s %s flow %s" % (lib, E.TABLE_IDS[ci], tname, flow_t))


def lowp_backward_call(lib, x, flow, filt, gout, g1, g2=None, g3=None):
    g2 = filled(flow, NAN) if g2 is None else g2
    g3 = filled(filt, NAN) if g3 is None else g3
    if lib == "lp":
        assert LPG().FilterInterpolationLayer_gpu_backward_lp(x, flow, filt, gout, g1, g2, g3) == 0
        assert LPG().last_kernel_path() == ("fi_bwd_lp:tiled_c3" if g1 is not None else "fi_bwd_lp:tiled_c3_noimage")
    else:
        assert MXG().FilterInterpolationLayer_gpu_backward_mx(x, flow, filt, gout, g1, g2, g3) == 0
        assert MXG().last_kernel_path() == ("fi_bwd_mx:tiled_c3" if g1 is not None else "fi_bwd_mx:tiled_c3_noimage")
    torch.cuda.synchronize()
    return g1, g2, g3


def lowp_backward_tensors(lib, case, T, FT, st):
    """half library: image and taps in T, the gradoutput in the flow's storage; mixed: fp32 image and gradoutput, taps in T"""
    x, flow, filt, gout = E.table_inputs(case, 3, st)
    if lib == "lp":
        return D(x, T), D(flow, FT), D(filt, T), D(gout, FT)
    return D(x), D(flow, FT), D(filt, T), D(gout)


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", FLOWS)
@pytest.mark.parametrize("image", [True, False], ids=["image", "noimage"])
@pytest.mark.parametrize("lib", ["lp", "mx"])
def test_lowp_backward(oracle, lib, tname, flow_t, image):
    """the fp32 gradinput1 (added into: 0.5 -> want + 0.5) is exact at fp32 resolution; the flow gradient comes back in the
    flow's storage and the tap gradient in T, each the oracle's rounded once"""
    T = DTYPES[tname]
    FT = T if flow_t == "T" else torch.float32
    st = storage(tname, flow_t)
    for ci in lowp_cases(flow_t):
        x, flow, filt, gout = lowp_backward_tensors(lib, E.TABLE[ci], T, FT, st)
        g1 = torch.full(x.shape, 0.5, dtype=torch.float32, device="cuda") if image else None
        g1, g2, g3 = lowp_backward_call(lib, x, flow, filt, gout, g1)
        w1, w2, w3 = want_fi(oracle, ("table", ci, 3, st), *E.table_inputs(E.TABLE[ci], 3, st))
        what = "%s backward %s %s flow %s" % (lib, E.TABLE_IDS[ci], tname, flow_t)
        assert g2.dtype == FT and g3.dtype == T
        exact(g2, w2, what + " flow gradient")
        exact(g3, w3, what + " tap gradient")
        if image:
            assert g1.dtype == torch.float32
            exact(g1, w1 + np.float32(0.5), what + " image gradient")


# ==================================================================================================================
# per library: row-padded views and a second identical call, on table case 1
# ==================================================================================================================
PAD_CI = 1


def pad(t):
    p = synth.padded_planes(t)
    assert not p.is_contiguous() and p.stride(2) == t.shape[3] + 64
    return p


def test_fp32_padded_views_and_run_to_run(oracle):
    x, flow, filt, gout = E.table_inputs(E.TABLE[PAD_CI], 3)
    w1, w2, w3 = want_fi(oracle, ("table", PAD_CI, 3, "fp32"), x, flow, filt, gout)
    want = want_fi(oracle, ("table", PAD_CI, 3, "fp32"), x, flow, filt)
    dense = [D(a) for a in (x, flow, filt, gout)]
    for rnd, (tx, tf, tk, tg) in enumerate((dense, dense, [pad(t) for t in dense])):
        mk = (lambda t, v: pad(filled(t, v))) if rnd == 2 else filled
        out, g1, g2, g3 = mk(dense[0], NAN), mk(dense[0], 0.5), mk(dense[1], NAN), mk(dense[2], NAN)
        assert F32().FilterInterpolationLayer_gpu_forward(tx, tf, tk, out) == 0
        assert F32().last_kernel_path() == "fi_fwd:tiled_c3"
        assert F32().FilterInterpolationLayer_gpu_backward(tx, tf, tk, tg, g1, g2, g3) == 0
        assert F32().last_kernel_path() == "fi_bwd:tiled_c3"
        what = "fp32 library, round %d (2: row-padded views)" % rnd
        exact(out, want, what + " forward")
        exact(g1, w1 + np.float32(0.5), what + " image gradient")
        exact(g2, w2, what + " flow gradient")
        exact(g3, w3, what + " tap gradient")
    # the blend forward on the same views
    h = E.blend_inputs(E.TABLE[PAD_CI])
    t = {n: D(h[n]) for n in NAMES}
    for rnd, tt in enumerate((t, t, {n: pad(v) for n, v in t.items()})):
        out = pad(filled(t["x0"], NAN)) if rnd == 2 else filled(t["x0"], NAN)
        assert F32().FilterInterpolationBlendLayer_gpu_forward(*[tt[n] for n in NAMES], out) == 0
        exact(out, want_blend(oracle, ("table", PAD_CI, "fp32"), h), "fp32 blend forward, round %d" % rnd)


def test_blend_grad_padded_views_and_run_to_run(oracle):
    h = E.blend_inputs(E.TABLE[PAD_CI])
    t = {n: D(h[n]) for n in NAMES + ("gout",)}
    _w1, w2, w3, w4, _w = want_direction(oracle, ("table", PAD_CI, "fp32"), h, 0)
    for rnd, tt in enumerate((t, t, {n: pad(v) for n, v in t.items()})):
        outs = tuple(pad(filled(t[n], NAN)) for n in ("f0", "k0", "o0")) if rnd == 2 else None
        g2, g3, g4 = blend_grad_call(tt, 0, outs)
        exact(g2, w2, "fused blend backward, round %d, flow gradient" % rnd)
        exact(g3, w3, "fused blend backward, round %d, tap gradient" % rnd)
        exact(g4, w4, "fused blend backward, round %d, occlusion gradient" % rnd)


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("lib", ["lp", "mx"])
def test_lowp_padded_views_and_run_to_run(oracle, lib, tname):
    T = DTYPES[tname]
    st = tname
    case = E.TABLE[PAD_CI]
    h = E.blend_inputs(case, st)
    want_b = want_blend(oracle, ("table", PAD_CI, st), h)
    t = lowp_blend_tensors(h, lib, T, T)
    dense = lowp_backward_tensors(lib, case, T, T, st)
    w1, w2, w3 = want_fi(oracle, ("table", PAD_CI, 3, st), *E.table_inputs(case, 3, st))
    for rnd in range(3):
        mk = (lambda t_, v, dt=None: pad(filled(t_, v, dt))) if rnd == 2 else filled
        tt = {n: pad(v) for n, v in t.items()} if rnd == 2 else t
        out = lowp_blend_call(lib, tt, mk(t["x0"], NAN))
        exact(out, want_b, "%s blend %s, round %d (2: row-padded views)" % (lib, tname, rnd))
        x, flow, filt, gout = [pad(v) for v in dense] if rnd == 2 else dense
        g1, g2, g3 = lowp_backward_call(lib, x, flow, filt, gout, mk(dense[0], 0.5, torch.float32), mk(dense[1], NAN), mk(dense[2], NAN))
        what = "%s backward %s, round %d (2: row-padded views)" % (lib, tname, rnd)
        exact(g1, w1 + np.float32(0.5), what + " image gradient")
        exact(g2, w2, what + " flow gradient")
        exact(g3, w3, what + " tap gradient")


# ==================================================================================================================
# the layers, one backward per route on 2x3x40x64
# ==================================================================================================================
# route: (image dtype, payload dtype, flow storage, leaves that need a gradient)
ROUTES = {
    "fp32-fused": ("fp32", "fp32", "fp32", ()),
    "fp32-one-frame-gradient": ("fp32", "fp32", "fp32", ("x0",)),
    "half-composition-fp16": ("fp16", "fp16", "fp16", ("x0", "x2")),
    "half-composition-bf16": ("bf16", "bf16", "fp32", ("x0", "x2")),
    "mixed-frames-are-data-fp16": ("fp32", "fp16", "fp32", ()),
    "mixed-frames-are-data-bf16": ("fp32", "bf16", "bf16", ()),
    "mixed-frame-gradient-fp16": ("fp32", "fp16", "fp16", ("x0",)),
    "mixed-frame-gradient-bf16": ("fp32", "bf16", "fp32", ("x0", "x2")),
}
_TORCH = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_layers_backward(oracle, route):
    from my_package.modules.FilterInterpolationBlendModule import FilterInterpolationBlendModule
    from my_package.modules.FilterInterpolationModule import FilterInterpolationModule
    img, pay, st, frames = ROUTES[route]
    h = E.blend_inputs(E.LAYER_CASE, st)
    key = ("layer", st)

    def leaves():
        dt = {n: _TORCH[img] if n[0] == "x" else _TORCH[st] if n[0] == "f" else _TORCH[pay] for n in NAMES}
        return {n: D(h[n], dt[n]).requires_grad_(n[0] != "x" or n in frames) for n in NAMES}
    # the blend
    t = leaves()
    out = FilterInterpolationBlendModule()(*[t[n] for n in NAMES])
    assert out.dtype == _TORCH[img]
    exact(out, want_blend(oracle, key, h), route + ": blend forward")
    out.backward(D(h["gout"], out.dtype))
    torch.cuda.synchronize()
    for d in (0, 1):
        x, f, k, o = DIRECTIONS[d]
        w1, w2, w3, w4, _w = want_direction(oracle, key, h, d)
        if x in frames:
            assert t[x].grad.dtype == t[x].dtype
            exact(t[x].grad, w1, "%s: blend grad %s" % (route, x))
        else:
            assert t[x].grad is None
        for n, w in ((f, w2), (k, w3), (o, w4)):
            assert t[n].grad.dtype == t[n].dtype
            exact(t[n].grad, w, "%s: blend grad %s" % (route, n))
    # the warp of direction 0
    t = leaves()
    out = FilterInterpolationModule()(t["x0"], t["f0"], t["k0"])
    assert out.dtype == _TORCH[img]
    exact(out, want_fi(oracle, key + ("warp",), h["x0"], h["f0"], h["k0"]), route + ": warp forward")
    out.backward(D(h["gout"], out.dtype))
    torch.cuda.synchronize()
    w1, w2, w3 = want_fi(oracle, key + ("warp",), h["x0"], h["f0"], h["k0"], h["gout"])
    if "x0" in frames:
        exact(t["x0"].grad, w1, route + ": warp grad x0")
    else:
        assert t["x0"].grad is None
    exact(t["f0"].grad, w2, route + ": warp grad f0")
    exact(t["k0"].grad, w3, route + ": warp grad k0")


# ==================================================================================================================
# FlowProjection / DepthFlowProjection forward
# ==================================================================================================================
OP_NAMES = {"flow": "FlowProjection", "depth": "DepthFlowProjection", "signed": "DepthFlowProjection, signed depths"}


def proj_ops(name):
    return [op for n, op in E.PROJECTION_OPS if n == name]


def proj_path(W, with_depth):
    """what last_kernel_path() must say, from the CPU restatement of launch_proj_fwd (test_exact_inputs.py holds it to the source)"""
    return "%s:%s" % ("dproj_fwd" if with_depth else "proj_fwd", E.LP.proj_fwd_route(W)[0])


def proj_call(tf, td, fill, cnt, out, ws=None):
    """the C entry point (with a workspace: the _ws one); asserts status and kernel path"""
    args = (tf, cnt, out, fill) if td is None else (tf, td, cnt, out, fill)
    name = ("FlowProjectionLayer" if td is None else "DepthFlowProjectionLayer") + "_gpu_forward" + ("" if ws is None else "_ws")
    assert getattr(F32(), name)(*(args if ws is None else args + (ws,))) == 0, name
    assert F32().last_kernel_path() == proj_path(tf.shape[3], td is not None), name
    return cnt, out


def sevens(B, C, H, W):
    return torch.full((B, C, H, W), 7.0, device="cuda")


def proj_want(oracle, name, op):
    """(s, c, float32(s), the oracle's count): the exact sums of tests/_exact.project_sums, once per session"""
    def make():
        flow, d = E.projection_operator(name, op)
        s, c = E.project_sums(flow, d)
        want_cnt = (oracle.flow_projection_forward(flow, 0) if d is None else oracle.depth_flow_projection_forward(flow, d, 0))[1]
        assert np.array_equal(want_cnt, c)
        return s, c, s.astype(np.float32), want_cnt
    return once(("proj", name, op), make)


def proj_plain(name, op, fill):
    """(count, output) of the plain C entry point from 7.0-filled dense buffers, once per session; never written again"""
    def make():
        flow, d = E.projection_operator(name, op)
        B, _, H, W = flow.shape
        cnt, out = proj_call(D(flow), None if d is None else D(d), fill, sevens(B, 1, H, W), sevens(B, 2, H, W))
        torch.cuda.synchronize()
        return cnt, out
    return once(("proj-plain", name, op, fill), make)


def check_divided(got, s, c, what):
    """cells with count > 0: |got - s / c| <= 2^-22 |s / c| (derived in this module's header)"""
    hit = np.broadcast_to(c > 0, s.shape)
    q = s[hit] / np.broadcast_to(c, s.shape)[hit]
    err = np.abs(got.astype(np.float64)[hit] - q)
    rel = float((err / np.maximum(np.abs(q), 1e-300)).max()) if q.size else 0.0
    print("%s: worst relative error of a quotient %.3g * 2^-24 over %d cells" % (what, rel * 2.0 ** 24, q.size))
    assert bool((err <= 2.0 ** -22 * np.abs(q)).all()), (what, rel)


@pytest.mark.parametrize("name", E.PROJECTION_ALL)
def test_projection_forward(oracle, name):
    """fillhole = 0: the count exact, a cell with count <= 0 holds float32(s) -- the raw sum nothing divided, 0 where nothing
    landed --, elsewhere the 2^-22 rule against s / c"""
    for op in proj_ops(name):
        s, c, s32, want_cnt = proj_want(oracle, name, op)
        cnt, out = proj_plain(name, op, 0)
        what = "%s %s" % (OP_NAMES[op], name)
        exact(cnt, want_cnt, what + " count")
        got = out.cpu().numpy()
        low = np.broadcast_to(c <= 0, s.shape)
        assert np.array_equal(got[low], s32[low]), what + ": a cell with count <= 0 must hold the raw sum (0 where nothing lands)"
        check_divided(got, s, c, what)


@pytest.mark.parametrize("name,op", E.PROJECTION_OPS, ids=E.PROJECTION_OP_IDS)
def test_projection_forward_with_hole_filling(oracle, name, op):
    """fillhole = 1 through the C entry point, from buffers pre-filled with 7.0.  The count and the cells with count > 0 as
    without hole filling; a kept hole holds float32(s).  A filled hole is held to tests/_exact.fill_expectation applied to
    the kernel's OWN output and count -- the expectation takes the kernel's quotients as they are (the cells it reads have
    count > 0: the fill does not write them), what is tested is the walk and the mix:
        |got - v| <= 2^-21 * S,   v = (fl vl + fr vr + fu vu) / n,   S = (fl |vl| + fr |vr| + fu |vu|) / n.
    Derived: at most two additions, each rounding at <= 2^-24 of a partial sum <= n S, and a division or a reciprocal and a
    multiply at <= 3 * 2^-24 more: 5 * 2^-24 * S; 2^-21 is the next power of two.  Where n = 1 the result is the
    neighbour's value itself.  Which walks leave their tile, cross how many tiles or find nothing, and what signed depths
    add: tests/test_exact_inputs.py::test_projection_fill_census; a walk one cell off moves most of the filled holes by more
    than four times the bound: ::test_projection_fill_sensitivity."""
    s, c, s32, want_cnt = proj_want(oracle, name, op)
    cnt, out = proj_plain(name, op, 1)
    what = "%s %s, hole filling" % (OP_NAMES[op], name)
    exact(cnt, want_cnt, what + " count")
    got = out.cpu().numpy()
    check_divided(got, s, c, what)
    v, S, n, filled, kept = E.fill_expectation(got, want_cnt)
    f2, k2 = np.broadcast_to(filled, v.shape), np.broadcast_to(kept, v.shape)
    assert np.array_equal(got[k2], s32[k2]), "%s: %d kept holes do not hold the raw sum" % (what, int((got[k2] != s32[k2]).sum()))
    err = np.abs(got.astype(np.float64) - v)
    worst = float((err[f2] / np.maximum(S[f2], 1e-300)).max()) * 2.0 ** 24 if f2.any() else 0.0
    bad = f2 & ~(err <= E.FILL_BOUND * S)
    print("%s: filled holes within %.3g * 2^-24 * S (%d filled, %d kept)" % (what, worst, int(filled.sum()), int(kept.sum())))
    assert not bad.any(), "%s: %d of %d filled values are off (worst %.3g * 2^-24 * S); first at %s: got %r, want %r" % (
        what, int(bad.sum()), int(f2.sum()), worst, tuple(int(i) for i in np.argwhere(bad)[0]), float(got[bad][0]), float(v[bad][0]))
    one = np.broadcast_to(filled & (n == 1), v.shape)
    assert np.array_equal(got[one].astype(np.float64), v[one]), what + ": one positive neighbour: its value, bit for bit"


@pytest.mark.parametrize("name", E.PROJECTION_ALL)
def test_projection_forward_workspace_entry_points(name):
    """the _ws entry points on a workspace full of 0xFF and of 0x01 bytes: count and output are the plain entry point's bit
    for bit (on these inputs no order of the sums can move a bit); where the route is the one-lane-per-site kernels, which
    use no workspace, the call still returns 0 and gives the same"""
    for op in proj_ops(name):
        flow, d = E.projection_operator(name, op)
        B, _, H, W = flow.shape
        tf, td = D(flow), None if d is None else D(d)
        want_cnt, want_out = proj_plain(name, op, 1)
        nbytes = F32().flow_projection_workspace_bytes(W, H, B, 1, d is not None)
        assert nbytes > 0 and nbytes % 256 == 0
        for garbage in (0xFF, 0x01):
            ws = torch.full((nbytes,), garbage, dtype=torch.uint8, device="cuda")
            cnt, out = proj_call(tf, td, 1, sevens(B, 1, H, W), sevens(B, 2, H, W), ws)
            what = "%s %s, workspace of 0x%02X" % (OP_NAMES[op], name, garbage)
            assert torch.equal(cnt, want_cnt), what + ": count"
            assert torch.equal(out, want_out), what + ": output"


def offset_by_one(t, value=None):
    """t's values (or `value`) one element into a 7.0-filled buffer of their own: same data, no 16-byte alignment: (view, buffer)"""
    buf = torch.full((t.numel() + 1,), 7.0, device="cuda")
    view = buf[1:].view(t.shape)
    if value is None:
        view.copy_(t)
    else:
        view.fill_(value)
    assert view.data_ptr() % 16 == 4
    return view, buf


@pytest.mark.parametrize("name", ["2x70x134-patch-empty", "row5"])
def test_projection_forward_views(name):
    """fillhole = 1 on row-padded views (row stride W + 64, every tensor in a 7.0-filled buffer of its own), twice, and on
    views that start one element into their buffers: the dense call's count and output bit for bit, nothing written behind
    a row or before the first element, the inputs unchanged.  (vec4_ok is the width alone: a misaligned view of a width of
    whole quads stays on the whole-quad owner kernels, whose quad accesses are unaligned ones.)"""
    for op in ("flow", "depth"):
        flow, d = E.projection_operator(name, op)
        B, _, H, W = flow.shape
        want_cnt, want_out = proj_plain(name, op, 1)
        dense = [D(flow)] + ([] if d is None else [D(d)])
        for kind, mk in (("row-padded", padded7), ("row-padded, second call", padded7), ("offset by one element", offset_by_one)):
            ins = [mk(a) for a in dense]
            outs = [mk(sevens(B, 1, H, W), 7.0), mk(sevens(B, 2, H, W), 7.0)]
            proj_call(ins[0][0], None if d is None else ins[1][0], 1, outs[0][0], outs[1][0])
            torch.cuda.synchronize()
            what = "%s %s, %s" % (OP_NAMES[op], name, kind)
            assert torch.equal(outs[0][0], want_cnt), what + ": count"
            assert torch.equal(outs[1][0], want_out), what + ": output"
            for view, buf in ins + outs:
                if mk is padded7:
                    assert bool((buf[:, :, :, W:] == 7.0).all()), what + ": the bytes behind a row were written"
                else:
                    assert float(buf[0]) == 7.0, what + ": the element before a view was written"
            for (view, _buf), a in zip(ins, dense):
                assert torch.equal(view, a), what + ": an input changed"


@pytest.mark.parametrize("name", ["2x70x134-patch-empty", "row5"])
def test_projection_modules(name):
    """FlowProjectionModule / DepthFlowProjectionModule: requires_grad = False fills the holes (the C entry point's
    fillhole = 1 result, bit for bit), requires_grad = True does not (its fillhole = 0 result)"""
    from my_package.modules.DepthFlowProjectionModule import DepthFlowProjectionModule
    from my_package.modules.FlowProjectionModule import FlowProjectionModule
    for op, module in (("flow", FlowProjectionModule), ("depth", DepthFlowProjectionModule)):
        flow, d = E.projection_operator(name, op)
        args = [D(flow)] + ([] if d is None else [D(d)])
        with torch.no_grad():
            got = module(requires_grad=False)(*args)
        assert torch.equal(got, proj_plain(name, op, 1)[1]), "%s %s: requires_grad = False" % (module.__name__, name)
        got = module(requires_grad=True)(*args)
        assert torch.equal(got, proj_plain(name, op, 0)[1]), "%s %s: requires_grad = True" % (module.__name__, name)


# ==================================================================================================================
# FlowProjection / DepthFlowProjection backward on synthetic power-of-two counts: every quotient is exact
# ==================================================================================================================
def want_proj_bwd(oracle, name, with_depth):
    def make():
        h = E.proj_bwd_inputs(name, with_depth)
        if with_depth:
            return oracle.depth_flow_projection_backward(h["flow"], h["depth"], h["count"], h["fwd_out"], h["gout"])
        return (oracle.flow_projection_backward(h["flow"], h["count"], h["gout"]),)
    return once(("pb", name, with_depth), make)


def proj_bwd_call(t, with_depth, outs):
    """the C entry point from pre-filled gradient buffers (every site stores); asserts status and kernel family"""
    path = "%s:%s" % ("dproj_bwd" if with_depth else "proj_bwd", "scalar" if t["scalar"] else "tiled")
    if with_depth:
        assert F32().DepthFlowProjectionLayer_gpu_backward(t["flow"], t["depth"], t["count"], t["fwd_out"], t["gout"], *outs) == 0
    else:
        assert F32().FlowProjectionLayer_gpu_backward(t["flow"], t["count"], t["gout"], outs[0]) == 0
    assert F32().last_kernel_path() == path
    return outs


def proj_bwd_tensors(name, with_depth):
    h = E.proj_bwd_inputs(name, with_depth)
    t = {n: D(h[n]) for n in ("flow", "count", "gout") + (("depth", "fwd_out") if with_depth else ())}
    t["scalar"] = name in E.PB_SCALAR
    return t


@pytest.mark.parametrize("with_depth", [False, True], ids=["flow", "depth"])
@pytest.mark.parametrize("name", E.PB_IDS)
def test_projection_backward(oracle, name, with_depth):
    """which in-kernel branches a case reaches (covered and uncovered sites, boxes clipped in x and y, ragged staging, the
    tail columns' launch): tests/test_exact_inputs.py::test_projection_backward_census"""
    t = proj_bwd_tensors(name, with_depth)
    outs = [filled(t["flow"], NAN)] + ([filled(t["depth"], NAN)] if with_depth else [])
    proj_bwd_call(t, with_depth, outs)
    what = "%s backward %s" % ("DepthFlowProjection" if with_depth else "FlowProjection", name)
    for got, want, n in zip(outs, want_proj_bwd(oracle, name, with_depth), ("gradinput1", "gradinput2")):
        exact(got, want, "%s %s" % (what, n))


def padded7(t, value=None):
    """t's values (or `value`) in rows 64 floats longer, in a buffer of their own filled with 7.0: (view, buffer)"""
    B, C, H, W = t.shape
    buf = torch.full((B, C, H, W + 64), 7.0, device="cuda")
    view = buf[:, :, :, :W]
    if value is None:
        view.copy_(t)
    else:
        view.fill_(value)
    assert not view.is_contiguous() and view.stride(2) == W + 64
    return view, buf


@pytest.mark.parametrize("name", ["2x100x132-smooth8", "2x33x131-iid12"], ids=["whole-quads", "ragged"])
def test_projection_backward_padded_views_and_run_to_run(oracle, name):
    """flow, depth, count, the forward's output, gradoutput and the gradients each in a padded buffer of its own (row
    stride W + 64): the results are the dense ones, twice, and the bytes behind every row of every buffer keep the sentinel"""
    for with_depth in (False, True):
        h = E.proj_bwd_inputs(name, with_depth)
        W = h["flow"].shape[3]
        names = ("flow", "count", "gout") + (("depth", "fwd_out") if with_depth else ())
        views = {n: padded7(D(h[n])) for n in names}
        t = {n: v for n, (v, _buf) in views.items()}
        t["scalar"] = name in E.PB_SCALAR
        want = want_proj_bwd(oracle, name, with_depth)
        runs = []
        for rnd in range(2):
            grads = [padded7(t["flow"], NAN)] + ([padded7(t["depth"], NAN)] if with_depth else [])
            proj_bwd_call(t, with_depth, [g for g, _buf in grads])
            torch.cuda.synchronize()
            what = "%s, %s, round %d, padded views" % (name, "depth" if with_depth else "flow", rnd)
            for (g, _buf), w, n in zip(grads, want, ("gradinput1", "gradinput2")):
                exact(g, w, "%s: %s" % (what, n))
            for n, (_v, buf) in list(views.items()) + list(zip(("gradinput1", "gradinput2"), grads)):
                assert bool((buf[:, :, :, W:] == 7.0).all()), "%s: the bytes behind a row of %s were written" % (what, n)
            runs.append([g.clone() for g, _buf in grads])
        assert all(torch.equal(a_, b_) for a_, b_ in zip(*runs))
        for n in names:                                   # the inputs themselves are untouched as well
            exact(t[n], h[n], "%s: input %s after the calls" % (name, n))


# ==================================================================================================================
# the frame and its context features in one pass (fi_fwd_ctx_img<BLEND>)
# ==================================================================================================================
def ctx_call(img, ctxf, flow, filt, prev=None, oa=None, ob=None):
    """FilterInterpolationCtxLayer_gpu_forward into NaN-filled outputs; the entry point records no kernel path: its status"""
    io, co = filled(img, NAN), filled(ctxf, NAN)
    assert F32().FilterInterpolationCtxLayer_gpu_forward(img, ctxf, flow, filt, prev, oa, ob, io, co) == 0
    return io, co


@pytest.mark.parametrize("ci", range(len(E.TABLE)), ids=E.TABLE_IDS)
def test_context_warp(oracle, ci):
    """launch 1 warps frame 0 and its context; launch 2 warps frame 2 and its context and blends the two frames (two
    products, one sum).  Lanes split over bands and sites no band covers blend one element at a time, out-of-range sites
    blend the input pixel: tests/test_exact_inputs.py::test_context_cases_reach_split_lanes_and_slow_sites_in_both_directions"""
    case = E.TABLE[ci]
    h = E.blend_inputs(case)
    key = ("table", ci, "fp32")
    t = {n: D(h[n]) for n in NAMES}
    for C in E.CTX_CHANNELS[ci]:
        c0, c2 = E.ctx_inputs(case, C)
        what = "context warp %s C%d" % (E.TABLE_IDS[ci], C)
        io, co = ctx_call(t["x0"], D(c0), t["f0"], t["k0"])
        exact(io, want_direction(oracle, key, h, 0)[4], what + ", launch 1: frame")
        exact(co, want_fi(oracle, ("ctx", ci, C, 0), c0, h["f0"], h["k0"]), what + ", launch 1: context")
        io2, co2 = ctx_call(t["x2"], D(c2), t["f1"], t["k1"], io, t["o0"], t["o1"])
        exact(io2, want_blend(oracle, key, h), what + ", launch 2: blended frame")
        exact(co2, want_fi(oracle, ("ctx", ci, C, 1), c2, h["f1"], h["k1"]), what + ", launch 2: context")


@pytest.mark.parametrize("name", E.CTX_LAYER)
def test_context_layer(oracle, name):
    """FilterInterpolationCtxBlendModule: the fused route, and the two shapes it composes from the separate operators"""
    from my_package.functions.FilterInterpolationCtxBlendLayer import fused_supported
    from my_package.modules.FilterInterpolationCtxBlendModule import FilterInterpolationCtxBlendModule
    h = E.ctx_layer_inputs(name)
    names = ("x0", "x2", "c0", "c2", "f0", "f1", "k0", "k1", "o0", "o1")
    t = {n: D(h[n]) for n in names}
    assert fused_supported(t["x0"], t["c0"], t["k0"], t["o0"], *[t[n] for n in ("x2", "c2", "f0", "f1", "k1", "o1")]) == \
        (name == "fused-C8")
    with torch.no_grad():
        blended, c0w, c2w = FilterInterpolationCtxBlendModule()(*[t[n] for n in names])
    key = ("ctxlayer", name)
    exact(blended, want_blend(oracle, key, h), name + ": blended frame")
    exact(c0w, want_fi(oracle, key + (0,), h["c0"], h["f0"], h["k0"]), name + ": context 0")
    exact(c2w, want_fi(oracle, key + (1,), h["c2"], h["f1"], h["k1"]), name + ": context 2")


# ==================================================================================================================
# x4 upsampling of the scaled flow (flow_upsample4): the column loop's later trips, both divisor branches
# ==================================================================================================================
UP_IDS = ["%dx%dx%dx%d" % s for s in E.UPSAMPLE_SHAPES]


def upsample_call(f, mul, div, align):
    B, C, h, w = f.shape
    out = torch.full((B, C, 4 * h, 4 * w), NAN, device="cuda")
    assert F32().FlowUpsample4Layer_gpu_forward(f, out, mul, div, align) == 0
    return out


@pytest.mark.parametrize("mul,div", E.UPSAMPLE_SCALES)
@pytest.mark.parametrize("shape", E.UPSAMPLE_SHAPES, ids=UP_IDS)
def test_flow_upsample4_exact(shape, mul, div):
    """align_corners = False: weights k / 8 per axis on an exactly scaled flow -- torch's CPU result in float64 is the
    expectation (tests/test_exact_inputs.py::test_upsample_inputs: its fp32 result is the same numbers)"""
    import torch.nn.functional as F
    f = E.upsample_input(shape)
    want = once(("up", shape, mul, div), lambda: F.interpolate(mul * torch.from_numpy(f).double() / div, scale_factor=4,
                                                               mode="bilinear", align_corners=False).numpy())
    exact(upsample_call(D(f), mul, div, False), want, "flow_upsample4 %s * %g / %g" % (shape, mul, div))


@pytest.mark.parametrize("mul,div", E.UPSAMPLE_SCALES)
@pytest.mark.parametrize("shape", E.UPSAMPLE_SHAPES, ids=UP_IDS)
def test_flow_upsample4_align_corners(shape, mul, div):
    """align_corners = True has no dyadic weights: the rule of test_gpu_parity.test_flow_upsample4, against the torch
    expression the kernel replaces"""
    import torch.nn.functional as F
    f = D(E.upsample_input(shape))
    got = upsample_call(f, mul, div, True)
    want = F.interpolate(mul * f / div, scale_factor=4, mode="bilinear", align_corners=True)
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    print("flow_upsample4 align_corners %s * %g / %g: max error %g, max |want| %g" % (shape, mul, div, err, float(want.abs().max())))
    assert err <= 2e-5 * max(1.0, float(want.abs().max())), err
