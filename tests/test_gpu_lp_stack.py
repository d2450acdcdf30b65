"""The stacked adaptive-warp forward on float16 / bfloat16 (libmemc_hip_lp_stack.so, my_lib_lp_stack,
FilterInterpolationStackLayer's half route), MEMC_Net_VE cast to half precision and the video-enhancement loop with
dtype=.

Six neighbours of two batch elements, stacked neighbour-major (row n * B + b), C = 3 (the RGB kernel) and C = 8 (the chunk
pipeline), with and without a slot left for the centre, the flow in T and in float32.  `out` is pre-filled with the byte
0xFF; every written slot must be `torch.equal` to FilterInterpolationLayer_gpu_forward_lp on that neighbour's contiguous
rows, every tap slot must have the taps' bits, every flow slot the bits of `flow.to(T)`, every other byte of `out` must
still be 0xFF, and the widened values must lie within tests/_netcalls.rule_lp_forward of the oracle on the widened inputs.

Shapes and path expectations: tests/_lp_stack_cases.py (those of tests/test_gpu_stack.py), the census taken on the flow as
rounded to T.  The half library's tile grid is unshifted, so the census is the kernel's own at W = 256 too.
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
import _lowp_paths as LP                   # noqa: E402
import _lp_stack_cases as K                # noqa: E402
import _netcalls as NC                     # noqa: E402
import _netutil                            # noqa: E402
import _septuplets as SP                   # noqa: E402
from tools import synth                    # noqa: E402

pytestmark = pytest.mark.gpu
N, B = K.N, K.B
TNAMES = ["fp16", "bf16"]
FLOWS = ["flowT", "flow32"]


def LPL():
    import my_package._ext.my_lib_lp as M
    return M


def LPS():
    import my_package._ext.my_lib_lp_stack as M
    return M


def D(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def per_neighbour_reference(x, flow, taps, path=None):
    """FilterInterpolationLayer_gpu_forward_lp on each neighbour's contiguous rows -> [N * B, C, H, W]"""
    want = torch.empty_like(x)
    for n in range(N):
        rows = slice(n * B, (n + 1) * B)
        assert LPL().FilterInterpolationLayer_gpu_forward_lp(x[rows], flow[rows], taps[rows], want[rows]) == 0
        if path is not None:
            assert LPL().last_kernel_path() == path
    return want


def reference(name, C, tname, flowkind):
    """(device tensors x, flow, taps in their storage, the half library's result, the oracle's fp32 result on the widened
    inputs as numpy); computed once, never written"""
    def make():
        T = K.DTYPES[tname]
        x, flow, taps = K.inputs(name, C)
        dx, dk = D(x, T), D(taps, T)
        df = D(flow, T) if flowkind == "flowT" else D(flow)
        from oracle import memc_oracle as O
        oracle = O.filter_interpolation_forward(NC.widen(dx), NC.widen(df), NC.widen(dk))
        return dx, df, dk, per_neighbour_reference(dx, df, dk, K.LP_PATH[C]), oracle
    return K.once(("reference", name, C, tname, flowkind), make)


def test_the_shapes_reach_every_path_between_them():
    reached = set()
    for name in K.SHAPES:
        reached |= {k for k, v in K.SHAPES[name][3].items() if v}
    assert reached == {"one_band", "bands", "capped", "slow", "split", "empty", "invalid", "mixed"}
    H, W = K.SHAPES["20x72-smooth"][:2]
    assert (W + LP.TW - 1) // LP.TW == 2 and (H + LP.TH - 1) // LP.TH == 2 and W % LP.TW and H % LP.TH


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_the_rounded_flow_reaches_the_shape_s_paths(name, tname):
    K.check_census(name, tname)


@pytest.mark.parametrize("flowkind", FLOWS)
@pytest.mark.parametrize("skip", [3, -1])
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_stacked_forward_is_the_half_library_s_bit_for_bit(name, tname, C, skip, flowkind):
    T = K.DTYPES[tname]
    x, flow, taps, want, oracle = reference(name, C, tname, flowkind)
    K.check_census(name, tname)
    lay = K.Layout(C, skip)
    H, W = x.shape[2:]
    out = K.ff_filled(T, B, lay.ctot, H, W)
    assert LPS().FilterInterpolationStackLayer_gpu_forward_lp(x, flow, taps, out, *lay.args()) == 0
    assert LPS().last_kernel_path() == K.PATH[C]
    K.check_out(out, lay, want, flow, taps)
    got = torch.cat([out[:, lay.warp(n)] for n in range(N)], 0)
    NC.rule_lp_forward(got, oracle, T, "stacked %s warp %s C=%d skip=%d %s vs oracle" % (tname, name, C, skip, flowkind))


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("tname", TNAMES)
def test_without_pass_through_and_with_the_flow_alone(tname, C):
    T = K.DTYPES[tname]
    for flowkind in FLOWS:
        x, flow, taps, want, _oracle = reference("20x72-smooth", C, tname, flowkind)
        H, W = x.shape[2:]
        lay = K.Layout(C, 3, passthrough=False)
        out = K.ff_filled(T, B, lay.ctot, H, W)
        assert LPS().FilterInterpolationStackLayer_gpu_forward_lp(x, flow, taps, out, *lay.args()) == 0
        K.check_out(out, lay, want, flow, taps)
        lay = K.Layout(C, 0)                                   # the centre's slot in front; the flows, but no taps
        out = K.ff_filled(T, B, lay.ctot, H, W)
        assert LPS().FilterInterpolationStackLayer_gpu_forward_lp(x, flow, taps, out, N, lay.c_base, 0, lay.flow_base, -1) == 0
        for n in range(N):
            assert torch.equal(out[:, lay.warp(n)], want[n * B:(n + 1) * B])
            assert K.same_bits(out[:, lay.flow(n)], flow[n * B:(n + 1) * B].to(T))
        assert K.all_ff(out[:, lay.tap_base:])
        assert K.all_ff(out[:, lay.c_base:lay.c_base + C])     # the centre's slot


@pytest.mark.parametrize("flowkind", FLOWS)
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("name", ["20x72-smooth", "96x256-bands", "112x320-slow"])
def test_exact_arithmetic_inputs_equal_the_oracle(name, tname, C, flowkind):
    """tests/_exact.py's grid (pixels k / 16, taps k / 8, flows on quarter pixels): pixels and taps are numbers of T, every
    product and partial sum is a number of fp32, so the oracle's answer rounded to T once is an exact expectation.  A flow
    stored in T is rounded to T first (it stays on a dyadic grid no finer than quarter pixels) and the oracle reads that."""
    from oracle import memc_oracle as O
    T = K.DTYPES[tname]
    H, W, (_b, _h, _w, kind, sigma, seed), _paths = K.SHAPES[name]
    x, flow, taps, _gout = E.shaped_inputs(N * B, C, H, W, kind, sigma, seed)
    dx, dk = D(x, T), D(taps, T)
    assert torch.equal(dx.float().cpu(), torch.from_numpy(x)) and torch.equal(dk.float().cpu(), torch.from_numpy(taps))
    df = D(flow, T) if flowkind == "flowT" else D(flow)
    want = D(O.filter_interpolation_forward(x, NC.widen(df), taps)).to(T)
    lay = K.Layout(C, 3)
    out = K.ff_filled(T, B, lay.ctot, H, W)
    assert LPS().FilterInterpolationStackLayer_gpu_forward_lp(dx, df, dk, out, *lay.args()) == 0
    K.check_out(out, lay, want, df, dk)


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("tname", TNAMES)
def test_own_strides_are_honoured(tname, C):
    """`out` a [..., :W] view of a wider tensor with a larger batch stride, and a view of it that starts at a channel and a
    column offset; input1 a padded view: the same bits, nothing written outside the view"""
    T = K.DTYPES[tname]
    x, flow, taps, want, _oracle = reference("20x72-smooth", C, tname, "flowT")
    H, W = x.shape[2:]
    lay = K.Layout(C, 3)
    xpad = K.ff_filled(T, N * B, C + 1, H + 2, W + 12)
    xv = xpad[:, :C, 1:H + 1, 4:W + 4]
    xv.copy_(x)
    assert not xv.is_contiguous() and xv.data_ptr() % 8 == 0
    for c0, x0 in ((0, 0), (2, 4)):                            # padded; padded and offset by two channels and four columns
        wide = K.ff_filled(T, B, lay.ctot + 3, H + 1, W + 8)
        out = wide[:, c0:c0 + lay.ctot, :H, x0:x0 + W]
        assert out.stride() == ((lay.ctot + 3) * (H + 1) * (W + 8), (H + 1) * (W + 8), W + 8, 1)
        assert out.data_ptr() % 8 == 0 and (x0 == 0 or out.data_ptr() % 16 == 8)
        assert LPS().FilterInterpolationStackLayer_gpu_forward_lp(xv, flow, taps, out, *lay.args()) == 0
        assert LPS().last_kernel_path() == K.PATH[C]
        K.check_out(out, lay, want, flow, taps)
        mask = torch.ones_like(wide, dtype=torch.bool)
        mask[:, c0:c0 + lay.ctot, :H, x0:x0 + W] = False
        assert bool((wide.view(torch.int16)[mask] == -1).all()), "written outside the view"


@pytest.mark.parametrize("what", ["C5", "W70", "misaligned"])
@pytest.mark.parametrize("tname", TNAMES)
def test_declined_calls_go_through_the_layer_composed(tname, what):
    from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer
    T = K.DTYPES[tname]
    C, H, W = (5, 20, 72) if what == "C5" else (3, 20, 70) if what == "W70" else (3, 20, 72)
    rng = np.random.default_rng(77)
    flow = D(synth.np_flow(rng, N * B, H, W, "smooth", 6.0), T)
    x, taps = D(synth.np_image(rng, N * B, C, H, W), T), D(synth.np_filter(rng, N * B, H, W), T)
    lay = K.Layout(C, 3)
    if what == "misaligned":
        out = K.ff_filled(T, B * lay.ctot * H * W + 1)[1:].view(B, lay.ctot, H, W)
        assert out.data_ptr() % 8 == 2
    else:
        out = K.ff_filled(T, B, lay.ctot, H, W)
    before = LPS().last_kernel_path()
    assert LPS().FilterInterpolationStackLayer_gpu_forward_lp(x, flow, taps, out, *lay.args()) == 1
    assert K.all_ff(out)                                       # a declined call writes nothing
    got = FilterInterpolationStackLayer()(out, x, flow, taps, lay.c_base, lay.skip, lay.flow_base, lay.tap_base)
    assert got is out
    assert LPL().last_kernel_path().startswith("fi_fwd_lp:") and LPS().last_kernel_path() == before
    K.check_out(out, lay, per_neighbour_reference(x, flow, taps), flow, taps)


def test_the_binding_refuses_other_dtypes():
    x, flow, taps = (D(a, torch.bfloat16) for a in K.inputs("16x8", 3))
    lay = K.Layout(3, 3)
    out = torch.zeros((B, lay.ctot, 16, 8), dtype=torch.bfloat16, device="cuda")
    f = LPS().FilterInterpolationStackLayer_gpu_forward_lp
    for bad in ((x.float(), flow.float(), taps.float(), out.float()), (x.half(), flow, taps, out), (x, flow.half(), taps, out),
                (x, flow, taps.float(), out), (x, flow, taps, out.half()), (x, flow.double(), taps, out)):
        with pytest.raises(TypeError):
            f(*bad, *lay.args())
    assert f(x, flow.float(), taps, out, *lay.args()) == 0     # a float32 flow is the one exception


# ---- autograd ------------------------------------------------------------------------------------------------------
AH, AW = 16, 24


def _autograd_inputs(C, T):
    rng = np.random.default_rng(91)
    flow = D(synth.np_flow(rng, N * B, AH, AW, "smooth", 3.0), T)
    x, taps = D(synth.np_image(rng, N * B, C, AH, AW), T), D(synth.np_filter(rng, N * B, AH, AW), T)
    lay = K.Layout(C, 3)
    weight = D(rng.standard_normal((B, lay.ctot, AH, AW)).astype(np.float32), T)
    return x, flow, taps, lay, weight


def _composed(x, flow, taps, lay):
    """six module calls + cat: zeros in the gaps and in the centre's slot"""
    from my_package.modules.FilterInterpolationModule import FilterInterpolationModule
    zeros = lambda c: torch.zeros((B, c, AH, AW), device="cuda", dtype=x.dtype)      # noqa: E731
    rows = [slice(n * B, (n + 1) * B) for n in range(N)]
    warped = [FilterInterpolationModule()(x[r], flow[r], taps[r]) for r in rows]
    warped.insert(lay.skip, zeros(lay.C))
    return torch.cat([zeros(1)] + warped + [zeros(2)] + [flow[r] for r in rows] + [zeros(1)] + [taps[r] for r in rows]
                     + [zeros(3)], dim=1)


@pytest.mark.parametrize("image_grad", [False, True])
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("tname", TNAMES)
def test_autograd_equals_the_composed_route(tname, C, image_grad):
    from my_package.modules.FilterInterpolationStackModule import FilterInterpolationStackModule
    T = K.DTYPES[tname]
    x, flow, taps, lay, weight = _autograd_inputs(C, T)
    grads = {}
    for route in ("stacked", "composed"):
        xr = x.clone().requires_grad_(image_grad)
        fr, kr = flow.clone().requires_grad_(True), taps.clone().requires_grad_(True)
        if route == "stacked":
            out = torch.zeros((B, lay.ctot, AH, AW), device="cuda", dtype=T)
            r = FilterInterpolationStackModule()(out, xr, fr, kr, lay.c_base, lay.skip, lay.flow_base, lay.tap_base)
            assert r is out and r.requires_grad and LPS().last_kernel_path() == K.PATH[C]
        else:
            before = LPS().last_kernel_path()
            r = _composed(xr, fr, kr, lay)
            assert LPS().last_kernel_path() == before
        grads[route + "/values"] = r.detach().clone()
        (r * weight).sum().backward()
        grads[route] = (xr.grad, fr.grad, kr.grad)
    assert torch.equal(grads["stacked/values"], grads["composed/values"])
    assert grads["stacked"][1].dtype == grads["stacked"][2].dtype == T
    assert torch.equal(grads["stacked"][1], grads["composed"][1])        # flow: the warps' gradient + the pass-through's
    assert torch.equal(grads["stacked"][2], grads["composed"][2])        # taps
    if image_grad:                                                       # (atomics: hardware order)
        NC.rule_rounded(grads["stacked"][0], grads["composed"][0], T,
                        "stacked %s warp image gradient C=%d vs composed" % (tname, C))
    else:
        assert grads["stacked"][0] is None and grads["composed"][0] is None


@pytest.mark.parametrize("tname", TNAMES)
def test_pass_through_slices_receive_gradient(tname):
    from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer
    T = K.DTYPES[tname]
    x, flow, taps, lay, weight = _autograd_inputs(3, T)
    fr, kr = flow.clone().requires_grad_(True), taps.clone().requires_grad_(True)
    out = torch.zeros((B, lay.ctot, AH, AW), device="cuda", dtype=T)
    r = FilterInterpolationStackLayer()(out, x, fr, kr, lay.c_base, lay.skip, lay.flow_base, lay.tap_base)
    assert LPS().last_kernel_path() == K.PATH[3]
    only = torch.zeros_like(weight)                                      # a loss on the pass-through slices alone
    only[:, lay.flow_base:lay.flow_base + 2 * N] = weight[:, lay.flow_base:lay.flow_base + 2 * N]
    only[:, lay.tap_base:lay.tap_base + 16 * N] = weight[:, lay.tap_base:lay.tap_base + 16 * N]
    (r * only).sum().backward()
    for n in range(N):
        assert torch.equal(fr.grad[n * B:(n + 1) * B], weight[:, lay.flow(n)])
        assert torch.equal(kr.grad[n * B:(n + 1) * B], weight[:, lay.taps(n)])


@pytest.mark.parametrize("tname", TNAMES)
def test_detached_slices_carry_no_gradient(tname):
    from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer
    T = K.DTYPES[tname]
    x, flow, taps, lay, weight = _autograd_inputs(8, T)
    xr, fr, kr = (t.clone().requires_grad_(True) for t in (x, flow, taps))
    out = torch.zeros((B, lay.ctot, AH, AW), device="cuda", dtype=T)
    r = FilterInterpolationStackLayer()(out, xr, fr, kr, lay.c_base, lay.skip, lay.flow_base, lay.tap_base, detach=True)
    assert r is out and not r.requires_grad and LPS().last_kernel_path() == K.PATH[8]
    # an `out` that carries gradient of its own keeps it outside the written slices and loses it inside
    leaf = torch.zeros((B, lay.ctot, AH, AW), device="cuda", dtype=T, requires_grad=True)
    r = FilterInterpolationStackLayer()(leaf * 1.0, xr, fr, kr, lay.c_base, lay.skip, lay.flow_base, lay.tap_base, detach=True)
    (r * weight).sum().backward()
    assert xr.grad is None and fr.grad is None and kr.grad is None
    written = torch.zeros(lay.ctot, dtype=torch.bool, device="cuda")
    for n in range(N):
        written[lay.warp(n)] = written[lay.flow(n)] = written[lay.taps(n)] = True
    assert torch.equal(leaf.grad[:, ~written], weight[:, ~written]) and bool((leaf.grad[:, written] == 0).all())


# ---- the routes the half kernel does not take ------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TNAMES)
def test_native_half_off_takes_the_composed_route(tname):
    from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer
    T = K.DTYPES[tname]
    x, flow, taps, want, _oracle = reference("20x72-smooth", 3, tname, "flowT")
    lay = K.Layout(3, 3)
    was = FilterInterpolationStackLayer.native_half
    try:
        for on in (True, False):
            FilterInterpolationStackLayer.native_half = on
            out = K.ff_filled(T, B, lay.ctot, 20, 72)
            if on:                                             # move the path off this kernel's, so that a call shows
                x8 = reference("20x72-smooth", 8, tname, "flowT")[0]
                FilterInterpolationStackLayer()(K.ff_filled(T, B, K.Layout(8, 3).ctot, 20, 72), x8, flow, taps, 1, 3)
                assert LPS().last_kernel_path() == K.PATH[8]
            before = LPS().last_kernel_path()
            FilterInterpolationStackLayer()(out, x, flow, taps, lay.c_base, lay.skip, lay.flow_base, lay.tap_base)
            assert LPS().last_kernel_path() == (K.PATH[3] if on else before)
            K.check_out(out, lay, want, flow, taps)
    finally:
        FilterInterpolationStackLayer.native_half = was


def test_an_autocast_call_and_a_mixed_call_keep_the_composed_route():
    from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer
    T = torch.bfloat16
    x, flow, taps, want, _oracle = reference("20x72-smooth", 3, "bf16", "flowT")
    lay = K.Layout(3, 3)
    was = FilterInterpolationStackLayer.native_half
    FilterInterpolationStackLayer.native_half = True
    try:
        x8 = reference("20x72-smooth", 8, "bf16", "flowT")[0]      # a plain call first: the path is the C = 8 kernel's
        FilterInterpolationStackLayer()(K.ff_filled(T, B, K.Layout(8, 3).ctot, 20, 72), x8, flow, taps, 1, 3)
        before = LPS().last_kernel_path()
        assert before == K.PATH[8]
        out = K.ff_filled(T, B, lay.ctot, 20, 72)
        with torch.autocast("cuda", dtype=T):
            FilterInterpolationStackLayer()(out, x, flow, taps, lay.c_base, lay.skip, lay.flow_base, lay.tap_base)
        assert LPS().last_kernel_path() == before
        K.check_out(out, lay, want, flow, taps)
        # mixed: a float32 `out` beside half inputs
        out32 = torch.zeros((B, lay.ctot, 20, 72), device="cuda")
        FilterInterpolationStackLayer()(out32, x, flow, taps, lay.c_base, lay.skip, lay.flow_base, lay.tap_base)
        assert LPS().last_kernel_path() == before
        for n in range(N):
            assert torch.equal(out32[:, lay.warp(n)], want[n * B:(n + 1) * B].float())
    finally:
        FilterInterpolationStackLayer.native_half = was


# ---- the network ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", ["bf16", "fp16"])
def test_memc_net_ve_cast_to_half_assembles_the_same_rectifier_input_by_both_routes(tname):
    """64 x 64, batch 2, named weights, the model cast to T.  The flow, the taps and the seven contexts are computed once
    and handed to both routes; the routes that assemble the rectifier input must give the same bits."""
    import networks
    from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer
    T = K.DTYPES[tname]
    dev = torch.device("cuda", 0)
    net = networks.MEMC_Net_VE(batch=1, channel=3, width=None, height=None, scale_num=1, scale_ratio=2, temporal=False,
                               filter_size=4, save_which=1, debug=False, offset_scale=None, cuda_available=True, cuda_id=None,
                               training=False)
    net.load_state_dict(_netutil.named_weights(net.state_dict()), warn_align_corners=False)
    net = net.to(dev).to(T).eval()
    g = torch.Generator().manual_seed(31)
    xs = [torch.rand((2, 3, 64, 64), generator=g).to(dev).to(T) for _ in range(7)]
    was = FilterInterpolationStackLayer.native_half
    FilterInterpolationStackLayer.native_half = True
    try:
        with torch.no_grad():
            flow, taps = net._estimate(xs)
            assert flow.dtype == taps.dtype == T
            contexts = [net.ctxNet(x) for x in xs]
            net.fused_stack = True
            assert net._use_stack(xs, flow, taps)
            stacked = net.rectifier_input(xs, flow, taps, contexts)
            assert LPS().last_kernel_path() == K.PATH[3]                 # the frames' call is the second of the two
            net.fused_stack = False
            before = LPS().last_kernel_path()
            composed = net.rectifier_input(xs, flow, taps, contexts)
            assert LPS().last_kernel_path() == before
            assert stacked.dtype == composed.dtype == T
            assert stacked.shape == composed.shape == (2, 577, 64, 64)
            assert torch.equal(stacked, composed)
            assert torch.equal(stacked[:, 556 + 9:556 + 12], xs[3]) and torch.equal(stacked[:, 192:256], contexts[3])
            for fused in (True, False):
                net.fused_stack = fused
                y = net(xs)
                assert y.shape == (2, 3, 64, 64) and y.dtype == T and bool(torch.isfinite(y).all())
            with torch.autocast("cuda", dtype=T):                        # autocast: the composed route whatever fused_stack says
                assert not net._use_stack(xs, flow, taps)
    finally:
        FilterInterpolationStackLayer.native_half = was


# ---- the loop ------------------------------------------------------------------------------------------------------
def test_the_loop_in_bf16_writes_the_same_bytes_and_scores_with_and_without_gpu_io(tmp_path):
    import networks
    import networks.png_io as png
    dev = torch.device("cuda", 0)
    root = str(tmp_path / "vimeo")
    SP.write_tree(root, png.write_png)
    runs = {}
    for name, kw in (("host", dict()), ("gpu", dict(gpu_io=True))):
        model = K.HalfStubEnhancer(torch.bfloat16)
        runs[name] = networks.enhance_septuplet_tree(model, os.path.join(root, "input"), os.path.join(root, "target"),
                                                     str(tmp_path / name), dev, dtype=torch.bfloat16, **kw)
        assert model.shapes == [SP.padded_shape(h, w) for _c, h, w in SP.CLIPS]
    assert runs["gpu"] == runs["host"] and len(runs["gpu"]) == len(SP.CLIPS)
    for clip, h, w in SP.CLIPS:
        a, b = (open(os.path.join(str(tmp_path / name), clip, "im4.png"), "rb").read() for name in ("gpu", "host"))
        assert a == b and png.read_png(os.path.join(str(tmp_path / "gpu"), clip, "im4.png")).shape == (h, w, 3)
    metrics = [open(os.path.join(str(tmp_path / name), "metrics.txt")).read() for name in ("gpu", "host")]
    assert metrics[0] == metrics[1] and metrics[0].startswith("The average interpolation error / PSNR for all images are : ")
    # the precision arguments are checked before a file is read
    with pytest.raises(ValueError):
        networks.enhance_septuplet_tree(model, "/nonexistent", "/nonexistent", str(tmp_path / "x"), dev,
                                        dtype=torch.bfloat16, autocast=torch.bfloat16)
    with pytest.raises(TypeError):
        networks.enhance_septuplet_tree(model, "/nonexistent", "/nonexistent", str(tmp_path / "x"), dev, dtype=torch.float64)


def test_the_loop_under_autocast_feeds_float32_planes(tmp_path):
    """autocast=: the float32 stub (it insists on float32 planes; none of its operations is one autocast casts) inside
    torch.autocast, with gpu_io on and off: the bytes and scores of the default run"""
    import networks
    import networks.png_io as png
    dev = torch.device("cuda", 0)
    root = str(tmp_path / "vimeo")
    SP.write_tree(root, png.write_png)
    runs = {}
    for name, kw in (("default", dict()), ("host", dict(autocast=torch.bfloat16)),
                     ("gpu", dict(autocast=torch.bfloat16, gpu_io=True))):
        runs[name] = networks.enhance_septuplet_tree(SP.StubEnhancer(), os.path.join(root, "input"),
                                                     os.path.join(root, "target"), str(tmp_path / name), dev, **kw)
    assert runs["host"] == runs["default"] and runs["gpu"] == runs["default"]
    for clip, _h, _w in SP.CLIPS:
        a, b, c = (open(os.path.join(str(tmp_path / name), clip, "im4.png"), "rb").read() for name in ("default", "host", "gpu"))
        assert a == b == c


def test_the_command_line_tool_runs_a_cast_network_over_a_tree(tmp_path, capsys):
    """tools/demo_vimeo_ve.py --precision bf16 --gpu-io on the two 24 x 40 clips of the synthetic tree: MEMC_Net_VE on its
    random initialisation, cast to bfloat16, the pixel work on the device"""
    import networks.png_io as png
    from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer
    from tools import demo_vimeo_ve as demo
    root = str(tmp_path / "vimeo")
    SP.write_tree(root, png.write_png)
    listing = str(tmp_path / "sep_testlist.txt")
    clips = [c for c, h, _w in SP.CLIPS if h == 24]
    open(listing, "w").write("".join(c + "\n" for c in clips))
    out = str(tmp_path / "bf16")
    before = LPS().last_kernel_path()
    torch.manual_seed(3)
    demo.main(["--input", os.path.join(root, "input"), "--target", os.path.join(root, "target"), "--list", listing,
               "--output", out, "--precision", "bf16", "--gpu-io"])
    text = capsys.readouterr().out.strip().split("\n")
    assert len(text) == len(clips) + 1 and text[-1] == open(os.path.join(out, "metrics.txt")).read().rstrip("\n")
    assert text[-1].startswith("The average interpolation error / PSNR for all images are : ")
    for c in clips:
        assert png.read_png(os.path.join(out, c, "im4.png")).shape == (24, 40, 3)
    assert LPS().last_kernel_path() == (K.PATH[3] if FilterInterpolationStackLayer.native_half else before)
