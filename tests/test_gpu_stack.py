"""The stacked adaptive-warp forward (libmemc_hip_stack.so, my_lib_stack, FilterInterpolationStackLayer), MEMC_Net_VE on the
device and the video-enhancement loop with its pixel work on the device.

Six neighbours of two batch elements, stacked neighbour-major (row n * B + b), C = 3 (the RGB kernel) and C = 8 (the chunk
pipeline), with and without a slot left for the centre.  `out` is pre-filled with the byte 0xFF; every written slot must be
`torch.equal` to FilterInterpolationLayer_gpu_forward on that neighbour's rows, every pass-through slot `torch.equal` to the
flow and the taps, every other byte of `out` still 0xFF, and the values within tests/_parity.py's rule of the oracle.

Shapes: 20 x 72 (two tile columns and two tile rows, both edge tiles part empty) and 16 x 8 (the narrowest width) reach
the one-band path, empty tiles and out-of-range sites; an image of 20 x 72 cannot reach more -- a tile's source box is
clipped to the image, and 72 x 20 pixels fit one LDS band -- so the band sweep, the capped tiles and the in-kernel one-site
path run at the shapes of the census cases that reach them (tests/_lowp_paths.py: CASES[0], 96 x 256, and CASES[2],
112 x 320).  Every flow is drawn as a census case draws its own (kind, sigma, seed: imported, not copied), at twelve rows;
tests/_lowp_paths.census counts, on the CPU, which paths the flow that is actually run reaches, and the test asserts it.
(The census tiles from x = 0.  With rows of a multiple of 1 KiB -- W = 256 here -- the RGB kernels of the fp32 library and
of this one shift their tile grid 32 sites left, so for that one case the counts are those of a neighbouring tiling; at
W = 320, and for C = 8 at either width, they are the kernel's own.  That case is also the one that shows a wrong grid:
the one-site path and the gather differ in the last bit at a few dozen sites, so the bits match only on the same tiles.)
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
import _netutil                            # noqa: E402
import _parity as P                        # noqa: E402
import _septuplets as SP                   # noqa: E402
from tools import synth                    # noqa: E402

pytestmark = pytest.mark.gpu
N, B = 6, 2                                # neighbours, batch elements

# name -> (H, W, the census case whose flow kind, sigma and seed are used, what tests/_lowp_paths.census must report)
SHAPES = {
    "20x72-smooth": (20, 72, LP.CASES[4], dict(one_band=True, empty=True, invalid=True, mixed=True)),
    "20x72-iid": (20, 72, LP.CASES[5], dict(one_band=True, invalid=True, mixed=True)),
    "16x8": (16, 8, LP.CASES[4], dict(one_band=True, empty=True, invalid=True)),
    "96x256-bands": (96, 256, LP.CASES[0], dict(bands=True, capped=True, slow=True, split=True, invalid=True)),
    "112x320-slow": (112, 320, LP.CASES[2], dict(bands=True, capped=True, slow=True, split=True, invalid=True)),
}
PATH = {3: "fi_fwd_stack:tiled_c3", 8: "fi_fwd_stack:tiled_c4n"}


def F32():
    import my_package._ext.my_lib as M
    return M


def STK():
    import my_package._ext.my_lib_stack as M
    return M


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def inputs(name, C):
    """(image [12, C, H, W], flow, taps) as numpy, the flow drawn first as the census cases draw theirs; never written"""
    def make():
        H, W, (_b, _h, _w, kind, sigma, seed), _paths = SHAPES[name]
        rng = np.random.default_rng(seed)
        flow = synth.np_flow(rng, N * B, H, W, kind, sigma)
        return synth.np_image(rng, N * B, C, H, W), flow, synth.np_filter(rng, N * B, H, W)
    return _once(("inputs", name, C), make)


def per_neighbour_reference(x, flow, taps):
    """FilterInterpolationLayer_gpu_forward on each neighbour's rows -> [N * B, C, H, W]"""
    want = torch.full_like(x, float("nan"))
    for n in range(N):
        rows = slice(n * B, (n + 1) * B)
        assert F32().FilterInterpolationLayer_gpu_forward(x[rows], flow[rows], taps[rows], want[rows]) == 0
    return want


def reference(name, C):
    """(device tensors x, flow, taps, the fp32 library's result, the oracle's result as numpy); computed once"""
    def make():
        x, flow, taps = inputs(name, C)
        from oracle import memc_oracle as O
        dx, df, dk = D(x), D(flow), D(taps)
        return dx, df, dk, per_neighbour_reference(dx, df, dk), O.filter_interpolation_forward(x, flow, taps)
    return _once(("reference", name, C), make)


class Layout:
    """channel layout of `out`: a gap, the warps (with or without the centre's slot), a gap, the flows, a gap, the taps, a gap"""

    def __init__(self, C, skip, passthrough=True):
        self.C, self.skip = C, skip
        slots = N + (1 if skip >= 0 else 0)
        self.c_base = 1
        self.flow_base = self.c_base + slots * C + 2 if passthrough else -1
        self.tap_base = self.flow_base + 2 * N + 1 if passthrough else -1
        self.ctot = (self.tap_base + 16 * N + 3) if passthrough else self.c_base + slots * C + 2

    def slot(self, n):
        return n + (1 if 0 <= self.skip <= n else 0)

    def warp(self, n):
        return slice(self.c_base + self.slot(n) * self.C, self.c_base + (self.slot(n) + 1) * self.C)

    def flow(self, n):
        return slice(self.flow_base + 2 * n, self.flow_base + 2 * n + 2)

    def taps(self, n):
        return slice(self.tap_base + 16 * n, self.tap_base + 16 * n + 16)

    def args(self):
        return (N, self.c_base, self.skip, self.flow_base, self.tap_base)


def ff_filled(*shape):
    """a float32 tensor of `shape` whose every byte is 0xFF"""
    return torch.full(shape[:-1] + (4 * shape[-1],), 0xFF, dtype=torch.uint8, device="cuda").view(torch.float32)


def check_out(out, lay, want, flow, taps):
    """written slots == want's rows, pass-through == flow / taps, every other channel still 0xFF bytes"""
    touched = torch.zeros(out.size(1), dtype=torch.bool)
    for n in range(N):
        rows = slice(n * B, (n + 1) * B)
        assert torch.equal(out[:, lay.warp(n)], want[rows]), "neighbour %d" % n
        touched[lay.warp(n)] = True
        if lay.flow_base >= 0:
            assert torch.equal(out[:, lay.flow(n)].view(torch.int32), flow[rows].view(torch.int32)), "flow %d" % n
            assert torch.equal(out[:, lay.taps(n)].view(torch.int32), taps[rows].view(torch.int32)), "taps %d" % n
            touched[lay.flow(n)] = True
            touched[lay.taps(n)] = True
    rest = out[:, (~touched).nonzero().flatten().cuda()]
    assert rest.size(1) >= 3 + (lay.C if lay.skip >= 0 else 0)
    assert bool((rest.contiguous().view(torch.int32) == -1).all()), "a channel outside the written slices was touched"


def check_census(name, flow):
    c = LP.census(flow)
    want = SHAPES[name][3]
    print(name, c)
    assert c["valid"] > 0
    if want.get("one_band"):
        assert c["max_bands_run"] == 1 and c["nbx_gt1"] == 0 and c["nby_gt1"] == 0 and c["slow"] == 0
    if want.get("bands"):
        assert c["nbx_gt1"] > 0 and c["nby_gt1"] > 0 and c["max_bands_run"] > 1
    if want.get("capped"):
        assert c["capped"] > 0
    if want.get("slow"):
        assert c["slow"] > 0
    if want.get("split"):
        assert c["split_lanes"] > 0
    if want.get("empty"):
        assert c["empty"] > 0
    if want.get("invalid"):
        assert c["valid"] < c["sites"]
    if want.get("mixed"):
        assert c["mixed_lanes"] > 0


def test_the_shapes_reach_every_path_between_them():
    reached = set()
    for name in SHAPES:
        reached |= {k for k, v in SHAPES[name][3].items() if v}
    assert reached == {"one_band", "bands", "capped", "slow", "split", "empty", "invalid", "mixed"}
    H, W = SHAPES["20x72-smooth"][:2]
    assert (W + LP.TW - 1) // LP.TW == 2 and (H + LP.TH - 1) // LP.TH == 2 and W % LP.TW and H % LP.TH


@pytest.mark.parametrize("skip", [3, -1])
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("name", list(SHAPES))
def test_stacked_forward_is_the_fp32_library_s_bit_for_bit(name, C, skip):
    x, flow, taps, want, oracle = reference(name, C)
    check_census(name, inputs(name, C)[1])
    lay = Layout(C, skip)
    H, W = x.shape[2:]
    out = ff_filled(B, lay.ctot, H, W)
    assert STK().FilterInterpolationStackLayer_gpu_forward(x, flow, taps, out, *lay.args()) == 0
    assert STK().last_kernel_path() == PATH[C]
    check_out(out, lay, want, flow, taps)
    got = torch.cat([out[:, lay.warp(n)] for n in range(N)], 0)
    P.close(got.cpu().numpy(), oracle, "stacked warp %s C=%d skip=%d vs oracle" % (name, C, skip))


@pytest.mark.parametrize("C", [3, 8])
def test_without_pass_through_and_with_the_flow_alone(C):
    x, flow, taps, want, _oracle = reference("20x72-smooth", C)
    H, W = x.shape[2:]
    lay = Layout(C, 3, passthrough=False)
    out = ff_filled(B, lay.ctot, H, W)
    assert STK().FilterInterpolationStackLayer_gpu_forward(x, flow, taps, out, *lay.args()) == 0
    check_out(out, lay, want, flow, taps)
    lay = Layout(C, 0)                                     # the centre's slot in front; the flows, but no taps
    out = ff_filled(B, lay.ctot, H, W)
    assert STK().FilterInterpolationStackLayer_gpu_forward(x, flow, taps, out, N, lay.c_base, 0, lay.flow_base, -1) == 0
    for n in range(N):
        assert torch.equal(out[:, lay.warp(n)], want[n * B:(n + 1) * B])
        assert torch.equal(out[:, lay.flow(n)], flow[n * B:(n + 1) * B])
    assert bool((out[:, lay.tap_base:].contiguous().view(torch.int32) == -1).all())
    assert bool((out[:, lay.c_base:lay.c_base + C].contiguous().view(torch.int32) == -1).all())      # the centre's slot


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("name", ["20x72-smooth", "96x256-bands", "112x320-slow"])
def test_exact_arithmetic_inputs_equal_the_oracle(name, C):
    """tests/_exact.py's grid (pixels k / 16, taps k / 8, flows on quarter pixels): every product and partial sum is a number
    of fp32, so the oracle's answer is an exact expectation"""
    from oracle import memc_oracle as O
    H, W, (_b, _h, _w, kind, sigma, seed), _paths = SHAPES[name]
    x, flow, taps, _gout = E.shaped_inputs(N * B, C, H, W, kind, sigma, seed)
    want = D(O.filter_interpolation_forward(x, flow, taps))
    lay = Layout(C, 3)
    out = ff_filled(B, lay.ctot, H, W)
    assert STK().FilterInterpolationStackLayer_gpu_forward(D(x), D(flow), D(taps), out, *lay.args()) == 0
    check_out(out, lay, want, D(flow), D(taps))


@pytest.mark.parametrize("C", [3, 8])
def test_own_strides_are_honoured(C):
    """`out` a [..., :W] view of a wider tensor with a larger batch stride, input1 a padded view: the same bits"""
    x, flow, taps, want, _oracle = reference("20x72-smooth", C)
    H, W = x.shape[2:]
    lay = Layout(C, 3)
    wide = ff_filled(B, lay.ctot + 3, H + 1, W + 8)
    out = wide[:, :lay.ctot, :H, :W]
    assert out.stride() == ((lay.ctot + 3) * (H + 1) * (W + 8), (H + 1) * (W + 8), W + 8, 1)
    xpad = ff_filled(N * B, C + 1, H + 2, W + 12)
    xv = xpad[:, :C, 1:H + 1, 4:W + 4]
    xv.copy_(x)
    assert not xv.is_contiguous() and xv.data_ptr() % 16 == 0
    assert STK().FilterInterpolationStackLayer_gpu_forward(xv, flow, taps, out, *lay.args()) == 0
    assert STK().last_kernel_path() == PATH[C]
    check_out(out, lay, want, flow, taps)
    mask = torch.ones_like(wide, dtype=torch.bool)
    mask[:, :lay.ctot, :H, :W] = False
    assert bool((wide.view(torch.int32)[mask] == -1).all()), "written outside the view"


@pytest.mark.parametrize("what", ["C5", "W70", "misaligned"])
def test_declined_calls_go_through_the_layer_composed(what):
    from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer
    C, H, W = (5, 20, 72) if what == "C5" else (3, 20, 70) if what == "W70" else (3, 20, 72)
    rng = np.random.default_rng(77)
    flow = D(synth.np_flow(rng, N * B, H, W, "smooth", 6.0))
    x, taps = D(synth.np_image(rng, N * B, C, H, W)), D(synth.np_filter(rng, N * B, H, W))
    lay = Layout(C, 3)
    if what == "misaligned":
        out = ff_filled(B * lay.ctot * H * W + 1)[1:].view(B, lay.ctot, H, W)
        assert out.data_ptr() % 16 == 4
    else:
        out = ff_filled(B, lay.ctot, H, W)
    assert STK().FilterInterpolationStackLayer_gpu_forward(x, flow, taps, out, *lay.args()) == 1
    assert bool((out.contiguous().view(torch.int32) == -1).all())        # a declined call writes nothing
    before = STK().last_kernel_path()
    got = FilterInterpolationStackLayer()(out, x, flow, taps, lay.c_base, lay.skip, lay.flow_base, lay.tap_base)
    assert got is out
    assert F32().last_kernel_path().startswith("fi_fwd:") and STK().last_kernel_path() == before
    check_out(out, lay, per_neighbour_reference(x, flow, taps), flow, taps)


def test_half_tensors_take_the_composed_route():
    from my_package.functions.FilterInterpolationLayer import FilterInterpolationLayer
    from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer
    x, flow, taps = (D(a).half() for a in inputs("20x72-smooth", 3))
    lay = Layout(3, 3)
    out = torch.zeros((B, lay.ctot, 20, 72), dtype=torch.float16, device="cuda")
    before = STK().last_kernel_path()
    FilterInterpolationStackLayer()(out, x, flow, taps, lay.c_base, lay.skip, lay.flow_base, lay.tap_base)
    assert STK().last_kernel_path() == before
    want = FilterInterpolationLayer()(x, flow, taps)
    for n in range(N):
        assert torch.equal(out[:, lay.warp(n)], want[n * B:(n + 1) * B])
        assert torch.equal(out[:, lay.taps(n)], taps[n * B:(n + 1) * B])


# ---- autograd ------------------------------------------------------------------------------------------------------
AH, AW = 16, 24


def _autograd_inputs(C):
    rng = np.random.default_rng(91)
    flow = D(synth.np_flow(rng, N * B, AH, AW, "smooth", 3.0))
    x, taps = D(synth.np_image(rng, N * B, C, AH, AW)), D(synth.np_filter(rng, N * B, AH, AW))
    lay = Layout(C, 3)
    weight = D(rng.standard_normal((B, lay.ctot, AH, AW)).astype(np.float32))
    return x, flow, taps, lay, weight


def _composed(x, flow, taps, lay):
    """six module calls + cat: zeros in the gaps and in the centre's slot"""
    from my_package.modules.FilterInterpolationModule import FilterInterpolationModule
    zeros = lambda c: torch.zeros((B, c, AH, AW), device="cuda")      # noqa: E731
    rows = [slice(n * B, (n + 1) * B) for n in range(N)]
    warped = [FilterInterpolationModule()(x[r], flow[r], taps[r]) for r in rows]
    warped.insert(lay.skip, zeros(lay.C))
    return torch.cat([zeros(1)] + warped + [zeros(2)] + [flow[r] for r in rows] + [zeros(1)] + [taps[r] for r in rows]
                     + [zeros(3)], dim=1)


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("image_grad", [False, True])
def test_autograd_equals_the_composed_route(C, image_grad):
    from my_package.modules.FilterInterpolationStackModule import FilterInterpolationStackModule
    x, flow, taps, lay, weight = _autograd_inputs(C)
    grads = {}
    for route in ("stacked", "composed"):
        xr = x.clone().requires_grad_(image_grad)
        fr, kr = flow.clone().requires_grad_(True), taps.clone().requires_grad_(True)
        if route == "stacked":
            out = torch.zeros((B, lay.ctot, AH, AW), device="cuda")
            r = FilterInterpolationStackModule()(out, xr, fr, kr, lay.c_base, lay.skip, lay.flow_base, lay.tap_base)
            assert r is out and r.requires_grad and STK().last_kernel_path() == PATH[C]
        else:
            r = _composed(xr, fr, kr, lay)
        grads[route + "/values"] = r.detach().clone()
        (r * weight).sum().backward()
        grads[route] = (xr.grad, fr.grad, kr.grad)
    assert torch.equal(grads["stacked/values"], grads["composed/values"])
    assert torch.equal(grads["stacked"][1], grads["composed"][1])        # flow: the warps' gradient + the pass-through's
    assert torch.equal(grads["stacked"][2], grads["composed"][2])        # taps
    if image_grad:                                                       # (atomics: hardware order)
        P.close(grads["stacked"][0], grads["composed"][0], "stacked warp image gradient C=%d vs composed" % C)
    else:
        assert grads["stacked"][0] is None and grads["composed"][0] is None


def test_pass_through_slices_receive_gradient():
    from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer
    x, flow, taps, lay, weight = _autograd_inputs(3)
    fr, kr = flow.clone().requires_grad_(True), taps.clone().requires_grad_(True)
    out = torch.zeros((B, lay.ctot, AH, AW), device="cuda")
    r = FilterInterpolationStackLayer()(out, x, fr, kr, lay.c_base, lay.skip, lay.flow_base, lay.tap_base)
    only = torch.zeros_like(weight)                                      # a loss on the pass-through slices alone
    only[:, lay.flow_base:lay.flow_base + 2 * N] = weight[:, lay.flow_base:lay.flow_base + 2 * N]
    only[:, lay.tap_base:lay.tap_base + 16 * N] = weight[:, lay.tap_base:lay.tap_base + 16 * N]
    (r * only).sum().backward()
    for n in range(N):
        assert torch.equal(fr.grad[n * B:(n + 1) * B], weight[:, lay.flow(n)])
        assert torch.equal(kr.grad[n * B:(n + 1) * B], weight[:, lay.taps(n)])


def test_detached_slices_carry_no_gradient():
    from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer
    x, flow, taps, lay, weight = _autograd_inputs(8)
    xr, fr, kr = (t.clone().requires_grad_(True) for t in (x, flow, taps))
    out = torch.zeros((B, lay.ctot, AH, AW), device="cuda")
    r = FilterInterpolationStackLayer()(out, xr, fr, kr, lay.c_base, lay.skip, lay.flow_base, lay.tap_base, detach=True)
    assert r is out and not r.requires_grad
    # an `out` that carries gradient of its own keeps it outside the written slices and loses it inside
    leaf = torch.zeros((B, lay.ctot, AH, AW), device="cuda", requires_grad=True)
    r = FilterInterpolationStackLayer()(leaf * 1.0, xr, fr, kr, lay.c_base, lay.skip, lay.flow_base, lay.tap_base, detach=True)
    (r * weight).sum().backward()
    assert xr.grad is None and fr.grad is None and kr.grad is None
    written = torch.zeros(lay.ctot, dtype=torch.bool, device="cuda")
    for n in range(N):
        written[lay.warp(n)] = written[lay.flow(n)] = written[lay.taps(n)] = True
    assert torch.equal(leaf.grad[:, ~written], weight[:, ~written]) and bool((leaf.grad[:, written] == 0).all())


# ---- the network ---------------------------------------------------------------------------------------------------
def test_memc_net_ve_rectifier_input_is_the_same_by_both_routes():
    """64 x 64, batch 2, named weights.  The flow, the taps and the seven contexts are computed once and handed to both
    routes: MIOpen's fp32 convolutions need not give the same bits twice (README), the routes that assemble the rectifier
    input must.  The final outputs are compared for shape and finiteness only, for the same reason."""
    import networks
    dev = torch.device("cuda", 0)
    net = networks.MEMC_Net_VE(batch=1, channel=3, width=None, height=None, scale_num=1, scale_ratio=2, temporal=False,
                               filter_size=4, save_which=1, debug=False, offset_scale=None, cuda_available=True, cuda_id=None,
                               training=False)
    net.load_state_dict(_netutil.named_weights(net.state_dict()), warn_align_corners=False)
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(31)
    xs = [torch.rand((2, 3, 64, 64), generator=g).to(dev) for _ in range(7)]
    with torch.no_grad():
        flow, taps = net._estimate(xs)
        contexts = [net.ctxNet(x) for x in xs]
        assert net.fused_stack in (True, False)
        net.fused_stack = True
        stacked = net.rectifier_input(xs, flow, taps, contexts)
        assert STK().last_kernel_path() == PATH[3]                       # the frames' call is the second of the two
        net.fused_stack = False
        before = STK().last_kernel_path()
        composed = net.rectifier_input(xs, flow, taps, contexts)
        assert STK().last_kernel_path() == before
        assert stacked.shape == composed.shape == (2, 577, 64, 64)
        assert torch.equal(stacked, composed)
        assert torch.equal(stacked[:, 556 + 9:556 + 12], xs[3]) and torch.equal(stacked[:, 192:256], contexts[3])
        outs = {}
        for fused in (True, False):
            net.fused_stack = fused
            outs[fused] = net(xs)
            assert outs[fused].shape == (2, 3, 64, 64) and bool(torch.isfinite(outs[fused]).all())
        print("max |rectified(stacked) - rectified(composed)| =", float((outs[True] - outs[False]).abs().max()))


def test_memc_net_ve_training_step_by_both_routes():
    """one training step at 64 x 64, batch 1: seven residuals, the same modules with a gradient by both routes, ctxNet's the
    centre frame's alone"""
    import networks
    dev = torch.device("cuda", 0)
    net = networks.MEMC_Net_VE(training=False)
    net.load_state_dict(_netutil.named_weights(net.state_dict()), warn_align_corners=False)
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(32)
    xs = [torch.rand((1, 3, 64, 64), generator=g).to(dev) for _ in range(7)]
    y = torch.rand((1, 3, 64, 64), generator=g).to(dev)
    net.training = True
    l1 = {}
    for fused in (True, False):
        net.zero_grad()
        net.fused_stack = fused
        losses = net(xs, y)
        assert len(losses) == 7 and all(l.shape == y.shape for l in losses)
        sum(l.abs().mean() for l in losses).backward()
        l1[fused] = _netutil.grad_l1_by_module(net)
        assert all(np.isfinite(v) and v > 0 for v in l1[fused].values())
    assert sorted(l1[True]) == sorted(l1[False]) == sorted(["ctxNet", "flownets", "initScaleNets_filter",
                                                            "initScaleNets_filter1", "rectifyNet"])
    for k in l1[True]:                                     # (printed, not compared: the dense layers are not reproducible)
        print(k, l1[True][k], l1[False][k])


# ---- the loop ------------------------------------------------------------------------------------------------------
def test_the_loop_with_gpu_io_writes_the_host_route_s_bytes_and_scores(tmp_path):
    import networks
    import networks.png_io as png
    dev = torch.device("cuda", 0)
    root = str(tmp_path / "vimeo")
    made = SP.write_tree(root, png.write_png)
    runs = {}
    for name, kw in (("host", dict()), ("gpu", dict(gpu_io=True))):
        model = SP.StubEnhancer()
        runs[name] = networks.enhance_septuplet_tree(model, os.path.join(root, "input"), os.path.join(root, "target"),
                                                     str(tmp_path / name), dev, ssim=True, **kw)
        assert model.shapes == [SP.padded_shape(h, w) for _c, h, w in SP.CLIPS]
    assert [r[:3] for r in runs["gpu"]] == [r[:3] for r in runs["host"]]
    for (clip, h, w), g, hst in zip(SP.CLIPS, runs["gpu"], runs["host"]):
        want = SP.expected_centre(made[clip][0])
        for name in runs:
            assert np.array_equal(png.read_png(os.path.join(str(tmp_path / name), clip, "im4.png")), want)
        assert (open(os.path.join(str(tmp_path / "gpu"), clip, "im4.png"), "rb").read()
                == open(os.path.join(str(tmp_path / "host"), clip, "im4.png"), "rb").read())
        assert hst[1:3] == png.rgb_scores(want, made[clip][1])[:2]
        bound = (32 + (h - 6) * (w - 6)) * 2.0 ** -53 + 2.0 ** -52     # tests/test_gpu_ssim.py::tolerance(h, w) + 2^-52
        assert abs(g[3] - hst[3]) <= bound, (g, hst)
    metrics = [open(os.path.join(str(tmp_path / name), "metrics.txt")).read() for name in ("gpu", "host")]
    assert metrics[0] == metrics[1] and metrics[0].startswith("The average interpolation error / PSNR for all images are : ")


def test_the_command_line_tool_runs_the_network_over_a_tree(tmp_path, capsys):
    """tools/demo_vimeo_ve.py on the two 24 x 40 clips of the synthetic tree (padded to 128 x 128): MEMC_Net_VE on its random
    initialisation, both routes of the rectifier input, the pixel work on the device for one of them"""
    import networks.png_io as png
    from tools import demo_vimeo_ve as demo
    root = str(tmp_path / "vimeo")
    SP.write_tree(root, png.write_png)
    listing = str(tmp_path / "sep_testlist.txt")
    clips = [c for c, h, _w in SP.CLIPS if h == 24]
    open(listing, "w").write("".join(c + "\n" for c in clips))
    base = ["--input", os.path.join(root, "input"), "--target", os.path.join(root, "target"), "--list", listing]
    for name, extra in (("stacked", ["--gpu-io", "--ssim"]), ("composed", ["--composed"])):
        out = str(tmp_path / name)
        before = STK().last_kernel_path() if name == "composed" else None
        torch.manual_seed(3)
        demo.main(base + ["--output", out] + extra)
        text = capsys.readouterr().out.strip().split("\n")
        assert len(text) == len(clips) + 1 and text[-1] == open(os.path.join(out, "metrics.txt")).read().rstrip("\n")
        assert text[-1].startswith("The average interpolation error / PSNR for all images are : ")
        assert ("ssim" in text[-1]) == (name == "stacked")
        for c in clips:
            assert png.read_png(os.path.join(out, c, "im4.png")).shape == (24, 40, 3)
        if name == "stacked":
            assert STK().last_kernel_path() == PATH[3]
        else:
            assert STK().last_kernel_path() == before
