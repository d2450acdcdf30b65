"""The SPyNet level backward kernel (libmemc_hip_spynet_grad.so, my_lib_spynet_grad, SpyNetLevelLayer.native_backward) on
the device.

Shapes (tests/_spynet_grad_spec.SHAPES): those of tests/test_gpu_spynet_level.py, then 2 x 3 and 3 x 2 (h or w equal to 1
with a padded column or row) and 37 x 70 (a coarse grid of 18 x 35: two tiles of 16 down and three across, a padded row, a
width that is no multiple of four); each under the flag pairs (0, 0), (1, 1), (0, 1) with a coarse flow N(0, 4^2) (the
first admissible draw), zero (align_sample = 1 only) and a pan of 1e9 in x; gradoutput N(0, 1) / 4.

The rule: gradcoarse, written into a NaN-filled tensor, is within tests/_parity.close of `level_grad` in float64 evaluated
on the KERNEL'S OWN `up` (from a forward call on the same inputs: under align_upsample the fp32 upsampling weights move `up`
by about 2e-5, which the warp's second derivative turns into gradient differences of up to 6e-4 through no fault of the
backward).  Torch's own float32 autograd against float64 on the same `up` is 2.5e-5 off at worst on these shapes with this
gradoutput (max |want| about 10); at 64 x 96 it exceeds the rule, so the cases stay below 64.  On the exact cases the result
equals the float64 rule bit for bit.  Observed errors go to the parity log as the other parity tests' do.
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

import _netutil                            # noqa: E402
import _parity                             # noqa: E402
import _spynet_spec as S                   # noqa: E402
import _spynet_grad_spec as SG             # noqa: E402

pytestmark = pytest.mark.gpu
PATH = "spynet_level_bwd:tiled"


def FWD():
    import my_package._ext.my_lib_spynet as M
    return M


def BWD():
    import my_package._ext.my_lib_spynet_grad as M
    return M


def layer(flags, native=True):
    from my_package.functions.SpyNetLevelLayer import SpyNetLevelLayer
    f = SpyNetLevelLayer(*flags)
    f.native_backward = native                 # the instance's own: the class attribute stays False
    return f


def D(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def own_up(second, coarse, flags):
    """the forward kernel's `up` on these inputs, as numpy"""
    s, c = D(second), D(coarse)
    out = torch.empty((s.size(0), 8, s.size(2), s.size(3)), device="cuda")
    assert FWD().SpyNetLevelLayer_gpu_forward(torch.zeros_like(s), s, c, out, *flags) == 0
    return out[:, 6:8].cpu().numpy()


def run(second, coarse, G, flags, fill=float("nan")):
    """the entry point on a NaN-filled gradcoarse: the result as numpy"""
    s, c, g = D(second), D(coarse), D(G)
    gc = torch.full(c.shape, fill, device="cuda")
    assert BWD().SpyNetLevelLayer_gpu_backward(s, c, g, gc, *flags) == 0
    assert BWD().last_kernel_path() == PATH
    torch.cuda.synchronize()
    return gc.cpu().numpy()


@pytest.mark.parametrize("flags", SG.FLAGS)
@pytest.mark.parametrize("shape", SG.SHAPES)
def test_gradient_against_the_float64_rule(shape, flags):
    for flow in SG.flows(flags):
        second, coarse, G, _attempt = SG.ordinary_case(shape, flags, flow)
        got = run(second, coarse, G, flags)
        assert not np.isnan(got).any(), "an element of gradcoarse was not written"
        up = own_up(second, coarse, flags)
        want = SG.level_grad(second, coarse, G, flags, np.float64, up=up)
        what = "%s %s %s" % (shape, flags, flow)
        err = _parity.close(got.astype(np.float64), want, what + ": gradcoarse vs the float64 rule on the kernel's own up")
        print(what, "worst error %.3g, max |want| %.3g" % (err, float(np.abs(want).max())))
        if flow == "pan":
            # every warp term is 0: the pure adjoint of the upsampling of G[6:8] -- the rule's, and torch's float64 one
            h, w = coarse.shape[2:]
            assert np.array_equal(want, SG.upsample_adjoint(G[:, 6:8].astype(np.float64), h, w, flags[0], np.float64))
            g = torch.from_numpy(G[:, 6:8].copy()).double()
            c = torch.zeros(coarse.shape, dtype=torch.float64, requires_grad=True)
            t = torch.nn.functional.interpolate(c, scale_factor=2, mode="bilinear", align_corners=bool(flags[0])) * 2.0
            t = torch.nn.functional.pad(t, [0, shape[2] - t.size(3), 0, shape[1] - t.size(2)], "replicate")
            adj = torch.autograd.grad(t, c, g)[0].numpy()
            _parity.close(got.astype(np.float64), adj, what + ": gradcoarse vs torch's float64 adjoint of interpolate + pad")


@pytest.mark.parametrize("shape", SG.SHAPES)
def test_exact_cases_bit_for_bit(shape):
    second, coarse, G = SG.exact_case(shape)
    got = run(second, coarse, G, SG.EXACT_FLAGS)
    want = SG.level_grad(second, coarse, G, SG.EXACT_FLAGS, np.float64)
    assert np.array_equal(own_up(second, coarse, SG.EXACT_FLAGS).astype(np.float64),
                          S.upsampled(coarse, shape[1], shape[2], SG.EXACT_FLAGS[0], np.float64))
    _parity.exact(got.astype(np.float64), want, "exact %s: gradcoarse" % (shape,))
    assert np.array_equal(got.astype(np.float64), want)


def test_two_calls_give_the_same_bits():
    for shape, flags in (((1, 37, 70), (1, 1)), ((2, 25, 40), (0, 0))):
        second, coarse, G, _a = SG.ordinary_case(shape, flags)
        s, c, g = D(second), D(coarse), D(G)
        a, b = torch.full_like(c, float("nan")), torch.full_like(c, float("nan"))
        assert BWD().SpyNetLevelLayer_gpu_backward(s, c, g, a, *flags) == 0
        assert BWD().SpyNetLevelLayer_gpu_backward(s, c, g, b, *flags) == 0
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize("shape", [(2, 25, 40), (1, 37, 70)])
def test_padded_stride_views_give_the_contiguous_call_s_bits(shape):
    B, H, W = shape
    h, w = H // 2, W // 2
    for flags in SG.FLAGS:
        second, coarse, G, _a = SG.ordinary_case(shape, flags)
        s, c, g = D(second), D(coarse), D(G)
        want = torch.full_like(c, float("nan"))
        assert BWD().SpyNetLevelLayer_gpu_backward(s, c, g, want, *flags) == 0
        wide_s = torch.full((B, 3, H + 2, W + 5), -7.0, device="cuda")
        wide_c = torch.full((B, 3, h + 1, w + 3), 5.0, device="cuda")
        wide_g = torch.full((B, 11, H + 1, W + 2), 3.0, device="cuda")         # gradoutput: a channel slice of a wider tensor
        wide_q = torch.full((B, 4, h + 3, w + 2), 9.0, device="cuda")
        vs, vc = wide_s[:, :, 1:H + 1, 3:W + 3], wide_c[:, 1:3, :h, 2:w + 2]
        vg, vq = wide_g[:, 2:10, 1:, :W], wide_q[:, 1:3, 2:h + 2, 1:w + 1]
        vs.copy_(s), vc.copy_(c), vg.copy_(g)
        for v in (vs, vc, vg, vq):
            assert not v.is_contiguous() and v.stride(3) == 1
        assert BWD().SpyNetLevelLayer_gpu_backward(vs, vc, vg, vq, *flags) == 0
        assert BWD().last_kernel_path() == PATH
        assert torch.equal(vq, want)
        # the surroundings: untouched
        ring = wide_q.clone()
        ring[:, 1:3, 2:h + 2, 1:w + 1] = 9.0
        assert bool((ring == 9.0).all())
        assert torch.equal(vs, s) and torch.equal(vc, c) and torch.equal(vg, g)
        assert float(wide_s[:, :, 0].max()) == -7.0 and float(wide_c[:, 0].min()) == 5.0 and float(wide_g[:, 0].min()) == 3.0


def test_autograd_through_the_layer(monkeypatch):
    from my_package.functions.SpyNetLevelLayer import SpyNetLevelLayer
    assert SpyNetLevelLayer.native_backward is False
    calls = []
    entry = BWD().SpyNetLevelLayer_gpu_backward

    def recording(second, coarse, gradoutput, gradcoarse, *flags):
        err = entry(second, coarse, gradoutput, gradcoarse, *flags)
        # the path string is the calling thread's, and autograd's backward runs on a thread of its own: read it there
        calls.append((tuple(second.shape[2:]), gradoutput.stride(), flags, BWD().last_kernel_path()))
        return err
    monkeypatch.setattr(BWD(), "SpyNetLevelLayer_gpu_backward", recording)
    for shape, flags in (((2, 25, 40), (0, 0)), ((1, 37, 70), (1, 1)), ((1, 6, 5), (0, 1))):
        second, coarse, G, _a = SG.ordinary_case(shape, flags)
        first = D(S.ordinary_case(shape)[0]).requires_grad_(True)
        s, c, g = D(second), D(coarse).requires_grad_(True), D(G)
        want = torch.full_like(c, float("nan"))
        assert entry(s, c.detach(), g, want, *flags) == 0
        out = layer(flags)(first, s, c)
        assert FWD().last_kernel_path() == S.family(shape[2])                  # the forward is the forward kernel's call
        assert "SpyNetLevelFunction" in type(out.grad_fn).__name__
        with torch.no_grad():
            assert torch.equal(out, layer(flags)(first, s, c))
        n = len(calls)
        out.backward(g)
        assert len(calls) == n + 1 and calls[-1][0] == shape[1:] and calls[-1][2] == tuple(bool(f) for f in flags)
        assert calls[-1][3] == PATH
        assert torch.equal(c.grad, want)
        assert torch.equal(first.grad, g[:, 0:3]) and s.grad is None
        # an expanded gradoutput (sum().backward()): made contiguous before the call
        c2 = D(coarse).requires_grad_(True)
        layer(flags)(first.detach(), s, c2).sum().backward()
        assert len(calls) == n + 2 and calls[-1][1][3] == 1
        ones = torch.full_like(c, float("nan"))
        assert entry(s, c.detach(), torch.ones_like(g), ones, *flags) == 0
        assert torch.equal(c2.grad, ones)
    # `second` wanting a gradient, or native_backward = False: torch's autograd, the binding is not reached
    shape, flags = (2, 25, 40), (0, 0)
    second, coarse, G, _a = SG.ordinary_case(shape, flags)
    first, g = D(S.ordinary_case(shape)[0]), D(G)
    n = len(calls)
    for native, second_wants in ((True, True), (False, False), (False, True)):
        s, c = D(second).requires_grad_(second_wants), D(coarse).requires_grad_(True)
        out = layer(flags, native)(first, s, c)
        assert "SpyNetLevelFunction" not in type(out.grad_fn).__name__
        out.backward(g)
        assert c.grad is not None and bool(torch.isfinite(c.grad).all()) and (s.grad is not None) == second_wants
    # and so do a layer with `fused` off, autocast and no_grad
    off = layer(flags)
    off.fused = False
    c = D(coarse).requires_grad_(True)
    off(first, D(second), c).backward(g)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        c = D(coarse).requires_grad_(True)
        assert "SpyNetLevelFunction" not in type(layer(flags)(first, D(second), c).grad_fn).__name__
    with torch.no_grad():
        assert layer(flags)(first, D(second), D(coarse).requires_grad_(True)).grad_fn is None
    assert len(calls) == n
    assert SpyNetLevelLayer.native_backward is False


def test_a_declined_backward_takes_torch_s_gradient():
    """a gradoutput whose ROW stride is beyond what the library takes cannot be built cheaply; a `second` with a w-stride of
    2 can: both libraries decline, the Function composes forward and backward"""
    shape, flags = (2, 24, 40), (0, 0)
    second, coarse, G, _a = SG.ordinary_case(shape, flags)
    first, g = D(S.ordinary_case(shape)[0]), D(G)
    wide = torch.zeros((2, 3, 24, 80), device="cuda")
    wide[..., ::2] = D(second)
    gc = torch.empty((2, 2, 12, 20), device="cuda")
    assert BWD().SpyNetLevelLayer_gpu_backward(wide[..., ::2], D(coarse), g, gc, *flags) == 1
    assert BWD().SpyNetLevelLayer_gpu_backward(D(second), g[:, 6:8, :12, :20], g, g[:, 0:2, :12, :20], *flags) == 1   # over an input
    c = D(coarse).requires_grad_(True)
    out = layer(flags)(first, wide[..., ::2], c)
    assert "SpyNetLevelFunction" in type(out.grad_fn).__name__
    out.backward(g)
    want = torch.full_like(gc, float("nan"))
    assert BWD().SpyNetLevelLayer_gpu_backward(D(second), D(coarse), g, want, *flags) == 0
    torch.cuda.synchronize()
    _parity.close(c.grad, want, "declined backward: torch's gradient vs the kernel's on the contiguous call")


def test_non_finite_flows_stay_inside_second():
    """NaN, +-inf and huge coarse flows at a few cells: the call returns 0 and the program runs on; every coarse cell whose
    candidate sites (footprint) hold no affected site -- a site whose `up` is not what it is without them -- has the clean
    call's bits"""
    shape = (1, 37, 70)
    H, W = shape[1:]
    h, w = H // 2, W // 2
    for flags in SG.FLAGS:
        second, coarse, G, _a = SG.ordinary_case(shape, flags)
        bad = coarse.copy()
        bad[0, 0, 2, 3], bad[0, 1, 5, 7], bad[0, 0, 15, 16], bad[0, 1, 17, 34], bad[0, 0, 9, 1] = np.nan, np.inf, -np.inf, 3e38, -3e38
        want = run(second, coarse, G, flags)
        got = run(second, bad, G, flags, fill=0.0)
        affected = (own_up(second, bad, flags) != own_up(second, coarse, flags)).any(axis=1)[0]         # [H, W]
        ylo, yhi = SG.footprint(np.arange(h), h, H, flags[0])
        xlo, xhi = SG.footprint(np.arange(w), w, W, flags[0])
        clean = np.array([[not affected[ylo[i]:yhi[i] + 1, xlo[j]:xhi[j] + 1].any() for j in range(w)] for i in range(h)])
        assert 0 < clean.sum() < clean.size
        assert np.array_equal(got[0][:, clean], want[0][:, clean])
        assert not np.array_equal(got, want, equal_nan=True)
    torch.cuda.synchronize()                   # the program runs on
    assert float(torch.ones(4, device="cuda").sum()) == 4.0


def test_one_training_step_of_memc_net_s(monkeypatch):
    """MEMC_Net_s at 64 x 64, batch 2, with `fused_level_backward = True`: the 64 x 64 levels reach both bindings, in both
    directions; every parameter of the two used stacks has a finite non-zero gradient; the per-module gradient L1 agrees
    with a flag-off step within the larger of 1e-4 relative (the project's rule for this quantity, tests/test_network_s.py)
    and four times the relative difference of two flag-off steps on the same input (the parent route's own spread: MIOpen's
    convolutions do not repeat bits)."""
    import networks
    B, H, W = 2, 64, 64
    net = networks.MEMC_Net_s(channel=3, filter_size=4, training=False).eval()
    net.load_state_dict(_netutil.named_weights(net.state_dict()), strict=True, warn_align_corners=False)
    net = net.cuda()
    assert net.flownets.fused_level_backward is False
    x3 = _netutil.training_frames(33, B, H, W).cuda()
    fwd_calls, bwd_calls = [], []
    fwd_entry, bwd_entry = FWD().SpyNetLevelLayer_gpu_forward, BWD().SpyNetLevelLayer_gpu_backward

    def rec_fwd(first, second, coarse, out, *flags):
        fwd_calls.append(tuple(first.shape[2:]))
        return fwd_entry(first, second, coarse, out, *flags)

    def rec_bwd(second, coarse, gradoutput, gradcoarse, *flags):
        err = bwd_entry(second, coarse, gradoutput, gradcoarse, *flags)
        bwd_calls.append((tuple(second.shape[2:]), BWD().last_kernel_path()))      # the path of the thread that called
        return err
    monkeypatch.setattr(FWD(), "SpyNetLevelLayer_gpu_forward", rec_fwd)
    monkeypatch.setattr(BWD(), "SpyNetLevelLayer_gpu_backward", rec_bwd)

    def step(flag):
        net.zero_grad()
        net.flownets.fused_level_backward = flag
        del fwd_calls[:], bwd_calls[:]
        net.training = True                    # the class's own flag; the sub-modules stay in eval mode
        try:
            losses, _flows, _filters, _occl = net(x3)
            total = sum(l.abs().mean() for l in losses)
            total.backward()
        finally:
            net.training = False
        assert bool(torch.isfinite(total))
        return _netutil.grad_l1_by_module(net), sorted(fwd_calls), sorted(bwd_calls)

    off_a, fwd_off, bwd_off = step(False)
    off_b, _f, _b = step(False)
    # the parent route: the coarsest levels alone reach the forward binding, nothing reaches the backward one
    assert fwd_off == [(32, 32)] * 2 and bwd_off == []
    on, fwd_on, bwd_on = step(True)
    assert fwd_on == [(32, 32)] * 2 + [(64, 64)] * 2, fwd_on
    assert bwd_on == [((64, 64), PATH)] * 2, bwd_on
    for level, stack in enumerate(net.flownets.moduleBasic):
        for name, p in stack.named_parameters():
            if level < 2:
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, (level, name)
            else:
                assert p.grad is None, (level, name)
    assert sorted(on) == sorted(off_a) == sorted(off_b)
    for k in sorted(on):
        spread = abs(off_a[k] - off_b[k]) / off_a[k]
        diff = abs(on[k] - off_a[k]) / off_a[k]
        bound = max(1e-4, 4.0 * spread)
        print("%-24s grad L1 off %.9g, on %.9g: relative difference %.3g; two flag-off steps differ by %.3g; bound %.3g" % (
            k, off_a[k], on[k], diff, spread, bound))
        assert np.isfinite(on[k]) and on[k] > 0 and diff <= bound, k
    net.zero_grad()
