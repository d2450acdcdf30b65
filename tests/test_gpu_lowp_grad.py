"""The fp16 / bf16 RGB adaptive-warp backward (libmemc_hip_lp_grad.so, include/memc_warp_lp_grad.h) and its use by the half
autograd Functions.

Contract: for the same inputs, gradinput2 and gradinput3 equal, bit for bit, the fp32 library's (libmemc_hip.so) results
on the widened inputs rounded to their dtype -- with the same gradinput1 choice (NULL or a buffer), which picks the same
summation order for sites that no LDS band covers.  gradinput1 is an fp32 buffer flushed with fp32 atomics on both sides,
so neither side is bit-reproducible from run to run.  Its rule is image_gradients_agree: every finite cell of EITHER side,
before any rounding to T, lies within tests/_image_grad.py's bound of the float64 restatement of the operation on the call's
own inputs -- a bound derived from the kernels' sources (the packed planes' grid, fp32's roundings of the terms and of the
running sums), which holds for every order the hardware may add in and which a dropped or misweighted term of 1e-4 breaks;
after rounding to T the two sides have the same non-finite pattern and are equal on at least 99.9 % of the elements.  "Within
one ulp_T of each other", the earlier rule, follows wherever 2 * bound <= ulp_T (85 - 99 % of the cells:
tests/test_image_grad_bound.py); elsewhere, where terms cancel to a small sum, two correct results may differ by more, and the
bound replaces it.  The fp32 library run twice is held to the rule first (the control)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _image_grad as IG     # noqa: E402
from tools import synth      # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
MANT = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}
SHAPES = [(2, 3, 24, 160), (2, 3, 37, 8), (1, 3, 20, 1280)]


def L():
    import my_package._ext.my_lib_lp_grad as G
    return G


def F():
    import my_package._ext.my_lib as M
    return M


def np_flow(rng, B, H, W, kind):
    if kind == "far":                       # many sites look outside the image or past the LDS bands
        return synth.np_flow(rng, B, H, W, "iid", sigma=0.6 * W)
    return synth.np_flow(rng, B, H, W, kind)


def half_inputs(seed, shape, kind, T, flow_T, gout_T):
    """(x, flow, taps, gout) on the GPU: payloads in T, flow / gout in T or fp32 -- every value representable in T"""
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    x = synth.np_image(rng, B, C, H, W)
    flow = np_flow(rng, B, H, W, kind)
    filt = synth.np_filter(rng, B, H, W)
    gout = rng.standard_normal((B, C, H, W)).astype(np.float32)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dt)      # noqa: E731
    return (dev(x, T), dev(flow, T if flow_T else torch.float32), dev(filt, T),
            dev(gout, T).to(T if gout_T else torch.float32))


def native(x, flow, filt, gout, with_image):
    g1 = torch.zeros(x.shape, dtype=torch.float32, device=x.device) if with_image else None
    g2, g3 = torch.empty_like(flow), torch.empty_like(filt)
    err = L().FilterInterpolationLayer_gpu_backward_lp(x, flow, filt, gout, g1, g2, g3)
    torch.cuda.synchronize()
    return err, g1, g2, g3


def fp32(x, flow, filt, gout, with_image):
    """the fp32 library on the widened inputs"""
    x, flow, filt, gout = (t.float().contiguous() for t in (x, flow, filt, gout))
    g1 = torch.zeros_like(x) if with_image else None
    g2, g3 = torch.empty_like(flow), torch.empty_like(filt)
    assert F().FilterInterpolationLayer_gpu_backward(x, flow, filt, gout, g1, g2, g3) == 0
    torch.cuda.synchronize()
    return g1, g2, g3


def ulp(v, dtype):
    mant, emin = MANT[dtype]
    _, e = torch.frexp(v)
    e = torch.clamp(e - 1, min=emin)
    return torch.ldexp(torch.ones_like(v), e - mant)


TNAME = {torch.float16: "fp16", torch.bfloat16: "bf16"}


def image_reference(flow, taps, gout, fs=4, planes=True):
    """tests/_image_grad.Reference of one call's inputs (tensors of any storage, widened here): made once per call, shared
    by the checks of that call.  planes: the kernels pack the image gradient into LDS planes (C == 3, fs == 4)."""
    return IG.Reference(flow, taps, gout, fs=fs, planes=planes)


def image_gradients_agree(a, b, T, label, inputs, stored=(False, False)):
    """a, b: image gradients of the same call (fp32, or widened from T: then stored[side] is True and the bound gains
    ulp_T / 2).  inputs: image_reference(...) of the call, or its (flow, taps, gradoutput).
    Before rounding: every finite cell of a and of b lies within the derived bound of the float64 restatement.  Rounded to T:
    the same non-finite pattern, equal on at least 99.9 % of the elements.  Cells whose terms are not all finite (an Inf / NaN
    input reaches them) have no bound: there the finite results stay within one ulp_T of each other."""
    ref = inputs if isinstance(inputs, IG.Reference) else image_reference(*inputs)
    ra, rb = a.to(T).float(), b.to(T).float()
    assert torch.equal(torch.isnan(ra), torch.isnan(rb)), label
    fin = torch.isfinite(ra) & torch.isfinite(rb)
    assert torch.equal(ra[~fin & ~torch.isnan(ra)], rb[~fin & ~torch.isnan(rb)]), label      # the infinities
    d = (ra[fin] - rb[fin]).abs()
    tol = ulp(torch.maximum(ra[fin].abs(), rb[fin].abs()), T)
    same = float(((ra == rb) | (torch.isnan(ra) & torch.isnan(rb))).float().mean())
    worst = []
    for side, st in zip((a, b), stored):
        r, _ok = ref.ratio(side.detach().float().cpu().numpy(), TNAME[T] if st else None)
        worst.append(float(r.max()))
    print("%s: max diff %.3g ulp_T, equal %.6f, max err / bound %.3f and %.3f (bound up to %.3g)"
          % (label, float((d / tol).max()) if d.numel() else 0.0, same, worst[0], worst[1],
             float(np.nanmax(np.where(ref.finite, ref.bound(), 0.0)))))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (label, worst)
    loose = torch.from_numpy(~ref.finite).to(fin.device) & fin                   # no bound: today's treatment
    dl = (ra[loose] - rb[loose]).abs()
    assert bool((dl <= ulp(torch.maximum(ra[loose].abs(), rb[loose].abs()), T)).all()), label
    assert same >= 0.999, (label, same)


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("flow_T", [False, True], ids=["flowF32", "flowT"])
@pytest.mark.parametrize("gout_T", [True, False], ids=["goutT", "goutF32"])
@pytest.mark.parametrize("kind", ["smooth", "iid", "far"])
@pytest.mark.parametrize("with_image", [True, False], ids=["image", "noimage"])
def test_flow_and_tap_gradients_are_the_fp32_ones_rounded(tname, flow_T, gout_T, kind, with_image):
    T = DTYPES[tname]
    for i, shape in enumerate(SHAPES):
        x, flow, filt, gout = half_inputs(100 + i, shape, kind, T, flow_T, gout_T)
        err, g1, g2, g3 = native(x, flow, filt, gout, with_image)
        assert err == 0, shape
        assert L().last_kernel_path() == ("fi_bwd_lp:tiled_c3" if with_image else "fi_bwd_lp:tiled_c3_noimage")
        w1, w2, w3 = fp32(x, flow, filt, gout, with_image)
        assert g2.dtype == flow.dtype and g3.dtype == T
        assert torch.equal(g2, w2.to(flow.dtype)), ("flow gradient", shape)
        assert torch.equal(g3, w3.to(T)), ("tap gradient", shape)


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("kind", ["smooth", "iid", "far"])
def test_image_gradient_matches_the_fp32_library(tname, kind):
    T = DTYPES[tname]
    for i, shape in enumerate(SHAPES):
        x, flow, filt, gout = half_inputs(200 + i, shape, kind, T, False, True)
        ref = image_reference(flow, filt, gout)
        a1, _, _ = fp32(x, flow, filt, gout, True)
        b1, _, _ = fp32(x, flow, filt, gout, True)
        image_gradients_agree(a1, b1, T, "control: fp32 twice %s %s" % (kind, shape), ref)
        err, g1, _, _ = native(x, flow, filt, gout, True)
        assert err == 0 and g1.dtype == torch.float32
        image_gradients_agree(g1, a1, T, "native vs fp32 %s %s" % (kind, shape), ref)


@pytest.mark.parametrize("tname", sorted(DTYPES))
def test_half_gradients_match_the_oracle(tname, oracle):
    """Independent of the fp32 library: the CPU oracle on the widened inputs.  Bound: tests/_parity.py's rule (1e-4
    absolute up to |want| = 10, 1e-5 relative beyond) plus half an ulp_T for the single rounding to T."""
    T = DTYPES[tname]
    for kind in ("smooth", "iid", "far"):
        x, flow, filt, gout = half_inputs(300, (2, 3, 24, 160), kind, T, False, True)
        err, g1, g2, g3 = native(x, flow, filt, gout, True)
        assert err == 0
        want = oracle.filter_interpolation_backward(*(t.float().cpu().numpy() for t in (x, flow, filt, gout)))
        for got, w, name in zip((g1.to(T), g2, g3), want, ("image", "flow", "taps")):
            w = torch.from_numpy(np.asarray(w)).float()
            g = got.float().cpu()
            bound = torch.where(w.abs() <= 10, torch.full_like(w, 1e-4), torch.clamp(1e-5 * w.abs(), min=1e-4))
            if got.dtype != torch.float32:
                bound = bound + 0.5 * ulp(w, got.dtype)
            e = (g - w).abs()
            print("oracle %s %s %s: max err %.3g" % (tname, kind, name, float(e.max())))
            assert bool((e <= bound).all()), (kind, name, float(e.max()))


@pytest.mark.parametrize("tname", sorted(DTYPES))
def test_aligned_views_are_served_and_shifted_ones_declined(tname):
    T = DTYPES[tname]
    B, H, W, pad = 2, 16, 64, 8
    x, flow, filt, gout = half_inputs(400, (B, 3, H, W), "iid", T, False, True)

    def padded(t, extra_c, fill, shift):
        """t as a channel slice (channels 1..) of a row-padded buffer; `shift` elements further right"""
        big = torch.full((t.size(0), t.size(1) + extra_c, H, W + pad), fill, dtype=t.dtype, device=t.device)
        v = big[:, 1:1 + t.size(1), :, shift:shift + W]
        v.copy_(t)
        return big, v

    for shift, served in ((0, True), (1, False)):
        nan = float("nan")
        _, vx = padded(x, 2, 0.0, shift)
        _, vf = padded(flow, 2, 0.0, shift)
        _, vk = padded(filt, 2, 0.0, shift)
        _, vg = padded(gout, 2, 0.0, shift)
        b1, v1 = padded(torch.zeros_like(x, dtype=torch.float32), 2, nan, shift)
        b2, v2 = padded(torch.full_like(flow, nan), 2, nan, shift)
        b3, v3 = padded(torch.full_like(filt, nan), 2, nan, shift)
        assert vx.stride() == v1.stride() and vk.stride() == v3.stride()
        inside = [torch.zeros_like(b, dtype=torch.bool) for b in (b1, b2, b3)]
        for m, c in zip(inside, (3, 2, 16)):
            m[:, 1:1 + c, :, shift:shift + W] = True
        err = L().FilterInterpolationLayer_gpu_backward_lp(vx, vf, vk, vg, v1, v2, v3)
        torch.cuda.synchronize()
        assert err == (0 if served else 1), (shift, err)
        for b, m in zip((b1, b2, b3), inside):
            assert bool(torch.isnan(b[~m]).all()), "a sentinel around the view was written"
        if served:
            w1, w2, w3 = fp32(vx, vf, vk, vg, True)
            assert torch.equal(v2, w2) and torch.equal(v3, w3.to(T))
            image_gradients_agree(v1.contiguous(), w1, T, "view", (vf, vk, vg))
        else:                                                 # nothing touched
            assert bool((v1 == 0).all()) and bool(torch.isnan(v2).all()) and bool(torch.isnan(v3).all())


def test_fp16_overflow_and_infinite_gradoutput():
    T = torch.float16
    x, flow, filt, gout = half_inputs(500, (2, 3, 24, 160), "smooth", T, False, True)
    big = torch.full_like(gout, 6e4)                          # tap gradients (~ weight x 6e4 x the pixel sum) beyond 65504 in places
    for with_image in (True, False):
        err, g1, g2, g3 = native(x, flow, filt, big, with_image)
        assert err == 0
        w1, w2, w3 = fp32(x, flow, filt, big, with_image)
        w3T = w3.to(T)
        assert bool(torch.isinf(w3T).any()) and bool(torch.isfinite(w3T).any())
        assert torch.equal(torch.isinf(g3), torch.isinf(w3T)) and torch.equal(g3, w3T)
        assert torch.equal(g2, w2)
    # one infinite gradoutput value: the fp32 path's non-finite pattern, after rounding
    inf = gout.clone()
    inf[1, 1, 9, 77] = float("inf")
    for with_image in (True, False):
        err, g1, g2, g3 = native(x, flow, filt, inf, with_image)
        assert err == 0
        w1, w2, w3 = fp32(x, flow, filt, inf, with_image)
        for got, want in ((g2, w2), (g3, w3.to(T))):
            assert torch.equal(torch.isnan(got), torch.isnan(want))
            assert bool(torch.isnan(want).any()) or bool(torch.isinf(want).any())
            ok = ~torch.isnan(want)
            assert torch.equal(got[ok], want[ok])
        if with_image:
            image_gradients_agree(g1, w1, T, "inf gradoutput", (flow, filt, inf))


def device_inputs(seed, shape, T):
    """large inputs drawn on the GPU: image in [0, 1), flow of a few pixels, taps summing to about one, gradoutput N(0, 1)"""
    B, C, H, W = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand((B, C, H, W), generator=g, device="cuda").to(T)
    flow = (3.0 * torch.randn((B, 2, H, W), generator=g, device="cuda"))
    filt = (torch.rand((B, 16, H, W), generator=g, device="cuda") / 8.0).to(T)
    gout = torch.randn((B, C, H, W), generator=g, device="cuda").to(T)
    return x, flow, filt, gout


def test_large_shapes():
    """Once each: 720p batch 32 bf16 without the image gradient, BASELINE config 2's shape fp16 with it."""
    for shape, T, with_image in (((32, 3, 720, 1280), torch.bfloat16, False), ((8, 3, 256, 448), torch.float16, True)):
        x, flow, filt, gout = device_inputs(600, shape, T)
        err, g1, g2, g3 = native(x, flow, filt, gout, with_image)
        assert err == 0
        w1, w2, w3 = fp32(x, flow, filt, gout, with_image)
        assert torch.equal(g2, w2), shape
        assert torch.equal(g3, w3.to(T)), shape
        if with_image:
            image_gradients_agree(g1, w1, T, "config 2", (flow, filt, gout))
        del x, flow, filt, gout, g1, g2, g3, w1, w2, w3
        torch.cuda.empty_cache()


@pytest.fixture
def native_calls(monkeypatch):
    G = L()
    calls = []
    real = G.FilterInterpolationLayer_gpu_backward_lp

    def counted(*args):
        r = real(*args)
        calls.append((r, G.last_kernel_path()))
        return r

    monkeypatch.setattr(G, "FilterInterpolationLayer_gpu_backward_lp", counted)
    return calls


def _layer_grads(T, shape, fs, image_grad, seed=700):
    """gradients of the half layer and of the fp32 layer on the widened inputs, rounded; the inputs (flow, taps, gradoutput) in T"""
    from my_package.modules.FilterInterpolationModule import FilterInterpolationModule
    B, C, H, W = shape
    rng = np.random.default_rng(seed)
    arrs = (synth.np_image(rng, B, C, H, W), synth.np_flow(rng, B, H, W, "smooth"), synth.np_filter(rng, B, H, W, fs=fs))
    gout = torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32)).cuda().to(T)

    def run(dt):
        ts = [torch.from_numpy(a).cuda().to(T).to(dt) for a in arrs]
        for i, t in enumerate(ts):
            t.requires_grad_(image_grad or i > 0)
        FilterInterpolationModule()(*ts).backward(gout.to(dt))
        return [t.grad for t in ts]

    held = tuple(torch.from_numpy(a).cuda().to(T) for a in arrs[1:]) + (gout,)
    return run(T), run(torch.float32), held


@pytest.mark.parametrize("tname", sorted(DTYPES))
def test_routing(tname, native_calls):
    from my_package.modules.FilterInterpolationBlendModule import FilterInterpolationBlendModule
    T = DTYPES[tname]
    # covered: the native entry, with and without the image gradient
    for image_grad, path in ((True, "fi_bwd_lp:tiled_c3"), (False, "fi_bwd_lp:tiled_c3_noimage")):
        del native_calls[:]
        lo, hi, _ = _layer_grads(T, (2, 3, 24, 160), 4, image_grad)
        assert native_calls == [(0, path)], native_calls
        for g_lo, g_hi in zip(lo, hi):
            assert (g_lo is None) == (g_hi is None) and (g_lo is None or torch.equal(g_lo, g_hi.to(T)))
    # not covered: C = 4, W = 157, fs = 2 -- the widened path, untouched by the native entry (its image gradient is summed
    # in an order the hardware picks: held to the condition of test_image_gradient_matches_the_fp32_library, with half an
    # ulp_T more for the half layer's gradient, which is stored in T; only the RGB fs == 4 kernel has planes)
    for shape, fs in (((2, 4, 24, 160), 4), ((2, 3, 24, 157), 4), ((2, 3, 24, 160), 2)):
        del native_calls[:]
        lo, hi, held = _layer_grads(T, shape, fs, True)
        assert native_calls == [], (shape, fs, native_calls)
        image_gradients_agree(lo[0].float(), hi[0], T, "widened %s fs %d" % (shape, fs),
                              image_reference(*held, fs=fs, planes=shape[1] == 3 and fs == 4), stored=(True, False))
        for g_lo, g_hi in zip(lo[1:], hi[1:]):
            assert torch.equal(g_lo, g_hi.to(T)), (shape, fs)
    # the blend: both directions' backward launches (with the image gradient, as the float32 blend computes it)
    del native_calls[:]
    B, H, W = 2, 24, 160
    rng = np.random.default_rng(710)
    x0, x2 = synth.np_image(rng, B, 3, H, W), synth.np_image(rng, B, 3, H, W)
    f0, f1 = synth.np_flow(rng, B, H, W, "smooth"), synth.np_flow(rng, B, H, W, "iid")
    k0, k1 = synth.np_filter(rng, B, H, W), synth.np_filter(rng, B, H, W)
    o0 = rng.random((B, 1, H, W), dtype=np.float32)
    ts = [torch.from_numpy(a).cuda().to(T).requires_grad_(True)
          for a in (x0, x2, f0, f1, k0, k1, o0, (1 - o0).astype(np.float32))]
    FilterInterpolationBlendModule()(*ts).backward(torch.ones(B, 3, H, W, device="cuda", dtype=T))
    assert native_calls == [(0, "fi_bwd_lp:tiled_c3")] * 2, native_calls


def test_bf16_training_step_uses_the_native_backward(native_calls):
    import _netutil
    _netutil.purge_networks()
    import networks
    m = networks.MEMC_Net_star(channel=3, filter_size=4, training=True)
    m.load_state_dict(_netutil.named_weights(m.state_dict()), strict=True)
    m = m.cuda().to(torch.bfloat16).train()
    x = _netutil.training_frames(5, 1, 128, 128).cuda().to(torch.bfloat16)
    losses, _f, _k, _o = m(x)
    total = sum(l.float().abs().mean() for l in losses)
    total.backward()
    torch.cuda.synchronize()
    assert len(native_calls) >= 2 and all(r == 0 for r, _ in native_calls), native_calls
    grads = [(n, p.grad) for n, p in m.named_parameters() if p.grad is not None]
    assert grads
    bad = [n for n, g in grads if not bool(torch.isfinite(g.float()).all())]
    assert not bad, bad
