"""fp16 / bf16 adaptive warps (libmemc_hip_lp.so through my_package) against the fp32 oracle on the widened inputs.

Inputs are seeded tools/synth arrays rounded to T; the oracle (oracle/memc_oracle, fp32) runs on the widened values.  Per
element |got - want| <= ulp_T(want) / 2 + 2e-5 * max(1, |want|) (one rounding of an fp32 result that may differ from the
oracle's in its last bits: fused multiply-adds), and at least 99 % of the elements equal want.to(T) exactly (the observed
fraction is printed)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tools import synth      # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
MANT = {torch.float16: (10, -14), torch.bfloat16: (7, -126)}


def np_flow(rng, B, H, W, kind):
    if kind == "far":                       # a large share of the sites looks outside the image or past |flow| < W/2
        return synth.np_flow(rng, B, H, W, "iid", sigma=0.6 * W)
    return synth.np_flow(rng, B, H, W, kind)


def to_dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)


def ulp(want, dtype):
    mant, emin = MANT[dtype]
    _, e = torch.frexp(want)                                   # |want| in [2^(e-1), 2^e)
    e = torch.clamp(e - 1, min=emin)
    return torch.ldexp(torch.ones_like(want), e - mant)


def check(got, want, dtype, label):
    """got: T tensor (any device), want: fp32 numpy / tensor of the same shape"""
    got = got.detach().float().cpu()
    want = torch.as_tensor(want).float()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isinf(got) & ~fin, torch.isinf(want) & ~fin), label
    g, w = got[fin], want[fin]
    tol = 0.5 * ulp(w, dtype) + 2e-5 * torch.clamp(w.abs(), min=1.0)
    err = (g - w).abs()
    assert bool((err <= tol).all()), "%s: max err %g (tol there %g)" % (label, float(err.max()), float(tol[err.argmax()]))
    exact = float((got == want.to(dtype).float()).float().mean())
    print("%s: exact %.5f" % (label, exact))
    assert exact >= 0.99, (label, exact)
    return exact


def fi(x, flow, filt):
    from my_package.modules.FilterInterpolationModule import FilterInterpolationModule
    with torch.no_grad():
        return FilterInterpolationModule()(x, flow, filt)


def last_path():
    import my_package._ext.my_lib_lp as L
    return L.last_kernel_path()


def inputs(seed, B, C, H, W, kind, fs=4):
    rng = np.random.default_rng(seed)
    return (synth.np_image(rng, B, C, H, W), np_flow(rng, B, H, W, kind), synth.np_filter(rng, B, H, W, fs=fs))


def widened(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).float().numpy()


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("flow_t", ["fp32", "T"])
@pytest.mark.parametrize("kind", ["smooth", "iid", "far"])
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 64])
def test_forward_matches_oracle(oracle, tname, flow_t, kind, C):
    T = DTYPES[tname]
    FT = T if flow_t == "T" else torch.float32
    B, H, W = 2, 24, 160
    x, flow, filt = inputs(11 + C, B, C, H, W, kind)
    xw, fw, kw = widened(x, T), widened(flow, FT), widened(filt, T)
    got = fi(to_dev(xw, T), to_dev(fw, FT), to_dev(kw, T))
    assert got.dtype == T
    assert last_path() == ("fi_fwd_lp:tiled_c3" if C == 3 else "fi_fwd_lp:tiled_c4n")
    check(got, oracle.filter_interpolation_forward(xw, fw, kw), T, "fi %s flow %s %s C%d" % (tname, flow_t, kind, C))


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("W", [6, 157, 160])
@pytest.mark.parametrize("fs", [2, 4])
def test_forward_widths_and_filter_sizes(oracle, tname, W, fs):
    T = DTYPES[tname]
    x, flow, filt = inputs(5 + W + fs, 2, 3, 20, W, "smooth", fs=fs)
    xw, fw, kw = widened(x, T), widened(flow, T), widened(filt, T)
    got = fi(to_dev(xw, T), to_dev(fw, T), to_dev(kw, T))
    tiled = fs == 4 and W % 4 == 0 and W >= 8
    assert last_path() == ("fi_fwd_lp:tiled_c3" if tiled else "fi_fwd_lp:direct")
    check(got, oracle.filter_interpolation_forward(xw, fw, kw), T, "fi %s W%d fs%d" % (tname, W, fs))


@pytest.mark.parametrize("tname", sorted(DTYPES))
def test_strided_channel_sliced_views(oracle, tname):
    """Views straight through the C ABI: an aligned channel slice of a row-padded tensor (tiled) and the same slice
    shifted by one element (8-byte quads no longer aligned: direct)."""
    import my_package._ext.my_lib_lp as L
    T = DTYPES[tname]
    B, H, W = 2, 20, 160
    x, flow, filt = inputs(77, B, 6, H, W + 8, "smooth")
    xw, fw, kw = widened(x, T), widened(flow, torch.float32), widened(filt, T)
    base, fl, k = to_dev(xw, T), to_dev(fw, torch.float32), to_dev(kw, T)
    for shift, path in ((0, "fi_fwd_lp:tiled_c3"), (1, "fi_fwd_lp:direct")):
        xv = base[:, 1:4, :, shift:shift + W]
        flv, kv = fl[:, :, :, shift:shift + W], k[:, :, :, shift:shift + W]
        obase = torch.full_like(base, float("nan"))
        out = obase[:, 1:4, :, shift:shift + W]
        assert L.FilterInterpolationLayer_gpu_forward_lp(xv, flv, kv, out) == 0
        assert L.last_kernel_path() == path
        want = oracle.filter_interpolation_forward(xv.float().cpu().numpy(), flv.cpu().numpy(), kv.float().cpu().numpy())
        check(out, want, T, "view %s shift %d" % (tname, shift))
        rest = obase.clone()
        rest[:, 1:4, :, shift:shift + W] = 0
        assert torch.isnan(rest[:, 0]).all() and torch.isnan(rest[:, 4:]).all()      # nothing outside the view written


@pytest.mark.parametrize("tname,flow_t,kind", [("bf16", "fp32", "smooth"), ("fp16", "T", "iid"),
                                               ("bf16", "T", "far"), ("fp16", "fp32", "smooth")])
@pytest.mark.parametrize("W", [160, 157])
def test_blend_matches_oracle(oracle, tname, flow_t, kind, W):
    from my_package.modules.FilterInterpolationBlendModule import FilterInterpolationBlendModule
    T = DTYPES[tname]
    FT = T if flow_t == "T" else torch.float32
    B, C, H = 2, 3, 24
    rng = np.random.default_rng(3)
    x0, x2 = synth.np_image(rng, B, C, H, W), synth.np_image(rng, B, C, H, W)
    f0, f1 = np_flow(rng, B, H, W, kind), np_flow(rng, B, H, W, kind)
    k0, k1 = synth.np_filter(rng, B, H, W), synth.np_filter(rng, B, H, W)
    o0 = rng.random((B, 1, H, W), dtype=np.float32)
    o1 = (1.0 - o0).astype(np.float32)
    x0, x2, k0, k1, o0, o1 = (widened(a, T) for a in (x0, x2, k0, k1, o0, o1))
    f0, f1 = widened(f0, FT), widened(f1, FT)
    with torch.no_grad():
        got = FilterInterpolationBlendModule()(to_dev(x0, T), to_dev(x2, T), to_dev(f0, FT), to_dev(f1, FT),
                                               to_dev(k0, T), to_dev(k1, T), to_dev(o0, T), to_dev(o1, T))
    assert got.dtype == T
    assert last_path() == ("fi_blend_lp:tiled_c3" if W % 4 == 0 else "fi_blend_lp:direct")
    w0 = oracle.filter_interpolation_forward(x0, f0, k0)
    w2 = oracle.filter_interpolation_forward(x2, f1, k1)
    p0, p2 = (o0 * w0).astype(np.float32), (o1 * w2).astype(np.float32)
    check(got, (p0 + p2).astype(np.float32), T, "blend %s flow %s %s W%d" % (tname, flow_t, kind, W))


def test_large_shapes_once_each(oracle):
    for T, FT, (B, C, H, W) in ((torch.bfloat16, torch.float32, (32, 3, 720, 1280)),
                                (torch.float16, torch.float16, (2, 64, 720, 1280))):
        x, flow, filt = inputs(2024 + C, B, C, H, W, "smooth")
        xw, fw, kw = widened(x, T), widened(flow, FT), widened(filt, T)
        del x, filt
        got = fi(to_dev(xw, T), to_dev(fw, FT), to_dev(kw, T))
        assert last_path() == ("fi_fwd_lp:tiled_c3" if C == 3 else "fi_fwd_lp:tiled_c4n")
        check(got, oracle.filter_interpolation_forward(xw, fw, kw), T, "fi %s %dx%dx%dx%d" % (T, B, C, H, W))
        del got
        torch.cuda.empty_cache()


@pytest.mark.parametrize("W", [160, 157])
def test_fp16_overflow_goes_to_inf_like_a_cast(oracle, W):
    T = torch.float16
    rng = np.random.default_rng(9)
    B, C, H = 1, 3, 16
    x = widened(rng.uniform(1e4, 6e4, (B, C, H, W)).astype(np.float32), T)
    x[:, :, :, : W // 2] = widened(rng.random((B, C, H, W // 2), dtype=np.float32), T)      # finite half
    flow = widened(synth.np_flow(rng, B, H, W, "smooth"), T)
    filt = widened(rng.uniform(0.5, 1.5, (B, 16, H, W)).astype(np.float32), T)       # a quadrant sums ~4 taps: > 65504
    got = fi(to_dev(x, T), to_dev(flow, T), to_dev(filt, T))
    want = torch.from_numpy(oracle.filter_interpolation_forward(x, flow, filt))
    wT = want.to(T)
    assert bool(torch.isinf(wT).any()) and bool(torch.isfinite(wT).any())
    g = got.cpu()
    assert torch.equal(torch.isinf(g), torch.isinf(wT)) and torch.equal(g[torch.isinf(g)], wT[torch.isinf(wT)])
    fin = torch.isfinite(wT)
    check(g[fin], want[fin], T, "fp16 overflow W%d" % W)


@pytest.mark.parametrize("tname", sorted(DTYPES))
@pytest.mark.parametrize("C", [3, 4])
def test_backward_is_the_fp32_backward_on_widened_inputs(tname, C):
    """The half layer's gradients are the fp32 layer's on the widened inputs, rounded once: bit for bit for the flow and the
    taps.  The image gradient is not reproducible from run to run on either side, so it cannot be asked to be bit-equal:
      C = 4 (the half call widens on the host: the fp32 library twice).  fi_bwd_cn.hip's fi_bwd_image_owner stores every cell
            once, without global atomics -- but the cell's list of (coefficient, site) entries is built with LDS atomics:
            atomicCAS hands the head slot of a tap index to whichever site's lane gets there first, atomicAdd on the cell's
            cursor (oc) orders the tail entries, and the replay sums `entry coefficient x gradoutput` with fmas in list
            order, head slots, then the tails in segments.  That per-cell sum is order-dependent: last-bit differences in a
            few per cent of the cells between two runs.
      C = 3 (the half layer's native kernel against the fp32 one).  Both pack the same integers into the LDS planes; what
            differs is the order in which pk_flush's global fp32 atomics of neighbouring tiles' overlapping boxes retire.
    Rule (tests/_image_grad.py: float64 restatement `want`, derived per-cell `bound`; the planes' part only for C = 3): both
    results lie within bound + ulp_T / 2 of want; they are bit-equal wherever no rounding boundary of T lies inside
    want +- bound (a result within the bound then has one possible rounding); at most one ulp_T apart elsewhere."""
    from my_package.modules.FilterInterpolationModule import FilterInterpolationModule
    from my_package.modules.FilterInterpolationBlendModule import FilterInterpolationBlendModule
    T = DTYPES[tname]
    B, H, W = 2, 24, 160
    x, flow, filt = inputs(31, B, C, H, W, "smooth")
    rng = np.random.default_rng(32)
    gout = rng.standard_normal((B, C, H, W)).astype(np.float32)

    # every input is rounded to T first: the fp32 run sees exactly the half run's values, widened
    def run(dt):
        ts = [to_dev(widened(a, T), dt).requires_grad_(True) for a in (x, flow, filt)]
        out = FilterInterpolationModule()(*ts)
        out.backward(to_dev(widened(gout, T), dt))
        return [t.grad for t in ts]

    lo = run(T)
    hi = run(torch.float32)
    for g_lo, g_hi, name in zip(lo, hi, ("image", "flow", "taps")):
        assert g_lo.dtype == T
        if name != "image":
            assert torch.equal(g_lo, g_hi.to(T)), name
    # the image gradient: the restatement of the operation on these inputs and its derived bound (tests/_image_grad.py)
    import _image_grad as IG
    ref = IG.Reference(widened(flow, T), widened(filt, T), widened(gout, T), fs=4, planes=C == 3)
    lo1, hi1 = lo[0].double().cpu().numpy(), hi[0].to(T).double().cpu().numpy()
    worst = [float(ref.ratio(g, st)[0].max()) for g, st in ((lo1, tname), (hi1, tname), (hi[0].double().cpu().numpy(), None))]
    inside = ref.boundary_inside(tname)
    apart = np.abs(lo1 - hi1) / IG.ulp_T(np.maximum(np.abs(lo1), np.abs(hi1)), tname)
    print("image gradient C%d %s: max err / (bound + ulp_T / 2) %.3f (half layer) and %.3f (fp32 layer, rounded), fp32 layer before "
          "rounding: max err / bound %.3f; a rounding boundary in reach of %.4f of the cells, %d of them differ, %d elsewhere"
          % (C, tname, worst[0], worst[1], worst[2], float(inside.mean()), int((lo1 != hi1)[inside].sum()),
             int((lo1 != hi1)[~inside].sum())))
    assert max(worst) <= 1.0, worst
    assert bool((lo1 == hi1)[~inside].all()), "image: different roundings where no rounding boundary of T is in reach"
    assert float(apart[inside].max() if inside.any() else 0.0) <= 1.0, "image: more than one ulp_T apart"
    if C == 3:      # the blend as well
        o0 = rng.random((B, 1, H, W), dtype=np.float32)
        occs = (widened(o0, T), widened((1.0 - o0).astype(np.float32), T))

        def blend(dt):
            ts = [to_dev(widened(a, T), dt).requires_grad_(True) for a in (x, x[::-1].copy(), flow, flow[::-1].copy(),
                                                                           filt, filt[::-1].copy())]
            occ = [to_dev(a, dt).requires_grad_(True) for a in occs]
            FilterInterpolationBlendModule()(*ts, *occ).backward(to_dev(widened(gout, T), dt))
            return [t.grad for t in ts + occ]

        for g_lo, g_hi in zip(blend(T), blend(torch.float32)):
            assert g_lo.dtype == T and torch.equal(g_lo, g_hi.to(T))


def test_float32_is_not_rerouted():
    """A float32 call through the Modules is, bit for bit, a direct call of the fp32 entry points."""
    import my_package._ext.my_lib as my_lib
    from my_package.modules.FilterInterpolationModule import FilterInterpolationModule
    from my_package.modules.FilterInterpolationBlendModule import FilterInterpolationBlendModule
    B, C, H, W = 2, 3, 24, 160
    x, flow, filt = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in inputs(41, B, C, H, W, "smooth"))
    with torch.no_grad():
        got = FilterInterpolationModule()(x, flow, filt)
        want = torch.empty_like(x)
        assert my_lib.FilterInterpolationLayer_gpu_forward(x, flow, filt, want) == 0
        assert torch.equal(got, want) and got.dtype == torch.float32
        occ = torch.rand(B, 1, H, W, device="cuda")
        got = FilterInterpolationBlendModule()(x, x.flip(0).contiguous(), flow, flow.flip(0).contiguous(), filt,
                                               filt.flip(0).contiguous(), occ, 1 - occ)
        want = torch.empty_like(x)
        assert my_lib.FilterInterpolationBlendLayer_gpu_forward(x, x.flip(0).contiguous(), flow, flow.flip(0).contiguous(),
                                                                filt, filt.flip(0).contiguous(), occ, 1 - occ, want) == 0
        assert torch.equal(got, want)


@pytest.mark.parametrize("tname", sorted(DTYPES))
def test_host_widened_operators_return_the_input_dtype(tname):
    """Operators without half kernels widen on the host: the float32 result, cast to the input's dtype."""
    from my_package.modules.FlowProjectionModule import FlowProjectionModule
    from my_package.modules.DepthFlowProjectionModule import DepthFlowProjectionModule
    from my_package.modules.InterpolationModule import InterpolationModule
    from my_package.modules.InterpolationChModule import InterpolationChModule
    T = DTYPES[tname]
    rng = np.random.default_rng(5)
    B, H, W = 2, 24, 64
    flow = to_dev(synth.np_flow(rng, B, H, W, "smooth"), T)
    x = to_dev(synth.np_image(rng, B, 3, H, W), T)
    x8 = to_dev(synth.np_image(rng, B, 8, H, W), T)
    depth = to_dev(synth.np_depth(rng, B, H, W), T)
    with torch.no_grad():
        for got, want in ((FlowProjectionModule(False)(flow), FlowProjectionModule(False)(flow.float())),
                          (DepthFlowProjectionModule(False)(flow, depth),
                           DepthFlowProjectionModule(False)(flow.float(), depth.float())),
                          (InterpolationModule()(x, flow), InterpolationModule()(x.float(), flow.float())),
                          (InterpolationChModule()(x8, flow), InterpolationChModule()(x8.float(), flow.float()))):
            assert got.dtype == T
            # one rounding of the fp32 result (the projections' scattered sums may differ in their last fp32 bit)
            err = (got.float() - want).abs().cpu()
            assert bool((err <= ulp(want.cpu(), T) + 1e-6).all()), float(err.max())


def test_extensions_keep_float32_only():
    from my_package.modules.FlowUpsample4Module import FlowUpsample4Module
    from my_package.modules.FilterInterpolationCtxBlendModule import FilterInterpolationCtxBlendModule
    z = lambda c: torch.zeros(1, c, 16, 16, device="cuda", dtype=torch.float16)     # noqa: E731
    with pytest.raises(TypeError):
        FlowUpsample4Module(20.0, 2.0)(z(2))
    with pytest.raises(TypeError):
        FilterInterpolationCtxBlendModule()(z(3), z(3), z(8), z(8), z(2), z(2), z(16), z(16), z(1), z(1))
