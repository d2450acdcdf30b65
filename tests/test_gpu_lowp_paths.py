"""The tiled fp16 / bf16 warps (libmemc_hip_lp.so, libmemc_hip_lp_grad.so) on inputs that reach every path of the tile
machinery they share with the fp32 kernels (memc_tile.hpp): vertical and horizontal band sweeps, the kMaxBands cap, the
per-site loop from global memory, lanes whose four sites are stored in pieces, tiles without a valid site, lanes of mixed
validity, and -- in the backward -- the packed planes' outlier sites, a zero gradoutput, NaN / Inf inputs and a gradinput1
that already holds values.  tests/_lowp_paths.py is the case table; tests/test_lowp_path_census.py shows on the CPU which
case reaches which path (the libraries report only the kernel family), and that the 24 x 160 inputs of
tests/test_gpu_lowp_parity.py reach none of the band, cap or per-site paths.

Rules, all taken over unchanged from the modules that own them:
  forward, blend    test_gpu_lowp_parity.check: |got - want| <= ulp_T(want) / 2 + 2e-5 * max(1, |want|) against the fp32 oracle
                    on the widened inputs, and >= 99 % of the elements equal to want.to(T) (a last-bit fp32 difference flips
                    a half rounding about once in 2^13 elements; the observed fraction is printed).  Outputs are pre-filled
                    with NaN: an unwritten site fails.
  backward          gradinput2 / gradinput3 bit-equal to the fp32 library's on the widened inputs, rounded (pre-filled with
                    NaN on both sides: the kernels define them); gradinput1 through test_gpu_lowp_grad.image_gradients_agree:
                    every finite cell of either side, before rounding, within tests/_image_grad.py's derived bound (the packed
                    planes' grid plus fp32's roundings, whatever order the atomics retire in) of the float64 restatement on
                    the call's inputs, and 99.9 % equal after rounding to T -- after the fp32 library run twice passed it;
                    against the oracle: tests/_parity.py's rule plus half an ulp_T for a gradient stored in T.
  heavy tails       gradinput1 under the rules of test_gpu_parity.test_rgb_backward_packed_planes_heavy_tailed_tile, which the
                    fp32 library on the same widened inputs is held to first.
Every figure is printed before it is asserted (`pytest -s`); profiles/lowp_paths_observed.md keeps one run's.
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

import _lowp_paths as LP                   # noqa: E402
import _parity as P                        # noqa: E402
import test_gpu_lowp_parity as FWD         # noqa: E402  (check, ulp, to_dev, widened)
import test_gpu_lowp_grad as BWD           # noqa: E402  (image_gradients_agree, image_reference, ulp)
from tools import synth                    # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = FWD.DTYPES
TNAMES = sorted(DTYPES)
NAN = float("nan")

# channel counts per table case: the RGB kernel, the c4n kernel on whole chunks (8) and its RAGGED instantiation (5);
# the 64-channel context warp on the first and third case, a single channel on the second
FWD_CHANNELS = [[3, 8, 5, 64], [3, 8, 5, 1], [3, 8, 5, 64], [3, 8, 5], [3, 8, 5], [3, 8, 5]]


def lp():
    import my_package._ext.my_lib_lp as L
    return L


def lpg():
    import my_package._ext.my_lib_lp_grad as G
    return G


def f32lib():
    import my_package._ext.my_lib as M
    return M


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dtype)


def worst(got, want):
    """largest |got - want| over the finite elements (printed beside check()'s exact fraction)"""
    g, w = got.detach().float().cpu(), torch.as_tensor(want).float()
    fin = torch.isfinite(w) & torch.isfinite(g)
    return float((g[fin] - w[fin]).abs().max()) if bool(fin.any()) else 0.0


# --------------------------------------------------------------------------------------------------------------
# forward and blend
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", ["fp32", "T"])
@pytest.mark.parametrize("ci", range(len(LP.CASES)), ids=LP.CASE_IDS)
def test_forward_on_every_tile_path(oracle, ci, tname, flow_t):
    T = DTYPES[tname]
    FT = T if flow_t == "T" else torch.float32
    case = LP.CASES[ci]
    for C in FWD_CHANNELS[ci]:
        x, flow, filt, _ = LP.case_inputs(case, C)
        xw, fw, kw = FWD.widened(x, T), FWD.widened(flow, FT), FWD.widened(filt, T)
        tx = dev(xw, T)
        out = torch.full_like(tx, NAN)
        assert lp().FilterInterpolationLayer_gpu_forward_lp(tx, dev(fw, FT), dev(kw, T), out) == 0
        assert lp().last_kernel_path() == ("fi_fwd_lp:tiled_c3" if C == 3 else "fi_fwd_lp:tiled_c4n")
        want = oracle.filter_interpolation_forward(xw, fw, kw)
        label = "fwd %s %s flow %s C%d" % (LP.CASE_IDS[ci], tname, flow_t, C)
        print("%s: unwritten %d, worst err %.3g" % (label, int(torch.isnan(out).sum()), worst(out, want)))
        FWD.check(out, want, T, label)


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("flow_t", ["fp32", "T"])
@pytest.mark.parametrize("ci", range(len(LP.BLEND_CASES)), ids=LP.CASE_IDS[:len(LP.BLEND_CASES)])
def test_blend_on_every_tile_path(oracle, ci, tname, flow_t):
    T = DTYPES[tname]
    FT = T if flow_t == "T" else torch.float32
    case = LP.BLEND_CASES[ci]
    B, H, W, kind, sigma, seed = case
    rng = np.random.default_rng(seed)
    f0 = synth.np_flow(rng, B, H, W, kind, sigma)                  # the first draw: the census' flow
    f1 = LP.case_flow(case, second=True)                           # the first draw from seed + 100
    x0, x2 = synth.np_image(rng, B, 3, H, W), synth.np_image(rng, B, 3, H, W)
    k0, k1 = synth.np_filter(rng, B, H, W), synth.np_filter(rng, B, H, W)
    o0 = rng.random((B, 1, H, W), dtype=np.float32)
    o1 = (1.0 - o0).astype(np.float32)
    x0, x2, k0, k1, o0, o1 = (FWD.widened(a, T) for a in (x0, x2, k0, k1, o0, o1))
    f0, f1 = FWD.widened(f0, FT), FWD.widened(f1, FT)
    tx0 = dev(x0, T)
    out = torch.full_like(tx0, NAN)
    assert lp().FilterInterpolationBlendLayer_gpu_forward_lp(tx0, dev(x2, T), dev(f0, FT), dev(f1, FT), dev(k0, T), dev(k1, T),
                                                             dev(o0, T), dev(o1, T), out) == 0
    assert lp().last_kernel_path() == "fi_blend_lp:tiled_c3"
    w0 = oracle.filter_interpolation_forward(x0, f0, k0)
    w2 = oracle.filter_interpolation_forward(x2, f1, k1)
    p0, p2 = (o0 * w0).astype(np.float32), (o1 * w2).astype(np.float32)      # two products, one sum
    want = (p0 + p2).astype(np.float32)
    label = "blend %s %s flow %s" % (LP.CASE_IDS[ci], tname, flow_t)
    print("%s: unwritten %d, worst err %.3g" % (label, int(torch.isnan(out).sum()), worst(out, want)))
    FWD.check(out, want, T, label)


# --------------------------------------------------------------------------------------------------------------
# backward
# --------------------------------------------------------------------------------------------------------------
def run_lp(x, flow, filt, gout, g1):
    """the half library; g1: None or the fp32 buffer it adds into.  gradinput2 / gradinput3 start as NaN: the kernel defines them"""
    g2, g3 = torch.full_like(flow, NAN), torch.full_like(filt, NAN)
    err = lpg().FilterInterpolationLayer_gpu_backward_lp(x, flow, filt, gout, g1, g2, g3)
    torch.cuda.synchronize()
    assert err == 0
    assert lpg().last_kernel_path() == ("fi_bwd_lp:tiled_c3" if g1 is not None else "fi_bwd_lp:tiled_c3_noimage")
    return g1, g2, g3


def run_f32(x, flow, filt, gout, with_image, fill=0.0):
    """the fp32 library on the widened inputs"""
    x, flow, filt, gout = (t.float().contiguous() for t in (x, flow, filt, gout))
    g1 = torch.full_like(x, fill) if with_image else None
    g2, g3 = torch.full_like(flow, NAN), torch.full_like(filt, NAN)
    assert f32lib().FilterInterpolationLayer_gpu_backward(x, flow, filt, gout, g1, g2, g3) == 0
    torch.cuda.synchronize()
    assert f32lib().last_kernel_path() == "fi_bwd:tiled_c3"
    return g1, g2, g3


def bwd_inputs(case, T, flow_T, gout_T):
    """image and taps in T; flow / gradoutput in T, or float32 as generated (not on T's grid)"""
    x, flow, filt, gout = LP.case_inputs(case, 3)
    return dev(x, T), dev(flow, T if flow_T else torch.float32), dev(filt, T), dev(gout, T if gout_T else torch.float32)


def zeros_like_image(x, fill=0.0):
    return torch.full(x.shape, fill, dtype=torch.float32, device=x.device)


def against_oracle(oracle, x, flow, filt, gout, grads, label):
    """test_gpu_lowp_grad.test_half_gradients_match_the_oracle's bound: _parity's rule plus half an ulp_T for a gradient in T"""
    want = oracle.filter_interpolation_backward(*(t.float().cpu().numpy() for t in (x, flow, filt, gout)))
    for got, w, name in zip(grads, want, ("image", "flow", "taps")):
        if got is None:
            continue
        w = torch.from_numpy(np.asarray(w)).float()
        g = got.float().cpu()
        bound = torch.where(w.abs() <= 10, torch.full_like(w, 1e-4), torch.clamp(1e-5 * w.abs(), min=1e-4))
        if got.dtype != torch.float32:
            bound = bound + 0.5 * BWD.ulp(w, got.dtype)
        e = (g - w).abs()
        e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
        print("oracle %s %s: max err %.3g (|want| up to %.3g)" % (label, name, float(e.max()), float(w.abs().max())))
        assert bool((e <= bound).all()), (label, name, float(e.max()))


@pytest.mark.parametrize("tname", TNAMES)
@pytest.mark.parametrize("with_image", [True, False], ids=["image", "noimage"])
@pytest.mark.parametrize("ci", range(len(LP.CASES)), ids=LP.CASE_IDS)
def test_backward_on_every_tile_path(oracle, ci, tname, with_image):
    T = DTYPES[tname]
    case = LP.CASES[ci]
    # (flow in T, gradoutput in T): the two diagonal combinations everywhere, all four on the third case
    combos = [(True, True), (False, False)] + ([(True, False), (False, True)] if ci == 2 else [])
    for flow_T, gout_T in combos:
        x, flow, filt, gout = bwd_inputs(case, T, flow_T, gout_T)
        label = "bwd %s %s flow%s gout%s %s" % (LP.CASE_IDS[ci], tname, "T" if flow_T else "F32", "T" if gout_T else "F32",
                                               "image" if with_image else "noimage")
        g1, g2, g3 = run_lp(x, flow, filt, gout, zeros_like_image(x) if with_image else None)
        w1, w2, w3 = run_f32(x, flow, filt, gout, with_image)
        assert g2.dtype == flow.dtype and g3.dtype == T
        assert torch.equal(g2, w2.to(flow.dtype)), "flow gradient, " + label
        assert torch.equal(g3, w3.to(T)), "tap gradient, " + label
        if with_image:
            assert g1.dtype == torch.float32
            b1, _, _ = run_f32(x, flow, filt, gout, True)
            ref = BWD.image_reference(flow, filt, gout)
            BWD.image_gradients_agree(w1, b1, T, "control: fp32 twice, " + label, ref)
            BWD.image_gradients_agree(g1, w1, T, "native vs fp32, " + label, ref)
        if ci in (0, 2):
            against_oracle(oracle, x, flow, filt, gout, (g1.to(T) if with_image else None, g2, g3), label)


@pytest.mark.parametrize("tname", TNAMES)
def test_backward_adds_into_a_gradinput1_that_holds_values(oracle, tname):
    """The contract is "added into": a buffer pre-filled with 0.5 comes back as oracle + 0.5, under the rule (and the 3 x rtol)
    of the fp32 arms test -- on a case whose image gradient takes the planes' flushes, the outliers' and the slow sites' atomics."""
    T = DTYPES[tname]
    for ci in (0, 2):
        x, flow, filt, gout = bwd_inputs(LP.CASES[ci], T, True, True)
        g1, _, _ = run_lp(x, flow, filt, gout, zeros_like_image(x, 0.5))
        w1 = oracle.filter_interpolation_backward(*(t.float().cpu().numpy() for t in (x, flow, filt, gout)))[0]
        err = P.close(g1.cpu().numpy(), w1 + np.float32(0.5), "gradinput1 += %s %s" % (LP.CASE_IDS[ci], tname), 3 * P.RTOL)
        print("gradinput1 += %s %s: max err %.3g" % (LP.CASE_IDS[ci], tname, err))


# --------------------------------------------------------------------------------------------------------------
# backward, special values
# --------------------------------------------------------------------------------------------------------------
def heavy_tail_rules(got, want, kk, gg, name, label):
    """gradinput1 (fp32 numpy) under the rules of test_rgb_backward_packed_planes_heavy_tailed_tile"""
    if name.startswith("a step"):
        bound = float(np.abs(gg).max() * np.abs(kk).max())
        err = float(np.abs(got.astype(np.float64) - want).max())
        limit = 64 * 2.0 ** -22 * bound + 1e-5 * float(np.abs(want).max())
        print("%s, %s: err %.3g (tile-relative limit %.3g)" % (label, name, err, limit))
        assert err <= limit, (label, name, err, bound)
    else:
        small = np.abs(want) <= 1.0                                # the cells the outliers do not reach
        assert small.mean() > 0.3
        err_small = float(np.abs(got[small].astype(np.float64) - want[small]).max())
        print("%s, %s: max err %.3g, small cells %.3g" % (label, name, float(np.abs(got.astype(np.float64) - want).max()), err_small))
        P.close(got, want, "%s gradinput1, %s" % (label, name), P.RTOL)
        assert err_small <= 2e-5, "%s gradinput1, %s: small cells off by %.3g" % (label, name, err_small)


@pytest.mark.parametrize("tname", TNAMES)
def test_backward_heavy_tailed_tile(oracle, tname):
    """The inputs of test_gpu_parity.test_rgb_backward_packed_planes_heavy_tailed_tile rounded to T: sites beyond the tile's
    block exponent leave the packed planes for per-site atomics (pk_outlier_sites -> fi_bwd_site_image_atomics_lp)."""
    import test_gpu_parity as FP32
    T = DTYPES[tname]
    rng = np.random.default_rng(77)
    B, H, W = 1, 48, 128
    xn, fn = synth.np_image(rng, B, 3, H, W), synth.np_flow(rng, B, H, W, "smooth", 2.0)
    kn = (rng.random((B, 16, H, W)) * 0.05).astype(np.float32)
    gn = (rng.standard_normal((B, 3, H, W)) * 0.05).astype(np.float32)
    for name, kk, gg in FP32._heavy_tail_variants(rng, kn, gn):
        xw, fw, kw, gw = (FWD.widened(a, T) for a in (xn, fn, kk, gg))
        assert np.isfinite(kw).all() and np.isfinite(gw).all()
        want1 = oracle.filter_interpolation_backward(xw, fw, kw, gw)[0]
        for FT in (T, torch.float32):                              # the same values in T and in float32 storage
            x, flow, filt, gout = dev(xw, T), dev(fw, FT), dev(kw, T), dev(gw, FT)
            label = "heavy tail %s flow/gout %s" % (tname, "T" if FT == T else "F32")
            w1, w2, w3 = run_f32(x, flow, filt, gout, True)
            heavy_tail_rules(w1.cpu().numpy(), want1, kw, gw, name, "control: fp32 library, " + label)
            g1, g2, g3 = run_lp(x, flow, filt, gout, zeros_like_image(x))
            assert torch.equal(g2, w2.to(FT)), ("flow gradient", label, name)
            assert torch.equal(g3, w3.to(T)), ("tap gradient", label, name)
            heavy_tail_rules(g1.cpu().numpy(), want1, kw, gw, name, label)


@pytest.mark.parametrize("tname", TNAMES)
def test_backward_zero_gradoutput_adds_nothing(tname):
    """ps.any == 0: no packed site has anything to add.  gradinput1 (pre-filled with 0.25) comes back bit-identical."""
    T = DTYPES[tname]
    for ci in (0, 2, 4):
        for FT in (T, torch.float32):
            x, flow, filt, gout = bwd_inputs(LP.CASES[ci], T, FT == T, FT == T)
            gout = torch.zeros_like(gout)
            g1, g2, g3 = run_lp(x, flow, filt, gout, zeros_like_image(x, 0.25))
            assert torch.equal(g1, zeros_like_image(x, 0.25)), "zero gradoutput must add nothing"
            _, w2, w3 = run_f32(x, flow, filt, gout, True)
            assert torch.equal(g2, w2.to(flow.dtype)) and torch.equal(g3, w3.to(T))
            _, g2, g3 = run_lp(x, flow, filt, gout, None)
            _, w2, w3 = run_f32(x, flow, filt, gout, False)
            assert torch.equal(g2, w2.to(flow.dtype)) and torch.equal(g3, w3.to(T))


def same_specials_and_finite_bits(got, want, what):
    """the NaN and Inf patterns agree; the finite elements are bit-equal"""
    assert got.dtype == want.dtype
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN pattern of the " + what
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], want[inf]), "Inf pattern of the " + what
    fin = torch.isfinite(want)
    assert torch.equal(got[fin], want[fin]), "finite elements of the " + what
    return int(torch.isnan(want).sum()), int(inf.sum())


@pytest.mark.parametrize("tname", TNAMES)
def test_backward_nan_and_inf_inputs(tname):
    """One NaN tap, one -Inf tap and one NaN gradoutput, all at valid sites: such sites take per-site atomics, and every
    gradient carries the fp32 library's NaN / Inf pattern after rounding."""
    T = DTYPES[tname]
    case = LP.CASES[0]
    nan_tap, inf_tap, nan_gout = (0, 5, 40, 100), (0, 9, 70, 150), (0, 1, 50, 200)
    valid = LP.locate(LP.rounded(LP.case_flow(case), tname))[0]
    for _, _, y, xx in (nan_tap, inf_tap, nan_gout):
        assert valid[0, y, xx], "the special value must sit on a site that gathers"
    for with_image in (True, False):
        x, flow, filt, gout = bwd_inputs(case, T, True, True)
        filt[nan_tap] = NAN
        filt[inf_tap] = -float("inf")
        gout[nan_gout] = NAN
        g1, g2, g3 = run_lp(x, flow, filt, gout, zeros_like_image(x) if with_image else None)
        w1, w2, w3 = run_f32(x, flow, filt, gout, with_image)
        n2 = same_specials_and_finite_bits(g2, w2.to(T), "flow gradient")
        n3 = same_specials_and_finite_bits(g3, w3.to(T), "tap gradient")
        assert n2[0] + n2[1] > 0 and n3[0] + n3[1] > 0
        print("specials %s %s: flow gradient NaN %d Inf %d, tap gradient NaN %d Inf %d" % ((tname, with_image) + n2 + n3))
        if with_image:
            r1 = w1.to(T)
            assert 0 < int((~torch.isfinite(r1)).sum()) < 200
            b1, _, _ = run_f32(x, flow, filt, gout, True)
            ref = BWD.image_reference(flow, filt, gout)
            BWD.image_gradients_agree(w1, b1, T, "control: fp32 twice, NaN / Inf inputs %s" % tname, ref)
            BWD.image_gradients_agree(g1, w1, T, "native vs fp32, NaN / Inf inputs %s" % tname, ref)
