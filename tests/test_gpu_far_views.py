"""Both sides of the 32-bit addressing guards on the device (DESIGN.md "Addressing audit"; tests/_far_views.py).

Every case cuts its tensors out of ONE arena of 2^31 + 2^21 fp32 elements (8 GiB) filled with a NaN canary: the tensors of the
group at the limit share a gigantic row stride and interleave inside its gaps, the others are ordinary dense tensors.  A
kernel that reads outside its windows poisons its result; one that writes outside them is found by the scan of the arena
that ends every case.  Shapes: B = 2, H = 33 (two tile rows of 16 and a ragged one; row H - 1 carries the largest
offsets), W = 72 (a 64-wide tile and a ragged one) or 70 (a ragged width), C = 3 (the RGB kernels) or 8 (chunked / owner).
The flow is N(0, 2^2) px with one site of row H - 1 set so that it is valid and its window holds row H - 1.

  near   the largest admitted stride: returns 0, takes the dense call's kernel family, gives the dense call's bits
         (forward outputs, flow and tap gradients) or stays inside tests/_image_grad's bound (image gradients), and is held
         to tests/_parity.close against the CPU oracle; a second call gives the same bits where no atomics are involved;
  far    one quantum more: the backward passes of libmemc_hip.so go to their 64-bit family (asserted), a plane beyond
         INT32_MAX elements is refused with -1 and nothing is written;
  far batches / channels: ordinary rows, (B - 1) * batch stride or (C - 1) * channel stride beyond 2^31 elements.
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

import _far_views as V                     # noqa: E402
import _image_grad as IG                   # noqa: E402
import _parity as P                        # noqa: E402
import _spynet_spec as S                   # noqa: E402
import _spynet_grad_spec as SG             # noqa: E402
from tools import synth                    # noqa: E402

pytestmark = pytest.mark.gpu

B, H, W = 2, 33, 72
ARENA_NUMEL = V.ARENA_NUMEL
NEAR_U32, FAR_U32 = V.near_far(V.fits_u32, H, W, 4)
NEAR_INT, FAR_INT = V.near_far(V.fits_int, H, W, 4)
assert (NEAR_U32, FAR_U32, NEAR_INT, FAR_INT) == (33554428, 33554432, 67108860, 67108864)
assert NEAR_INT % 256 != 0 and NEAR_U32 % 256 != 0 and FAR_U32 % 256 == 0 and FAR_INT % 256 == 0


def my_lib():
    import my_package._ext.my_lib as M
    return M


@pytest.fixture(scope="module")
def arena():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a GPU")
    free, _total = torch.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip("needs 12 GiB of free device memory")
    a = V.Arena(ARENA_NUMEL, "cuda:0")
    yield a
    print("\ntest_gpu_far_views: torch.cuda.max_memory_allocated() = %.2f GiB" % (torch.cuda.max_memory_allocated() / 2.0 ** 30))
    del a.bits
    torch.cuda.empty_cache()


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_INPUTS = {}


def inputs(C, Wd=W, fs=4, nb=B):
    """x, flow, filt, gout as numpy, made once per shape and never written"""
    key = (C, Wd, fs, nb)
    if key not in _INPUTS:
        rng = np.random.default_rng(4100 + 7 * C + Wd + fs + 100 * nb)
        flow = synth.np_flow(rng, nb, H, Wd, "iid", 2.0)
        flow[:, 0, H - 1, 2], flow[:, 1, H - 1, 2] = 0.25, -0.5    # valid, and its window holds row H - 1 (asserted below)
        d = dict(x=synth.np_image(rng, nb, C, H, Wd), flow=flow, filt=synth.np_filter(rng, nb, H, Wd, fs),
                 gout=(synth.np_image(rng, nb, C, H, Wd) - np.float32(0.5)))
        valid, _ix, iy, _a, _b = IG.locate32(flow)
        assert valid[:, H - 1, 2].all() and (iy[:, H - 1, 2] + fs // 2 >= H - 1).all(), "no site forms the largest offsets"
        _INPUTS[key] = d
    return _INPUTS[key]


def place(arena, spec, at_limit, stride, outer=None):
    """spec: [(name, shape, group)].  The tensors whose group is in `at_limit` are cut out of the (re-filled) arena with the
    row stride `stride` (outer = 0 / 1: ordinary rows and a far batch / channel stride instead), the others are dense and
    NaN-filled.  Returns ({name: tensor}, [names inside the arena])."""
    arena.fill()
    lay = V.Layout()
    inside = [(n, s) for n, s, g in spec if g in at_limit]
    if outer is None:
        wins, _end = V.interleave(lay, inside, stride)
    else:
        wins = V.far_outer(lay, inside, outer)
    lay.check()
    assert lay.nbytes <= arena.numel * 4
    t = {}
    for n, s, _g in spec:
        t[n] = arena.tensor(wins[n]) if n in wins else torch.full(s, float("nan"), device="cuda")
    return t, [n for n, _s in inside]


def finish(arena, t, inside, outputs):
    torch.cuda.synchronize()
    arena.untouched_outside([t[n] for n in inside if n in outputs], [t[n] for n in inside if n not in outputs])


def refused(arena, t, inside, outputs):
    """after a call that was refused: its outputs hold what they held (the canary inside the arena, NaN outside it), and
    nothing else of the arena was written"""
    torch.cuda.synchronize()
    arena.unwritten([t[n] for n in outputs if n in inside])
    for n in outputs:
        if n not in inside:
            assert bool(torch.isnan(t[n]).all()), "the refused call wrote into " + str(n)
    arena.untouched_outside([], [t[n] for n in inside])


def same(got, want, what):
    assert torch.equal(got.contiguous(), want), "%s: not the dense call's bits" % what


# ------------------------------------------------------------------------------------------------------------------
# FilterInterpolation forward.  No u32 guard (64-bit addressing on the tiled paths); its one-lane-per-site, any-filter-size
# and one-site kernels form row offsets in int, so a plane beyond INT32_MAX elements is refused (include/memc_warp.h, Limits).
# ------------------------------------------------------------------------------------------------------------------
FI_FWD_GROUPS = {"image": ("x", "out"), "flow": ("flow",), "taps": ("filt",)}
_DENSE = {}


def fi_fwd_spec(C, Wd, fs, nb=B):
    return [("x", (nb, C, H, Wd), "image"), ("flow", (nb, 2, H, Wd), "flow"), ("filt", (nb, fs * fs, H, Wd), "taps"),
            ("out", (nb, C, H, Wd), "image")]


def fi_fwd_call(t):
    return my_lib().FilterInterpolationLayer_gpu_forward(t["x"], t["flow"], t["filt"], t["out"])


def fi_fwd_dense(oracle, C, Wd, fs, nb=B):
    key = ("fi_fwd", C, Wd, fs, nb)
    if key not in _DENSE:
        d = inputs(C, Wd, fs, nb)
        t = {"x": D(d["x"]), "flow": D(d["flow"]), "filt": D(d["filt"]), "out": torch.full(d["x"].shape, float("nan"), device="cuda")}
        assert fi_fwd_call(t) == 0
        path = my_lib().last_kernel_path()
        P.close(t["out"].cpu().numpy(), oracle.filter_interpolation_forward(d["x"], d["flow"], d["filt"]), "dense FI forward")
        _DENSE[key] = (t["out"], path)
    return _DENSE[key]


def fi_fwd_through(arena, oracle, C, Wd, fs, groups, stride, served):
    d = inputs(C, Wd, fs)
    want, path = fi_fwd_dense(oracle, C, Wd, fs)
    t, inside = place(arena, fi_fwd_spec(C, Wd, fs), groups, stride)
    for n in ("x", "flow", "filt"):
        t[n].copy_(D(d[n]))
    code = fi_fwd_call(t)
    if not served:
        assert code == -1, "a plane beyond INT32_MAX elements was not refused: %d" % code
        refused(arena, t, inside, ("out",))
        return
    assert code == 0 and my_lib().last_kernel_path() == path, (code, my_lib().last_kernel_path(), path)
    same(t["out"], want, "FI forward C=%d W=%d fs=%d %s at %d" % (C, Wd, fs, groups, stride))
    first = t["out"].contiguous()
    assert fi_fwd_call(t) == 0
    same(t["out"], first, "second call")
    finish(arena, t, inside, ("out",))


FWD_SIDES = [("near_u32", NEAR_U32, True), ("far_u32", FAR_U32, True), ("near_int", NEAR_INT, True),
             ("far_int", FAR_INT, False)]


@pytest.mark.parametrize("side,stride,served", FWD_SIDES, ids=[s[0] for s in FWD_SIDES])
@pytest.mark.parametrize("group", ["image", "flow", "taps", "all"])
@pytest.mark.parametrize("C", [3, 8])
def test_fi_forward(arena, oracle, C, group, side, stride, served):
    groups = tuple(FI_FWD_GROUPS) if group == "all" else (group,)
    fi_fwd_through(arena, oracle, C, W, 4, groups, stride, served)


FWD_HOLE = [(3, 72, 2, "fi_fwd:generic"), (8, 72, 2, "fi_fwd:generic"), (3, 70, 4, "fi_fwd:tiled_c3"),
            (8, 70, 4, "fi_fwd:tiled_c4n_ragged"), (3, 6, 4, "fi_fwd:direct"), (1, 72, 4, "fi_fwd:tiled_chunks")]


@pytest.mark.parametrize("C,Wd,fs,path", FWD_HOLE, ids=["C%d-W%d-fs%d" % c[:3] for c in FWD_HOLE])
def test_fi_forward_int_row_offsets(arena, oracle, C, Wd, fs, path):
    """The kernels that multiply a row by the row stride in int (any filter size; the one-lane-per-site kernel, alone at
    W = 6 and behind the whole quads of W = 70; the one-site path of the tiled ones): served up to the last stride that keeps
    (H - 1) * stride + W within INT32_MAX -- also at a multiple of 256, the RGB kernel's shifted grid --, refused beyond."""
    assert fi_fwd_dense(oracle, C, Wd, fs)[1] == path
    near, far = V.near_far(V.fits_int, H, Wd, 1)
    for stride, served in ((near, True), (near // 256 * 256, True), (far, False)):
        assert V.fits_int(H, Wd, stride) == served
        fi_fwd_through(arena, oracle, C, Wd, fs, tuple(FI_FWD_GROUPS), stride, served)


# ------------------------------------------------------------------------------------------------------------------
# FilterInterpolation backward: fi_bwd_c3.hip (RGB) and fi_bwd_cn.hip (owner) behind plane_fits_u32 and the 4-plane rule
# ------------------------------------------------------------------------------------------------------------------
FI_BWD_GROUPS = {"image": ("x", "gout", "g1"), "flow": ("flow", "g2"), "taps": ("filt", "g3")}


def fi_bwd_spec(C, nb=B):
    return [("x", (nb, C, H, W), "image"), ("flow", (nb, 2, H, W), "flow"), ("filt", (nb, 16, H, W), "taps"),
            ("gout", (nb, C, H, W), "image"), ("g1", (nb, C, H, W), "image"), ("g2", (nb, 2, H, W), "flow"),
            ("g3", (nb, 16, H, W), "taps")]


def fi_bwd_call(t):
    return my_lib().FilterInterpolationLayer_gpu_backward(t["x"], t["flow"], t["filt"], t["gout"], t["g1"], t["g2"], t["g3"])


def fi_bwd_refs(oracle, C, nb=B):
    """the dense call's results and path, the oracle's gradients and the image gradient's float64 restatement: made once"""
    key = ("fi_bwd", C, nb)
    if key not in _DENSE:
        d = inputs(C, W, 4, nb)
        t = {n: D(d[n]) for n in ("x", "flow", "filt", "gout")}
        stored = my_lib().gradinput1_is_stored(4, C)
        t["g1"] = torch.full(d["x"].shape, float("nan") if stored else 0.0, device="cuda")
        t["g2"], t["g3"] = (torch.full(d[n].shape, float("nan"), device="cuda") for n in ("flow", "filt"))
        assert fi_bwd_call(t) == 0
        path = my_lib().last_kernel_path()
        want = oracle.filter_interpolation_backward(d["x"], d["flow"], d["filt"], d["gout"])
        _DENSE[key] = (t, path, want, IG.Reference(d["flow"], d["filt"], d["gout"], 4, planes=(C == 3)), stored)
        check_bwd(t, _DENSE[key], "dense FI backward C=%d" % C, exact=False)
    return _DENSE[key]


def check_bwd(t, refs, what, exact):
    dense, _path, want, ref, _stored = refs
    g1, g2, g3 = (t[n].contiguous() for n in ("g1", "g2", "g3"))
    if exact:                                    # the same kernel: the flow and tap gradients are its bits
        same(g2, dense["g2"], what + " gradinput2")
        same(g3, dense["g3"], what + " gradinput3")
    P.close(g1.cpu().numpy(), want[0], what + " gradinput1", P.RTOL)
    P.close(g2.cpu().numpy(), want[1], what + " gradinput2", P.RTOL)
    P.close(g3.cpu().numpy(), want[2], what + " gradinput3", P.RTOL)
    ratio, compared = ref.ratio(g1.cpu().numpy())
    print(what, "image gradient: worst |err| / bound %.3g" % float(ratio.max()))
    assert compared.all() and float(ratio.max()) <= 1.0, "%s: image gradient beyond tests/_image_grad's bound" % what


def fi_bwd_through(arena, oracle, C, groups, stride, want_path, outer=None, nb=B):
    d = inputs(C, W, 4, nb)
    refs = fi_bwd_refs(oracle, C, nb)
    t, inside = place(arena, fi_bwd_spec(C, nb), groups, stride, outer)
    for n in ("x", "flow", "filt", "gout"):
        t[n].copy_(D(d[n]))
    if want_path is not None and not refs[4]:
        t["g1"].zero_()                          # three channels: an accumulation target.  Four and more: STORED on every
    code = fi_bwd_call(t)                        # path -- the window stays NaN, so the fallback's clear is asserted below
    if want_path is None:
        assert code == -1
        refused(arena, t, inside, ("g1", "g2", "g3"))
        return
    assert code == 0 and my_lib().last_kernel_path() == want_path, (code, my_lib().last_kernel_path(), want_path)
    assert not torch.isnan(t["g1"]).any(), "gradinput1 was not cleared before the accumulating kernel ran"
    check_bwd(t, refs, "FI backward C=%d %s at %s" % (C, groups, stride if outer is None else "outer %d" % outer),
              exact=want_path == refs[1])
    finish(arena, t, inside, ("g1", "g2", "g3"))


# the owner's four-plane rule with the interleaved layout's channel stride (the padded width)
NEAR_4P, FAR_4P = V.near_far(lambda h, w, s: V.fits_u32(h, w, s) and V.owner_4plane(h, w, s, V.pad4(W)), H, W, 4)
assert FAR_4P < NEAR_U32

BWD_CASES = [(3, g, "near", NEAR_U32, "fi_bwd:tiled_c3") for g in ("image", "flow", "taps", "all")] + \
            [(3, g, "far", FAR_U32, "fi_bwd:direct") for g in ("image", "flow", "taps", "all")] + \
            [(8, "image", "near", NEAR_4P, "fi_bwd:owner"), (8, "image", "far4", FAR_4P, "fi_bwd:direct"),
             (8, "image", "far", FAR_U32, "fi_bwd:direct"), (8, "all", "near", NEAR_4P, "fi_bwd:owner"),
             (8, "all", "far", FAR_U32, "fi_bwd:direct")] + \
            [(8, g, "near", NEAR_U32, "fi_bwd:owner") for g in ("flow", "taps")] + \
            [(8, g, "far", FAR_U32, "fi_bwd:direct") for g in ("flow", "taps")] + \
            [(3, "image", "near_int", NEAR_INT, "fi_bwd:direct"), (8, "image", "near_int", NEAR_INT, "fi_bwd:direct"),
             (3, "image", "far_int", FAR_INT, None), (8, "all", "far_int", FAR_INT, None)]


@pytest.mark.parametrize("C,group,side,stride,path", BWD_CASES, ids=["C%d-%s-%s" % c[:3] for c in BWD_CASES])
def test_fi_backward(arena, oracle, C, group, side, stride, path):
    assert fi_bwd_refs(oracle, C)[1] == ("fi_bwd:tiled_c3" if C == 3 else "fi_bwd:owner")
    groups = tuple(FI_BWD_GROUPS) if group == "all" else (group,)
    fi_bwd_through(arena, oracle, C, groups, stride, path)


# ------------------------------------------------------------------------------------------------------------------
# Interpolation / InterpolationCh (the bilinear warp)
# ------------------------------------------------------------------------------------------------------------------
def bl_names(C):
    return ("InterpolationLayer", "interpolation") if C == 3 else ("InterpolationChLayer", "interpolation_ch")


def bl_refs(oracle, C):
    key = ("bl", C)
    if key not in _DENSE:
        d = inputs(C)
        sym, orc = bl_names(C)
        x, f, g = D(d["x"]), D(d["flow"]), D(d["gout"])
        out = torch.full_like(x, float("nan"))
        assert getattr(my_lib(), sym + "_gpu_forward")(x, f, out) == 0
        fpath = my_lib().last_kernel_path()
        P.close(out.cpu().numpy(), getattr(oracle, orc + "_forward")(d["x"], d["flow"]), "dense bilinear forward")
        stored = my_lib().gradinput1_is_stored(0, C)
        g1 = torch.full_like(x, float("nan") if stored else 0.0)
        g2 = torch.full_like(f, float("nan"))
        assert getattr(my_lib(), sym + "_gpu_backward")(x, f, g, g1, g2) == 0
        bpath = my_lib().last_kernel_path()
        want = getattr(oracle, orc + "_backward")(d["x"], d["flow"], d["gout"])
        P.close(g1.cpu().numpy(), want[0], "dense bilinear gradinput1", P.RTOL)
        P.close(g2.cpu().numpy(), want[1], "dense bilinear gradinput2", P.RTOL)
        _DENSE[key] = (out, fpath, g2, bpath, want, stored)
    return _DENSE[key]


BL_SPEC = {"fwd": lambda C: [("x", (B, C, H, W), "image"), ("flow", (B, 2, H, W), "flow"), ("out", (B, C, H, W), "image")],
           "bwd": lambda C: [("x", (B, C, H, W), "image"), ("flow", (B, 2, H, W), "flow"), ("gout", (B, C, H, W), "image"),
                             ("g1", (B, C, H, W), "image"), ("g2", (B, 2, H, W), "flow")]}

BL_FWD = [(C, g, side, stride, served) for C in (3, 8) for g in ("image", "flow", "all")
          for side, stride, served in (("near_u32", NEAR_U32, True), ("near_int", NEAR_INT, True), ("far_int", FAR_INT, False))]


@pytest.mark.parametrize("C,group,side,stride,served", BL_FWD, ids=["C%d-%s-%s" % c[:3] for c in BL_FWD])
def test_bilinear_forward(arena, oracle, C, group, side, stride, served):
    d, (want, fpath, _g2, _bp, _w, _s), sym = inputs(C), bl_refs(oracle, C), bl_names(C)[0]
    t, inside = place(arena, BL_SPEC["fwd"](C), ("image", "flow") if group == "all" else (group,), stride)
    for n in ("x", "flow"):
        t[n].copy_(D(d[n]))
    code = getattr(my_lib(), sym + "_gpu_forward")(t["x"], t["flow"], t["out"])
    if not served:
        assert code == -1
        refused(arena, t, inside, ("out",))
        return
    assert code == 0 and my_lib().last_kernel_path() == fpath
    same(t["out"], want, "bilinear forward C=%d %s %s" % (C, group, side))
    assert getattr(my_lib(), sym + "_gpu_forward")(t["x"], t["flow"], t["out"]) == 0
    same(t["out"], want, "second call")          # no atomics
    finish(arena, t, inside, ("out",))


BL_BWD = [(3, "image", "near", NEAR_U32, "bl_bwd:tiled_c3"), (3, "image", "far", FAR_U32, "bl_bwd:direct"),
          (3, "flow", "far", FAR_U32, "bl_bwd:tiled_c3"),      # the RGB kernel addresses the flow with 64-bit offsets
          (3, "all", "near", NEAR_U32, "bl_bwd:tiled_c3"),
          (8, "image", "near", NEAR_4P, "bl_bwd:owner"), (8, "image", "far4", FAR_4P, "bl_bwd:direct"),
          (8, "flow", "near", NEAR_U32, "bl_bwd:owner"), (8, "flow", "far", FAR_U32, "bl_bwd:direct"),
          (8, "all", "near", NEAR_4P, "bl_bwd:owner"), (8, "all", "far", FAR_U32, "bl_bwd:direct"),
          (3, "image", "near_int", NEAR_INT, "bl_bwd:direct"), (3, "image", "far_int", FAR_INT, None),
          (8, "flow", "far_int", FAR_INT, None)]


@pytest.mark.parametrize("C,group,side,stride,path", BL_BWD, ids=["C%d-%s-%s" % c[:3] for c in BL_BWD])
def test_bilinear_backward(arena, oracle, C, group, side, stride, path):
    d, (_o, _fp, dense_g2, bpath, want, stored), sym = inputs(C), bl_refs(oracle, C), bl_names(C)[0]
    assert bpath == ("bl_bwd:tiled_c3" if C == 3 else "bl_bwd:owner")
    t, inside = place(arena, BL_SPEC["bwd"](C), ("image", "flow") if group == "all" else (group,), stride)
    for n in ("x", "flow", "gout"):
        t[n].copy_(D(d[n]))
    if path is not None and not stored:
        t["g1"].zero_()
    code = getattr(my_lib(), sym + "_gpu_backward")(t["x"], t["flow"], t["gout"], t["g1"], t["g2"])
    if path is None:
        assert code == -1
        refused(arena, t, inside, ("g1", "g2"))
        return
    assert code == 0 and my_lib().last_kernel_path() == path, (code, my_lib().last_kernel_path(), path)
    assert not torch.isnan(t["g1"]).any(), "gradinput1 was not cleared before the accumulating kernel ran"
    if path == bpath:
        same(t["g2"], dense_g2, "bilinear gradinput2 C=%d %s %s" % (C, group, side))
    P.close(t["g1"].contiguous().cpu().numpy(), want[0], "bilinear gradinput1 %s %s" % (group, side), P.RTOL)
    P.close(t["g2"].contiguous().cpu().numpy(), want[1], "bilinear gradinput2 %s %s" % (group, side), P.RTOL)
    finish(arena, t, inside, ("g1", "g2"))


# ------------------------------------------------------------------------------------------------------------------
# Far batches and far channels: ordinary rows, (B - 1) * batch stride or (C - 1) * channel stride beyond 2^31 elements
# ------------------------------------------------------------------------------------------------------------------
OUTER = [(3, 0, "all"), (8, 0, "all"), (3, 1, "image"), (8, 1, "image"), (3, 1, "taps"), (8, 1, "taps")]


@pytest.mark.parametrize("C,dim,group", OUTER, ids=["C%d-%s-%s" % (c, "batch" if d == 0 else "channel", g) for c, d, g in OUTER])
def test_far_batches_and_channels(arena, oracle, C, dim, group):
    nb = 3 if dim == 0 else B
    d = inputs(C, W, 4, nb)
    want, path = fi_fwd_dense(oracle, C, W, 4, nb)
    groups = tuple(FI_FWD_GROUPS) if group == "all" else (group,)
    t, inside = place(arena, fi_fwd_spec(C, W, 4, nb), groups, None, outer=dim)
    far = [n for n in inside if (t[n].size(dim) - 1) * t[n].stride(dim) > (1 << 31)]
    assert far, "no tensor of the case spans 2^31 elements"
    for n in ("x", "flow", "filt"):
        t[n].copy_(D(d[n]))
    assert fi_fwd_call(t) == 0 and my_lib().last_kernel_path() == path
    same(t["out"], want, "FI forward with far %s" % ("batches" if dim == 0 else "channels"))
    finish(arena, t, inside, ("out",))
    fi_bwd_through(arena, oracle, C, tuple(FI_BWD_GROUPS) if group == "all" else (group,), None,
                   "fi_bwd:tiled_c3" if C == 3 else "fi_bwd:owner", outer=dim, nb=nb)


# ------------------------------------------------------------------------------------------------------------------
# SPyNet level: more batch elements than a grid's y dimension holds (the kernels' batch loops make a second trip)
# ------------------------------------------------------------------------------------------------------------------
PICK = [0, 1, 65535, 65536]


@pytest.mark.parametrize("shape", [(65537, 2, 2), (65537, 3, 5)], ids=["2x2", "3x5"])
def test_spynet_level_batches_beyond_the_grid(shape):
    import my_package._ext.my_lib_spynet as FWD
    import my_package._ext.my_lib_spynet_grad as BWD
    flags = (0, 1)
    first, second, coarse = S.ordinary_case(shape)
    run = lambda a, b, c: _spynet_fwd(FWD, a, b, c, flags)          # noqa: E731
    got = run(first, second, coarse)
    four = run(first[PICK], second[PICK], coarse[PICK])
    assert np.array_equal(got[PICK], four), "elements 0, 1, 65535, 65536 differ from the same elements as a batch of four"
    S.check_level(got[PICK], (first[PICK], second[PICK], coarse[PICK]), flags, "B = 65537 %s" % (shape,))
    assert np.array_equal(got[:, 0:3], first) and not np.isnan(got).any()

    G = np.random.default_rng(shape[1]).standard_normal((shape[0], 8) + shape[1:]).astype(np.float32)
    gc = _spynet_bwd(BWD, second, coarse, G, flags)
    gc4 = _spynet_bwd(BWD, second[PICK], coarse[PICK], G[PICK], flags)
    assert np.array_equal(gc[PICK], gc4) and not np.isnan(gc).any()
    want = SG.level_grad(second[PICK], coarse[PICK], G[PICK], flags, np.float64, up=four[:, 6:8])
    P.close(gc4.astype(np.float64), want, "B = 65537 %s: gradcoarse vs the float64 rule" % (shape,))


def _spynet_fwd(lib, first, second, coarse, flags):
    out = torch.full((first.shape[0], 8) + first.shape[2:], float("nan"), device="cuda")
    assert lib.SpyNetLevelLayer_gpu_forward(D(first), D(second), D(coarse), out, *flags) == 0
    return out.cpu().numpy()


def _spynet_bwd(lib, second, coarse, G, flags):
    gc = torch.full(coarse.shape, float("nan"), device="cuda")
    assert lib.SpyNetLevelLayer_gpu_backward(D(second), D(coarse), D(G), gc, *flags) == 0
    return gc.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------
# libmemc_hip.so's fused blend and context forward: 32-bit byte offsets with no 64-bit family behind them -- the near stride
# is served with the dense call's bits, the far one refused (-1: the caller composes the result from the warp's entry points)
# ------------------------------------------------------------------------------------------------------------------
def _fused_spec(which):
    if which == "blend":
        return [("in0", "i", "image"), ("in2", "i", "image"), ("flow0", "f", "flow"), ("flow1", "f", "flow"), ("filt0", "t", "taps"),
                ("filt1", "t", "taps"), ("occ0", "o", "occlusion"), ("occ1", "o", "occlusion"), ("out", "i", "image")], ("out",)
    return [("image", "i", "image"), ("context", "c", "context"), ("flow", "f", "flow"), ("filt", "t", "taps"), ("prev", "i", "image"),
            ("occ_prev", "o", "occlusion"), ("occ_this", "o", "occlusion"), ("image_out", "i", "image"),
            ("context_out", "c", "context")], ("image_out", "context_out")


def _fused_inputs(which):
    key = ("fused", which)
    if key not in _INPUTS:
        rng = np.random.default_rng(977 if which == "blend" else 978)
        spec, outs = _fused_spec(which)
        d = {}
        for name, kind, _g in spec:
            shape = V.kind_shape(kind, B, 3, H, W)
            if kind == "f":
                d[name] = synth.np_flow(rng, B, H, W, "iid", 2.0)
                d[name][:, 0, H - 1, 2], d[name][:, 1, H - 1, 2] = 0.25, -0.5
                valid, _ix, iy, _a, _b = IG.locate32(d[name])
                assert valid[:, H - 1, 2].all() and (iy[:, H - 1, 2] + 2 >= H - 1).all()
            else:
                d[name] = rng.random(shape, dtype=np.float32)
        _INPUTS[key] = d
    return _INPUTS[key]


FUSED = [(which, group, side) for which, groups in (("blend", ("image", "flow", "taps", "occlusion", "all")),
                                                    ("ctx", ("image", "occlusion", "all")))
         for group in groups for side in ("near", "far")]


@pytest.mark.parametrize("which,group,side", FUSED, ids=["%s-%s-%s" % f for f in FUSED])
def test_fused_forwards(arena, oracle, which, group, side):
    spec, outs = _fused_spec(which)
    d = _fused_inputs(which)
    fn = getattr(my_lib(), "FilterInterpolationBlendLayer_gpu_forward" if which == "blend" else "FilterInterpolationCtxLayer_gpu_forward")
    order = [n for n, _k, _g in spec]
    key = ("fused dense", which)
    if key not in _DENSE:
        t = {n: (torch.full(d[n].shape, float("nan"), device="cuda") if n in outs else D(d[n])) for n in order}
        assert fn(*[t[n] for n in order]) == 0
        sat_oracle(oracle, "memc.fi_blend" if which == "blend" else "memc.fi_ctx", [t[n] for n in order])
        _DENSE[key] = ({n: t[n] for n in outs}, my_lib().last_kernel_path())
    dense, _no_path = _DENSE[key]
    near, far = V.near_far(V.fits_u32, H, W, 1)
    groups = {g for _n, _k, g in spec} if group == "all" else {group}
    if which == "ctx":
        groups &= {"image", "occlusion"}         # the groups the context forward addresses with 32-bit offsets
    t, inside = place(arena, [(n, d[n].shape, g) for n, _k, g in spec], groups, near if side == "near" else far)
    for n in order:
        if n not in outs:
            t[n].copy_(D(d[n]))
    code = fn(*[t[n] for n in order])
    if side == "far":
        assert code == -1
        refused(arena, t, inside, outs)
        return
    assert code == 0                             # (one kernel, no path string: _NO_PATH)
    for n in outs:
        same(t[n], dense[n], "%s forward %s near: %s" % (which, group, n))
    assert fn(*[t[n] for n in order]) == 0       # no atomics: a second call gives the same bits
    for n in outs:
        same(t[n], dense[n], "%s forward %s near, second call: %s" % (which, group, n))
    finish(arena, t, inside, outs)


# ------------------------------------------------------------------------------------------------------------------
# Every entry point of tests/_far_views.ENTRIES through its binding -- the satellites and libmemc_hip.so alike: the dense
# call held to the CPU oracle (or the float64 rule), every guarded group at its near stride (0, the dense call's family and
# bits) and at its far stride (the entry point's code, nothing written), and every group with batches / channels beyond 2^31
# elements.  Half tensors are float16, the flow and gradoutput float32, as in the ABI module's calls.
# ------------------------------------------------------------------------------------------------------------------
EVERY = list(V.GUARDED)
SAT = [(k, g) for k, g in EVERY if not k.startswith("memc.")]
_OUTS = {"memc.proj_fwd": (1, 2), "memc.proj_fwd_ws": (1, 2), "memc.dproj_fwd": (2, 3), "memc.dproj_fwd_ws": (2, 3),
         "memc.proj_bwd": (3,), "memc.dproj_bwd": (5, 6), "lp_proj_grad.bwd": (3,), "lp_dproj_grad.bwd": (5, 6)}
_OUT_NAMES = ("out", "output", "image_out", "context_out", "gradinput1", "gradinput2", "gradinput3", "gradflow", "gradfilter",
              "gradocclusion", "gradcoarse")
# outputs that fp32 atomics (or the packed planes) add into: held to a bound, not to the dense call's bits
_ATOMIC = {"lp_grad.bwd": (4,), "mx_grad.bwd": (4,), "memc.fi_bwd": (4,), "lp_bl.bwd": (3,), "lp_bl.bwd_ch": (3,),
           "memc.bl_bwd": (3,), "memc.bl_bwd_ch": (3,)}


_BILINEAR = ("lp_bl.bwd", "lp_bl.bwd_ch", "memc.bl_bwd", "memc.bl_bwd_ch")    # atomics outputs without a restatement in _image_grad


def sat_outputs(key):
    if key in _OUTS:
        return list(_OUTS[key])
    return [i for i, (n, _k) in enumerate(V.ENTRIES[key].tensors) if n in _OUT_NAMES]


def sat_inputs(key, nb=B):
    """torch tensors of the entry point's dtypes, made once: images / taps / occlusions U[0, 1) as tools/synth and the libraries' parity tests draw them, flows N(0, 2^2) with the
    fixed site of row H - 1, depths U[0.1, 1.1), SPyNet's coarse flow N(0, 4^2), gradients N(0, 1), counts 1 .. 3"""
    if ("sat", key, nb) not in _INPUTS:
        import zlib
        e = V.ENTRIES[key]
        rng = np.random.default_rng(zlib.crc32(key.encode()) + nb)
        out = []
        for i, (name, kind) in enumerate(e.tensors):
            shape = V.kind_shape(kind, nb, 3, H, W)
            if kind in ("f", "F") and name not in ("output",):
                a = rng.normal(0.0, 2.0, shape).astype(np.float32)
                a[:, 0, H - 1, 2], a[:, 1, H - 1, 2] = 0.25, -0.5
            elif kind == "q":
                a = rng.normal(0.0, 4.0, shape).astype(np.float32)
            elif name == "count":
                a = rng.integers(1, 4, shape).astype(np.float32)
            elif name.startswith("grad") or kind == "s":
                a = rng.standard_normal(shape).astype(np.float32)
            elif name in ("input2", "depth") and kind == "o":
                a = (rng.random(shape, dtype=np.float32) + np.float32(0.1))      # a depth: tools/synth.np_depth
            else:
                a = rng.random(shape, dtype=np.float32)                          # images, taps, occlusions: tools/synth
            out.append(D(a).to(torch.float16 if i in e.half else torch.float32))
        _INPUTS[("sat", key, nb)] = out
    return _INPUTS[("sat", key, nb)]


# one kernel each, no family to choose: these entry points of libmemc_hip.so set no path string (the thread's string stays
# what the call before left), so no path is compared for them
_NO_PATH = ("memc.fi_blend", "memc.fi_ctx", "memc.upsample4")


def sat_call(key, tensors):
    import importlib
    e = V.ENTRIES[key]
    M = importlib.import_module("my_package._ext.my_lib_" + e.lib) if e.lib else my_lib()
    tail = e.tail
    if key.endswith("_ws"):                      # (fillhole, a workspace of the library's own size)
        tail = (e.tail[0], M.flow_projection_workspace(tensors[0], e.tail[0], depth=key.startswith("memc.dproj")))
    code = getattr(M, e.symbol)(*tensors, *tail)
    return code, ("one kernel" if key in _NO_PATH else M.last_kernel_path())


def hold(got, want, what, half=False, rtol=P.RTOL, cancel=0.0):
    """tests/_parity.close; a result stored as float16 was rounded once more, by at most half an ulp of float16 at
    |want| + the rule's own bound: that much is added to the rule, nothing else"""
    got, want = np.asarray(got.float().cpu().numpy(), dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not half:
        return P.close(got, want, what, rtol, cancel)
    aw = np.abs(want)
    rule = np.where(aw <= P.BIG, P.ATOL, np.maximum(P.ATOL, rtol * aw))
    bound = rule + 0.5 * IG.ulp_T(aw + rule, "fp16")
    err = np.abs(got - want)
    assert np.all(err <= bound), "%s: max abs err %.3g beyond the rule + half an fp16 ulp" % (what, float(err.max()))


def sat_oracle(oracle, key, t):
    """the dense call's outputs of entry point `key` held to the CPU oracle / the float64 rule on the widened inputs"""
    e = V.ENTRIES[key]
    w = [x.float().cpu().numpy() for x in t]
    half = lambda i: i in e.half                                  # noqa: E731
    name = key.split(".", 1)[1] if key.startswith("memc.") else key
    fi_f, fi_b = oracle.filter_interpolation_forward, oracle.filter_interpolation_backward
    if name in ("lp_grad.bwd", "mx_grad.bwd", "fi_bwd"):
        g = fi_b(w[0], w[1], w[2], w[3])
        for i, want in zip((4, 5, 6), g):
            hold(t[i], want, "%s %s vs the oracle" % (key, e.tensors[i][0]), half(i))
        ratio, compared = IG.Reference(w[1], w[2], w[3], 4, planes=True).ratio(w[4])
        assert compared.all() and float(ratio.max()) <= 1.0
    elif name in ("mx.fwd", "fi_fwd"):
        hold(t[3], fi_f(w[0], w[1], w[2]), key + " vs the oracle", half(3))
    elif name in ("mx.blend", "fi_blend"):
        want = w[6].astype(np.float64) * fi_f(w[0], w[2], w[4]) + w[7].astype(np.float64) * fi_f(w[1], w[3], w[5])
        hold(t[8], want, key + " vs the oracle's two warps blended in float64", half(8))
    elif name == "fi_ctx":
        hold(t[7], w[5].astype(np.float64) * w[4] + w[6].astype(np.float64) * fi_f(w[0], w[2], w[3]), key + " image_out")
        hold(t[8], fi_f(w[1], w[2], w[3]), key + " context_out")
    elif name in ("blend_grad.bwd", "mx_blend_grad.bwd", "lp_blend_grad.bwd"):
        # out = occlusion * FI(input, flow, filter): the warp's gradients for gradoutput * occlusion, and the occlusion's
        # gradient sum_c gradoutput * FI
        _g1, g2, g3 = fi_b(w[0], w[1], w[2], (w[4].astype(np.float64) * w[3]).astype(np.float32))
        gocc = (w[4].astype(np.float64) * fi_f(w[0], w[1], w[2])).sum(axis=1, keepdims=True)
        for i, want in zip((5, 6, 7), (g2, g3, gocc)):
            hold(t[i], want, "%s %s vs the oracle" % (key, e.tensors[i][0]), half(i))
    elif name.startswith("lp_bl.") or name.startswith("bl_"):
        ch = "_ch" if name.endswith("_ch") else ""
        if "fwd" in name:
            hold(t[2], getattr(oracle, "interpolation%s_forward" % ch)(w[0], w[1]), key + " vs the oracle", half(2))
        else:
            g1, g2 = getattr(oracle, "interpolation%s_backward" % ch)(w[0], w[1], w[2])
            hold(t[3], g1, key + " gradinput1", False)
            hold(t[4], g2, key + " gradinput2", half(4))
    elif name in ("lp_proj_grad.bwd", "proj_bwd"):
        hold(t[3], oracle.flow_projection_backward(w[0], w[1], w[2]), key + " vs the oracle", half(3))
    elif name in ("lp_dproj_grad.bwd", "dproj_bwd"):
        g1, g2 = oracle.depth_flow_projection_backward(w[0], w[1], w[2], w[3], w[4])
        hold(t[5], g1, key + " gradinput1", half(5))
        hold(t[6], g2, key + " gradinput2", half(6), cancel=P.CANCEL)
    elif name in ("proj_fwd", "proj_fwd_ws"):
        out, cnt = oracle.flow_projection_forward(w[0], 1)
        hold(t[2], out, key + " output")
        P.exact(w[1], cnt, key + " count")
    elif name in ("dproj_fwd", "dproj_fwd_ws"):
        out, cnt = oracle.depth_flow_projection_forward(w[0], w[1], 1)
        hold(t[3], out, key + " output")
        hold(t[2], cnt, key + " count (a sum of depths)")
    elif name in ("stack.fwd", "lp_stack.fwd"):
        n, _cb, skip = e.tail[:3]
        warp = fi_f(w[0], w[1], w[2])
        nb = w[3].shape[0]
        for k in range(n):
            slot = k + (1 if skip >= 0 and k >= skip else 0)
            hold(t[3][:, 3 * slot:3 * slot + 3], warp[k * nb:(k + 1) * nb], "%s neighbour %d vs the oracle" % (key, k), half(3))
    elif name == "spynet.fwd":
        S.check_level(w[3], (w[0], w[1], w[2]), e.tail, key)
    elif name == "spynet_grad.bwd":
        import my_package._ext.my_lib_spynet as FWD
        up = _spynet_fwd(FWD, np.zeros_like(w[0]), w[0], w[1], e.tail)[:, 6:8]
        P.close(w[3].astype(np.float64), SG.level_grad(w[0], w[1], w[2], e.tail, np.float64, up=up), key + " vs the float64 rule")
    elif name == "upsample4":
        want = torch.nn.functional.interpolate(t[0].double().cpu(), scale_factor=4, mode="bilinear", align_corners=False)
        hold(t[1], want.numpy(), key + " vs torch's float64 interpolate")
    else:
        raise AssertionError("no reference for " + key)


def sat_dense(oracle, key, nb=B):
    if ("sat", key, nb) not in _DENSE:
        src, outs = sat_inputs(key, nb), sat_outputs(key)
        t = [torch.zeros_like(x) if i in outs else x for i, x in enumerate(src)]
        code, path = sat_call(key, t)
        assert code == 0 and path, (key, code, path)
        torch.cuda.synchronize()
        sat_oracle(oracle, key, t)
        _DENSE[("sat", key, nb)] = (t, path)
    return _DENSE[("sat", key, nb)]


def sat_compare(key, what, t, dense, src):
    e = V.ENTRIES[key]
    for i in sat_outputs(key):
        name = e.tensors[i][0]
        if i in _ATOMIC.get(key, ()) and key not in _BILINEAR:
            # the image gradient adds with atomics / packed planes: tests/_image_grad's bound on the inputs' widened values
            ratio, compared = IG.Reference(src[1], src[2], src[3], 4, planes=True).ratio(t[i].contiguous().cpu().numpy())
            assert compared.all() and float(ratio.max()) <= 1.0, (key, what, float(ratio.max()))
        elif i in _ATOMIC.get(key, ()):
            # the bilinear image gradient (atomics; no restatement in tests/_image_grad): tests/_parity.close to the dense call's
            P.close(t[i].contiguous().cpu().numpy(), dense[i].cpu().numpy(), "%s %s gradinput1 vs the dense call" % (key, what), P.RTOL)
        else:
            same(t[i], dense[i], "%s %s: %s" % (key, what, name))


def sat_refused(arena, t, wins, outs):
    """after a declined or refused call: the outputs hold what they held (the canary inside the arena, NaN outside it),
    and nothing else of the arena was written"""
    arena.unwritten([t[i] for i in wins if i in outs])
    for i in outs:
        if i not in wins:
            assert bool(torch.isnan(t[i]).all()), "the refused call wrote into output %d" % i
    arena.untouched_outside([], [t[i] for i in wins])


def sat_fill(arena, key, src, wins, zero_outputs=True):
    outs, t = sat_outputs(key), []
    for i, x in enumerate(src):
        v = arena.tensor(wins[i], x.dtype) if i in wins else torch.full_like(x, float("nan"))
        if i in outs and zero_outputs:
            v.zero_()                            # as the dense call's (an accumulated image gradient; the stack's free slots)
        elif i not in outs:
            v.copy_(x)
        t.append(v)
    return t


SIDES = [(k, g, s) for k, g in SAT for s in (("near", "far") + (("near256",) if k in ("stack.fwd", "lp_stack.fwd") else ()))]


@pytest.mark.parametrize("key,group,side", SIDES, ids=["%s-%s-%s" % kgs for kgs in SIDES])
def test_satellites(arena, oracle, key, group, side):
    e = V.ENTRIES[key]
    src, outs = sat_inputs(key), sat_outputs(key)
    dense, path = sat_dense(oracle, key)
    at_limit = e.groups[group]
    Hh, Ww = src[at_limit[0]].shape[2:]
    near, far = V.near_far(V.rule_of(key, group), Hh, Ww, e.quantum)
    stride = {"near": near, "far": far, "near256": near // 256 * 256}[side]     # (a multiple of 256: the stack's shifted grid)
    arena.fill()
    _lay, wins = V.group_layout(key, group, stride)
    assert all(tuple(src[i].shape) == w.shape and src[i].element_size() == w.itemsize for i, w in wins.items())
    t = sat_fill(arena, key, src, wins, zero_outputs=side != "far")
    code, got_path = sat_call(key, t)
    torch.cuda.synchronize()
    if side == "far":
        assert code == 1, "%s with its %s tensors beyond the guard returned %d" % (key, group, code)
        sat_refused(arena, t, wins, outs)
        return
    assert code == 0 and got_path == path, (code, got_path, path)
    sat_compare(key, group + " " + side, t, dense, src)
    if key not in _ATOMIC:                       # no atomics: a second call gives the same bits
        first = [t[i].contiguous() for i in outs]
        assert sat_call(key, t)[0] == 0
        for i, f in zip(outs, first):
            same(t[i], f, "%s second call" % key)
    arena.untouched_outside([t[i] for i in wins if i in outs], [t[i] for i in wins if i not in outs])


def outer_cases(dim):
    """(entry point, group) pairs whose every tensor has three or more planes along `dim` (with two, a stride that takes the
    second plane beyond 2^31 elements does not fit int)"""
    out = []
    for k, g in EVERY:
        shapes = [V.kind_shape(V.ENTRIES[k].tensors[i][1], 3, 3, H, W) for i in V.ENTRIES[k].groups[g]]
        if all(s[dim] >= 3 for s in shapes):
            out.append((k, g))
    return out


OUTER_EVERY = [(k, g, dim) for dim in (0, 1) for k, g in outer_cases(dim)]
assert {(k, g) for k, g, dim in OUTER_EVERY if dim == 0} == set(EVERY)     # every group has its far-batch case


@pytest.mark.parametrize("key,group,dim", OUTER_EVERY, ids=["%s-%s-%s" % (k, g, ("batch", "channel")[d]) for k, g, d in OUTER_EVERY])
def test_far_batches_and_channels_of_every_entry_point(arena, oracle, key, group, dim):
    """Ordinary rows; the group's tensors with (B - 1) * batch stride (B = 3) or (C - 1) * channel stride beyond 2^31
    elements: the dense call's family and bits (the atomics bound for the image gradients).  Groups with a tensor of one or
    two channels have no far-channel case (outer_cases)."""
    e = V.ENTRIES[key]
    nb = 3 if dim == 0 else B
    src, outs = sat_inputs(key, nb), sat_outputs(key)
    dense, path = sat_dense(oracle, key, nb)
    arena.fill()
    _lay, placed = V.outer_layout(key, group, dim, nb)
    assert all(tuple(src[i].shape) == w.shape and src[i].element_size() == w.itemsize for i, w in placed.items())
    for i, w in placed.items():
        span = (w.shape[dim] - 1) * w.strides[dim]
        assert span > 1 << 31 and span * w.itemsize > 1 << 32
    t = sat_fill(arena, key, src, placed)
    code, got_path = sat_call(key, t)
    torch.cuda.synchronize()
    assert code == 0 and got_path == path, (key, group, code, got_path, path)
    sat_compare(key, "%s far %s" % (group, ("batches", "channels")[dim]), t, dense, src)
    arena.untouched_outside([t[i] for i in placed if i in outs], [t[i] for i in placed if i not in outs])


# ------------------------------------------------------------------------------------------------------------------
# (Depth)FlowProjection forward: the owner kernel addresses the flow and depth planes with 32-bit byte offsets
# (flow_projection.hip: proj_resolve's plane_fits_u32); beyond the guard the call takes the general family.  The count's
# offsets are 64-bit on the owner path.  The backward has no fast-path guard.  Beyond INT32_MAX elements: refused.
# ------------------------------------------------------------------------------------------------------------------
PROJ = [(k, g, side) for k in ("memc.proj_fwd", "memc.proj_fwd_ws", "memc.dproj_fwd", "memc.dproj_fwd_ws", "memc.proj_bwd",
                               "memc.dproj_bwd")
        for g in V.ENTRIES[k].groups for side in ("near_u32", "far_u32", "near_int", "far_int")]


@pytest.mark.parametrize("key,group,side", PROJ, ids=["%s-%s-%s" % p for p in PROJ])
def test_projections(arena, oracle, key, group, side):
    e = V.ENTRIES[key]
    src, outs = sat_inputs(key), sat_outputs(key)
    dense, path = sat_dense(oracle, key)
    op = key.split(".")[1].replace("_ws", "")            # proj_fwd, dproj_fwd, proj_bwd, dproj_bwd
    assert path == op + (":owner" if "fwd" in op else ":tiled"), path
    rule, q = (V.fits_u32, 4) if side.endswith("u32") else (V.fits_int, 1)
    near, far = V.near_far(rule, H, W, q)
    stride = near if side.startswith("near") else far
    arena.fill()
    _lay, wins = V.group_layout(key, group, stride)
    t = sat_fill(arena, key, src, wins, zero_outputs=side != "far_int")
    code, got_path = sat_call(key, t)
    torch.cuda.synchronize()
    if side == "far_int":
        assert code == -1
        sat_refused(arena, t, wins, outs)
        return
    # the forward's fast path is guarded on the flow's and the depth's row stride
    slow = "fwd" in key and group in ("flow", "depth") and side != "near_u32"
    want_path = path.replace("owner", "general") if slow else path
    assert code == 0 and got_path == want_path, (code, got_path, want_path)
    if slow:                                     # another family: the oracle again
        sat_oracle(oracle, key, [x.contiguous() for x in t])
    else:
        sat_compare(key, "%s %s" % (group, side), t, dense, src)
    arena.untouched_outside([t[i] for i in wins if i in outs], [t[i] for i in wins if i not in outs])


# ------------------------------------------------------------------------------------------------------------------
# The one-site path of the tiled forwards (fi_site_scalar: the function whose int row offset was unguarded) through a
# view at the int limit.  A plane of 600 rows; one tile holds a site that moves 299 rows up and one that moves 299 rows
# down, so its source box spans the whole height, more than the six bands a tile sweeps: tests/_lowp_paths.census, which
# restates the band sweep, counts the sites left to the one-site path, and the site that lands on row H - 1 is one of them.
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 8])
def test_fi_forward_one_site_path_at_the_int_limit(arena, oracle, C):
    import _lowp_paths as LP
    Ht, Wt = 600, 72
    rng = np.random.default_rng(600 + C)
    flow = synth.np_flow(rng, 1, Ht, Wt, "iid", 2.0)
    flow[0, :, 300, 8], flow[0, :, 300, 12] = (0.25, 298.5), (0.25, -298.5)
    valid, _ix, iy, _a, _b = IG.locate32(flow)
    assert valid[0, 300, 8] and iy[0, 300, 8] + 2 >= Ht - 1, "the far site does not reach row H - 1"
    census = LP.census(flow)
    assert census["capped"] >= 1 and census["slow"] >= 1, census
    x, filt = synth.np_image(rng, 1, C, Ht, Wt), synth.np_filter(rng, 1, Ht, Wt)
    want = oracle.filter_interpolation_forward(x, flow, filt)
    dense = torch.full(x.shape, float("nan"), device="cuda")
    assert my_lib().FilterInterpolationLayer_gpu_forward(D(x), D(flow), D(filt), dense) == 0
    path = my_lib().last_kernel_path()
    assert path == ("fi_fwd:tiled_c3" if C == 3 else "fi_fwd:tiled_c4n")
    P.close(dense.cpu().numpy(), want, "one-site path, dense")
    near, far = V.near_far(V.fits_int, Ht, Wt, 4)
    spec = [("x", x.shape, "image"), ("flow", flow.shape, "flow"), ("filt", filt.shape, "taps"), ("out", x.shape, "image")]
    for stride, served in ((near, True), (far, False)):
        t, inside = place(arena, spec, ("image",), stride)
        for n, a in (("x", x), ("flow", flow), ("filt", filt)):
            t[n].copy_(D(a))
        code = fi_fwd_call(t)
        if not served:
            assert code == -1
            refused(arena, t, inside, ("out",))
            continue
        assert code == 0 and my_lib().last_kernel_path() == path
        same(t["out"], dense, "one-site path through a view at the int limit")
        finish(arena, t, inside, ("out",))


@pytest.mark.parametrize("C", [3, 8])
def test_bilinear_forward_ragged_width_at_the_int_limit(arena, oracle, C):
    """W = 70: the whole quads on the tiled kernel, the last columns on the one-lane-per-site kernel (int row offsets)"""
    Wd, (sym, orc) = 70, bl_names(C)
    d = inputs(C, Wd)
    x, f = D(d["x"]), D(d["flow"])
    dense = torch.full_like(x, float("nan"))
    fn = getattr(my_lib(), sym + "_gpu_forward")
    assert fn(x, f, dense) == 0
    path = my_lib().last_kernel_path()
    P.close(dense.cpu().numpy(), getattr(oracle, orc + "_forward")(d["x"], d["flow"]), "bilinear forward W = 70")
    near, far = V.near_far(V.fits_int, H, Wd, 1)
    spec = [("x", x.shape, "image"), ("flow", f.shape, "flow"), ("out", x.shape, "image")]
    for stride, served in ((near, True), (far, False)):
        t, inside = place(arena, spec, ("image", "flow"), stride)
        t["x"].copy_(x)
        t["flow"].copy_(f)
        code = fn(t["x"], t["flow"], t["out"])
        if not served:
            assert code == -1
            refused(arena, t, inside, ("out",))
            continue
        assert code == 0 and my_lib().last_kernel_path() == path
        same(t["out"], dense, "bilinear forward W = 70 at the int limit")
        first = t["out"].contiguous()
        assert fn(t["x"], t["flow"], t["out"]) == 0
        same(t["out"], first, "second call")
        finish(arena, t, inside, ("out",))


# ------------------------------------------------------------------------------------------------------------------
# The groups of libmemc_hip.so that only the int rule guards and that no case above puts at the limit: the context
# forward's context planes (fi_site_scalar's int row offsets), flow and taps, and the x4 upsample's input and output
# ------------------------------------------------------------------------------------------------------------------
MEMC_INT = [(k, g, side) for k, g in EVERY if k in ("memc.fi_ctx", "memc.upsample4") and V.rule_of(k, g) is V.fits_int
            for side in ("near_int", "far_int")]
assert len(MEMC_INT) == 10


@pytest.mark.parametrize("key,group,side", MEMC_INT, ids=["%s-%s-%s" % m for m in MEMC_INT])
def test_int_rule_groups_of_the_context_forward_and_the_upsample(arena, oracle, key, group, side):
    e = V.ENTRIES[key]
    src, outs = sat_inputs(key), sat_outputs(key)
    dense, path = sat_dense(oracle, key)
    Hh, Ww = src[e.groups[group][0]].shape[2:]
    near, far = V.near_far(V.fits_int, Hh, Ww, 1)
    arena.fill()
    _lay, wins = V.group_layout(key, group, near if side == "near_int" else far)
    t = sat_fill(arena, key, src, wins, zero_outputs=side == "near_int")
    code, got_path = sat_call(key, t)
    torch.cuda.synchronize()
    if side == "far_int":
        assert code == -1
        sat_refused(arena, t, wins, outs)
        return
    assert code == 0 and got_path == path, (code, got_path, path)
    sat_compare(key, group + " " + side, t, dense, src)
    first = [t[i].contiguous() for i in outs]
    assert sat_call(key, t)[0] == 0              # no atomics: a second call gives the same bits
    for i, f in zip(outs, first):
        same(t[i], f, "%s second call" % key)
    arena.untouched_outside([t[i] for i in wins if i in outs], [t[i] for i in wins if i not in outs])
