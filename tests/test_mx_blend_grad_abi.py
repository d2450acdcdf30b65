"""The mixed-precision blend backward library libmemc_hip_mx_blend_grad.so (include/memc_warp_mx_blend_grad.h: fp32 image
and gradoutput beside fp16 / bf16 taps and occlusion): loads without a GPU, exports exactly its header and none of the other
libraries' entry points, rejects malformed descriptors with -1 and declines calls outside its coverage with 1 before
touching the device, none of its kernels spills, and the Python door (my_lib_blend_grad) forwards the mixed pattern to it.
CPU only -- no kernel is launched here (every call below is rejected, declined or empty)."""
import ctypes
import glob
import os
import re
import shutil
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_blend_grad_abi as BG      # noqa: E402  (Tensor4, desc, the export helpers and the fp32 kernel's own check)
import test_mx_abi as MX              # noqa: E402  (the uncovered calls)

HEADER = os.path.join(ROOT, "include", "memc_warp_mx_blend_grad.h")
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
LIB = os.path.join(LIBDIR, "libmemc_hip_mx_blend_grad.so")
UNIT = "mx_fi_blend_bwd_c3.hip"
F32, F16, BF16 = 0, 1, 2
PAIRS = ((F16, F32), (F16, F16), (BF16, F32), (BF16, BF16))      # (tap, flow) dtypes
SYMBOLS = ["memc_mx_blend_grad_version", "memc_mx_blend_grad_last_kernel_path",
           "FilterInterpolationBlendLayer_gpu_backward_mx"]
ORDER = BG.ORDER                      # in1, flow, taps, occ, gout, gflow, gtaps, gocc
desc = BG.desc


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(names) == sorted(SYMBOLS), names
    return names


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(LIB)
    L.memc_mx_blend_grad_version.restype = ctypes.c_char_p
    L.memc_mx_blend_grad_last_kernel_path.restype = ctypes.c_char_p
    f = L.FilterInterpolationBlendLayer_gpu_backward_mx
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(BG.Tensor4)] * 8
    return L


class Call:
    """One call: the tensors of a well-formed, covered B x C x H x W call, any of them replaceable."""

    def __init__(self, lib, B=2, C=3, H=8, W=16, taps=16):
        self.f = lib.FilterInterpolationBlendLayer_gpu_backward_mx
        self.t = {"in1": desc((B, C, H, W)), "flow": desc((B, 2, H, W)), "taps": desc((B, taps, H, W)),
                  "occ": desc((B, 1, H, W)), "gout": desc((B, C, H, W)), "gflow": desc((B, 2, H, W)),
                  "gtaps": desc((B, taps, H, W)), "gocc": desc((B, 1, H, W))}

    def __call__(self, td=F16, fd=F32, **repl):
        """td / fd: the tap and flow dtypes; keywords in1 .. gocc replace a tensor (None: NULL)"""
        t = dict(self.t, **repl)
        return self.f(None, td, fd, *(None if t[k] is None else ctypes.byref(t[k]) for k in ORDER))


def test_loads_without_a_gpu_and_identifies_itself(lib):
    assert lib.memc_mx_blend_grad_version() == b"memc_hip_mx_blend_grad 0.1 gfx950"
    assert lib.memc_mx_blend_grad_last_kernel_path() == b""     # no call enqueued by this thread yet


def test_exports_exactly_the_header(lib):
    syms = BG._exported(LIB)
    c_surface = sorted(n for n in syms if not BG._is_hip_plumbing(n))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    assert any("fi_blend_bwd_c3_mx" in k for k in kernels), kernels
    # its own kernels only: not the fp32 instantiation of the shared body, not the warp's backward kernels
    assert not [n for n in syms if "fi_blend_bwd_c3I" in n or "fi_bwd_c3_pk" in n or "fi_bwd_c3_mx" in n]
    # a library of its own: none of its C symbols in any other product library
    other_libs = [p for p in glob.glob(os.path.join(LIBDIR, "libmemc_hip*.so")) if p != LIB]
    assert len(other_libs) >= 7, other_libs               # fp32, measure, lp, lp_grad, blend_grad, mx, mx_grad
    others = {n for p in other_libs for n in BG._exported(p) if not BG._is_hip_plumbing(n)}
    for name in ("FilterInterpolationBlendLayer_gpu_backward", "FilterInterpolationLayer_gpu_backward_mx",
                 "FilterInterpolationBlendLayer_gpu_forward_mx", "FilterInterpolationLayer_gpu_backward_lp"):
        assert name in others, name
    assert not others & set(syms), others & set(syms)


def test_rejects_bad_descriptors(lib):
    call = Call(lib)
    # tap dtype: fp32 (the fp32 library's business) or no dtype at all; flow neither fp32 nor the taps'
    for taps, fl in ((F32, F32), (3, F32), (-1, F16), (F16, BF16), (BF16, F16), (F16, 7)):
        assert call(taps, fl) == -1, (taps, fl)
    for taps, fl in PAIRS:
        kw = dict(td=taps, fd=fl)
        # each of the eight tensors null, or with null data
        for k in ORDER:
            assert call(**{k: None}, **kw) == -1, k
            assert call(**{k: desc(tuple(call.t[k].size), data=0)}, **kw) == -1, k
        # a flow that is not [B, 2, H, W]; an occlusion with two channels
        assert call(flow=desc((2, 3, 8, 16)), gflow=desc((2, 3, 8, 16)), **kw) == -1
        assert call(flow=desc((1, 2, 8, 16)), gflow=desc((1, 2, 8, 16)), **kw) == -1
        assert call(flow=desc((2, 2, 7, 16)), gflow=desc((2, 2, 7, 16)), **kw) == -1
        assert call(flow=desc((2, 2, 8, 12)), gflow=desc((2, 2, 8, 12)), **kw) == -1
        assert call(occ=desc((2, 2, 8, 16)), gocc=desc((2, 2, 8, 16)), **kw) == -1
        # a tap count that is not a square (with its gradient of the same shape)
        for k in (15, 8, 0):
            assert call(taps=desc((2, k, 8, 16)), gtaps=desc((2, k, 8, 16)), **kw) == -1, k
        # each gradient of another shape or layout than its input
        assert call(gout=desc((2, 3, 8, 12)), **kw) == -1
        assert call(gout=desc((2, 4, 8, 16)), **kw) == -1
        assert call(gout=desc((2, 3, 8, 16), strides=(800, 200, 20, 1)), **kw) == -1
        assert call(gflow=desc((2, 2, 8, 12)), **kw) == -1
        assert call(gflow=desc((2, 2, 8, 16), strides=(512, 256, 32, 1)), **kw) == -1
        assert call(gtaps=desc((2, 9, 8, 16)), **kw) == -1
        assert call(gtaps=desc((2, 16, 8, 16), strides=(4096, 256, 32, 1)), **kw) == -1
        assert call(gocc=desc((2, 2, 8, 16)), **kw) == -1
        assert call(gocc=desc((2, 1, 8, 16), strides=(256, 256, 32, 1)), **kw) == -1
        # a w-stride of 2
        assert call(in1=desc((2, 3, 8, 16), strides=(768, 256, 32, 2)),
                    gout=desc((2, 3, 8, 16), strides=(768, 256, 32, 2)), **kw) == -1
        assert call(occ=desc((2, 1, 8, 16), strides=(256, 256, 32, 2)),
                    gocc=desc((2, 1, 8, 16), strides=(256, 256, 32, 2)), **kw) == -1
        # a stride beyond int32
        assert call(in1=desc((2, 3, 8, 16), strides=(1 << 33, 128, 16, 1)), **kw) == -1
        assert call(gflow=desc((2, 2, 8, 16), strides=(256, 1 << 32, 16, 1)), **kw) == -1
    assert lib.memc_mx_blend_grad_last_kernel_path() == b""     # nothing was enqueued


@pytest.mark.parametrize("case", MX.uncovered(), ids=[c[0] for c in MX.uncovered()])
def test_calls_outside_the_coverage_are_declined(lib, case):
    """tests/test_mx_abi.py's uncovered calls: return code 1 for every dtype pair, nothing touched"""
    _label, C, taps, W, tap_ptr, tap_row = case
    B, H = 2, 8
    row = tap_row or W
    tap_strides = (taps * H * row, H * row, row, 1)
    c = Call(lib, C=C, H=H, W=W, taps=taps)
    k = desc((B, taps, H, W), data=tap_ptr, strides=tap_strides)
    g3 = desc((B, taps, H, W), strides=tap_strides)       # of the taps' layout, on a quad itself
    for tdt, fdt in PAIRS:
        assert c(tdt, fdt, taps=k, gtaps=g3) == 1
    assert lib.memc_mx_blend_grad_last_kernel_path() == b""     # nothing was enqueued


def test_occlusions_off_a_quad_are_declined(lib):
    """half quads are 8 bytes: an occlusion (or its gradient) whose base is two bytes off one, or whose rows are not a
    multiple of four elements apart, is well-formed and not covered"""
    c = Call(lib)
    rows = (8 * 18, 8 * 18, 18, 1)
    for tdt, fdt in PAIRS:
        assert c(tdt, fdt, occ=desc((2, 1, 8, 16), data=0x10002)) == 1
        assert c(tdt, fdt, gocc=desc((2, 1, 8, 16), data=0x10002)) == 1
        assert c(tdt, fdt, occ=desc((2, 1, 8, 16), strides=rows), gocc=desc((2, 1, 8, 16), strides=rows)) == 1
    assert lib.memc_mx_blend_grad_last_kernel_path() == b""     # nothing was enqueued


def test_empty_batch_is_a_no_op(lib):
    e = lambda c: desc((0, c, 8, 16), data=0)      # noqa: E731
    for taps, fl in PAIRS:
        assert Call(lib)(taps, fl, in1=e(3), flow=e(2), taps=e(16), occ=e(1), gout=e(3), gflow=e(2), gtaps=e(16),
                         gocc=e(1)) == 0
    assert lib.memc_mx_blend_grad_last_kernel_path() == b""     # nothing was launched


def test_no_mixed_blend_backward_kernel_spills():
    """The compiler's own resource remarks: the four instantiations by name -- 2 tap dtypes x 2 flow dtypes -- no private
    scratch, no dynamic stack, the fp32 kernel's two workgroups of 256 lanes per CU (occupancy of at least 2 waves per
    SIMD)."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    from tools import kernel_resources as KR
    kernels = KR.resources_of(UNIT)
    names = sorted(k["name"] for k in kernels)
    want = sorted("memc::fi_blend_bwd_c3_mx<memc::%s, memc::%s>" % (t, f) for t in ("F16", "BF16") for f in ("F32", t))
    assert names == want, names
    bad = [(k["name"], k.get("scratch"), k.get("dynstack"), k.get("occupancy")) for k in kernels
           if int(k.get("scratch", "0")) > 0 or k.get("dynstack", "False") != "False" or int(k.get("occupancy", "0")) < 2]
    assert not bad, bad
    assert UNIT in KR.SOURCES


def test_the_fp32_blend_backward_library_keeps_its_kernel():
    """tests/test_blend_grad_abi.py's own kernel check for libmemc_hip_blend_grad.so: the shared kernel body instantiates
    there what it did"""
    BG.test_blend_grad_kernel_does_not_spill()


# --------------------------------------------------------------------------------------------------------------
# the Python side: the binding, and my_lib_blend_grad's function as the one door
# --------------------------------------------------------------------------------------------------------------
def _bindings():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_blend_grad as B
    import my_package._ext.my_lib_mx_blend_grad as M
    return B, M


def test_the_python_loader_binds_the_library():
    _B, M = _bindings()
    assert M.LIB_PATH == LIB
    assert M.version() == "memc_hip_mx_blend_grad 0.1 gfx950"
    assert M.last_kernel_path() == ""
    assert callable(M.FilterInterpolationBlendLayer_gpu_backward_mx)


def _tensors(t, ft, **other):
    """the eight tensors of one direction on the CPU (no kernel is reached): dtypes by position, `other` replaces some"""
    import torch
    f32 = torch.float32
    dt = dict(zip(ORDER, (f32, ft, t, t, f32, ft, t, t)), **other)
    shapes = dict(zip(ORDER, (3, 2, 16, 1, 3, 2, 16, 1)))
    return tuple(torch.zeros((1, shapes[k], 8, 16), dtype=dt[k]) for k in ORDER)


def test_the_blend_backward_door_forwards_the_mixed_pattern(monkeypatch):
    import torch
    B, M = _bindings()
    seen = []
    monkeypatch.setattr(M, "FilterInterpolationBlendLayer_gpu_backward_mx", lambda *a: seen.append(("mx", a)) or 0)
    monkeypatch.setattr(B._SAT, "call", lambda symbol, leading, tensors, **kw: seen.append(("f32", tensors, kw)) or 0)
    for t in (torch.float16, torch.bfloat16):
        for ft in (torch.float32, t):
            args = _tensors(t, ft)
            del seen[:]
            assert B.FilterInterpolationBlendLayer_gpu_backward(*args) == 0
            assert len(seen) == 1 and seen[0][0] == "mx" and all(a is b for a, b in zip(seen[0][1], args)), seen
    # eight float32 tensors: the float32 library, its dtype check as before
    args = _tensors(torch.float32, torch.float32)
    del seen[:]
    assert B.FilterInterpolationBlendLayer_gpu_backward(*args) == 0
    assert len(seen) == 1 and seen[0][0] == "f32" and seen[0][2] == {"dtypes": (torch.float32,) * 8}, seen


def test_the_blend_backward_door_rejects_other_dtype_mixes(monkeypatch):
    """neither eight float32 tensors nor the mixed pattern: the TypeError of the float32 binding's dtype check, and the
    mixed library is not reached"""
    import torch
    B, M = _bindings()
    reached = []
    monkeypatch.setattr(M, "FilterInterpolationBlendLayer_gpu_backward_mx", lambda *a: reached.append(a) or 0)
    # the check under test comes behind the descriptors': keep a CPU tensor from ending the call before it, and the C
    # function out of reach
    import my_package._ext._satellite as S
    monkeypatch.setattr(S, "describe", lambda t, symbol, position: BG.Tensor4())
    monkeypatch.setattr(B._SAT, "_lib", types.SimpleNamespace(
        FilterInterpolationBlendLayer_gpu_backward=lambda *a: pytest.fail("the float32 library was called")))
    h, b, f32 = torch.float16, torch.bfloat16, torch.float32
    for args in (_tensors(h, f32, occ=b), _tensors(h, f32, gtaps=f32), _tensors(h, b), _tensors(h, f32, gflow=h),
                 _tensors(h, f32, in1=h), _tensors(b, b, gout=b), _tensors(f32, f32, occ=h), _tensors(f32, h),
                 _tensors(h, f32, gocc=f32)):
        with pytest.raises(TypeError, match="expected float32"):
            B.FilterInterpolationBlendLayer_gpu_backward(*args)
    assert not reached
