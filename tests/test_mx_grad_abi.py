"""The mixed-precision backward library libmemc_hip_mx_grad.so (include/memc_warp_mx_grad.h: fp32 image and gradoutput
beside fp16 / bf16 taps): loads without a GPU, exports exactly its header and none of the other libraries' entry points,
rejects malformed descriptors with -1 and declines calls outside its coverage with 1 before touching the device, and none of
its kernels spills.  CPU only -- no kernel is launched here (every call below is rejected, declined or empty)."""
import ctypes
import glob
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_lowp_grad_abi as LPG      # noqa: E402  (Tensor4, desc, the export helpers and the half backward's kernel check)
import test_mx_abi as MX              # noqa: E402  (the uncovered calls)

HEADER = os.path.join(ROOT, "include", "memc_warp_mx_grad.h")
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
LIB = os.path.join(LIBDIR, "libmemc_hip_mx_grad.so")
UNIT = "mx_fi_bwd_c3.hip"
F32, F16, BF16 = 0, 1, 2
PAIRS = ((F16, F32), (F16, F16), (BF16, F32), (BF16, BF16))      # (tap, flow) dtypes
SYMBOLS = ["memc_mx_grad_version", "memc_mx_grad_last_kernel_path", "FilterInterpolationLayer_gpu_backward_mx"]
desc = LPG.desc


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
    L.memc_mx_grad_version.restype = ctypes.c_char_p
    L.memc_mx_grad_last_kernel_path.restype = ctypes.c_char_p
    f = L.FilterInterpolationLayer_gpu_backward_mx
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(LPG.Tensor4)] * 7
    return L


class Call:
    """One backward call: the tensors of a well-formed, covered 2 x C x H x W call, any of them replaceable."""

    def __init__(self, lib, C=3, H=8, W=16, taps=16):
        self.f = lib.FilterInterpolationLayer_gpu_backward_mx
        self.t = {"in1": desc((2, C, H, W)), "flow": desc((2, 2, H, W)), "taps": desc((2, taps, H, W)),
                  "gout": desc((2, C, H, W)), "g1": desc((2, C, H, W)), "g2": desc((2, 2, H, W)),
                  "g3": desc((2, taps, H, W))}

    def __call__(self, td=F16, fd=F32, **repl):
        """td / fd: the tap and flow dtypes; keywords in1 .. g3 replace a tensor (g1=None: NULL)"""
        t = dict(self.t, **repl)
        P = lambda k: None if t[k] is None else ctypes.byref(t[k])      # noqa: E731
        return self.f(None, td, fd, *(P(k) for k in ("in1", "flow", "taps", "gout", "g1", "g2", "g3")))


def test_loads_without_a_gpu_and_identifies_itself(lib):
    assert lib.memc_mx_grad_version() == b"memc_hip_mx_grad 0.1 gfx950"
    assert lib.memc_mx_grad_last_kernel_path() == b""     # no call enqueued by this thread yet


def test_exports_exactly_the_header(lib):
    syms = LPG._exported(LIB)
    c_surface = sorted(n for n in syms if not LPG._is_hip_plumbing(n))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    assert any("fi_bwd_c3_mx" in k for k in kernels), kernels
    # a library of its own: none of the entry points of the other product libraries, none of their kernels
    other_libs = [p for p in glob.glob(os.path.join(LIBDIR, "libmemc_hip*.so")) if p != LIB]
    assert len(other_libs) >= 6, other_libs               # fp32, measure, lp, lp_grad, blend_grad, mx
    others = {n for p in other_libs for n in LPG._exported(p) if not LPG._is_hip_plumbing(n)}
    for name in ("FilterInterpolationLayer_gpu_backward", "FilterInterpolationLayer_gpu_backward_lp",
                 "FilterInterpolationLayer_gpu_forward_mx", "FilterInterpolationLayer_gpu_forward_lp"):
        assert name in others, name
    assert not others & set(syms), others & set(syms)
    assert not [n for n in syms if "fi_bwd_c3_pk" in n or "fi_bwd_c3_lp" in n or "fi_fwd_mx_tiled" in n]


def test_the_python_loader_binds_the_library():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_mx_grad as M
    assert M.LIB_PATH == LIB
    assert M.version() == "memc_hip_mx_grad 0.1 gfx950"
    assert M.last_kernel_path() == ""
    assert callable(M.FilterInterpolationLayer_gpu_backward_mx)


def test_rejects_bad_descriptors(lib):
    call = Call(lib)
    # tap dtype: fp32 (the fp32 library's business) or no dtype at all; flow neither fp32 nor the taps'
    for taps, fl in ((F32, F32), (3, F32), (-1, F16), (F16, BF16), (BF16, F16), (F16, 7)):
        assert call(taps, fl) == -1, (taps, fl)
        assert call(taps, fl, g1=None) == -1, (taps, fl)
    for taps, fl in PAIRS:
        kw = dict(td=taps, fd=fl)
        # mismatched shapes: flow with 3 channels / wrong batch / height; taps of another size
        assert call(flow=desc((2, 3, 8, 16)), **kw) == -1
        assert call(flow=desc((1, 2, 8, 16)), g2=desc((1, 2, 8, 16)), **kw) == -1
        assert call(flow=desc((2, 2, 7, 16)), g2=desc((2, 2, 7, 16)), **kw) == -1
        assert call(taps=desc((2, 16, 8, 12)), g3=desc((2, 16, 8, 12)), **kw) == -1
        # gradients of another shape or layout than their inputs
        assert call(gout=desc((2, 3, 8, 12)), **kw) == -1
        assert call(gout=desc((2, 3, 8, 16), strides=(800, 200, 20, 1)), **kw) == -1
        assert call(g2=desc((2, 2, 8, 12)), **kw) == -1
        assert call(g2=desc((2, 2, 8, 16), strides=(512, 256, 32, 1)), **kw) == -1
        assert call(g3=desc((2, 9, 8, 16)), **kw) == -1
        assert call(g3=desc((2, 16, 8, 16), strides=(4096, 256, 32, 1)), **kw) == -1
        # a tap count that is not a square (with its gradient of the same shape)
        for k in (15, 8, 0):
            assert call(taps=desc((2, k, 8, 16)), g3=desc((2, k, 8, 16)), **kw) == -1, k
            assert call(taps=desc((2, k, 8, 16)), g3=desc((2, k, 8, 16)), g1=None, **kw) == -1, k
        # null data
        assert call(taps=desc((2, 16, 8, 16), data=0), **kw) == -1
        assert call(in1=desc((2, 3, 8, 16), data=0), **kw) == -1
        assert call(gout=desc((2, 3, 8, 16), data=0), g1=None, **kw) == -1
        assert call(g3=desc((2, 16, 8, 16), data=0), **kw) == -1
        # a w-stride other than 1
        assert call(in1=desc((2, 3, 8, 16), strides=(768, 256, 32, 2)), **kw) == -1
        assert call(taps=desc((2, 16, 8, 16), strides=(4096, 256, 32, 2)), **kw) == -1
        # strides beyond int32
        assert call(in1=desc((2, 3, 8, 16), strides=(1 << 33, 128, 16, 1)), **kw) == -1
        assert call(g2=desc((2, 2, 8, 16), strides=(256, 1 << 32, 16, 1)), **kw) == -1
        # a gradinput1 that is not of input1's shape or layout
        assert call(g1=desc((2, 3, 8, 12)), **kw) == -1
        assert call(g1=desc((2, 4, 8, 16)), **kw) == -1
        assert call(g1=desc((2, 3, 8, 16), strides=(800, 200, 20, 1)), **kw) == -1
    assert lib.memc_mx_grad_last_kernel_path() == b""     # nothing was enqueued


@pytest.mark.parametrize("case", MX.uncovered(), ids=[c[0] for c in MX.uncovered()])
def test_calls_outside_the_coverage_are_declined(lib, case):
    """tests/test_mx_abi.py's uncovered calls: return code 1 with and without gradinput1, nothing touched"""
    _label, C, taps, W, tap_ptr, tap_row = case
    B, H = 2, 8
    row = tap_row or W
    tap_strides = (taps * H * row, H * row, row, 1)
    c = Call(lib, C=C, H=H, W=W, taps=taps)
    k = desc((B, taps, H, W), data=tap_ptr, strides=tap_strides)
    g3 = desc((B, taps, H, W), strides=tap_strides)       # of the taps' layout, on a quad itself
    for tdt, fdt in PAIRS:
        assert c(tdt, fdt, taps=k, g3=g3) == 1
        assert c(tdt, fdt, taps=k, g3=g3, g1=None) == 1
    assert lib.memc_mx_grad_last_kernel_path() == b""     # nothing was enqueued


def test_empty_batch_is_a_no_op(lib):
    P = ctypes.byref
    e = lambda c: desc((0, c, 8, 16), data=0)      # noqa: E731
    f = lib.FilterInterpolationLayer_gpu_backward_mx
    for taps, fl in PAIRS:
        assert f(None, taps, fl, P(e(3)), P(e(2)), P(e(16)), P(e(3)), P(e(3)), P(e(2)), P(e(16))) == 0
        assert f(None, taps, fl, P(e(3)), P(e(2)), P(e(16)), P(e(3)), None, P(e(2)), P(e(16))) == 0
    assert lib.memc_mx_grad_last_kernel_path() == b""     # nothing was launched


def test_no_mixed_backward_kernel_spills():
    """The compiler's own resource remarks: the eight instantiations by name -- 2 tap dtypes x 2 flow dtypes x (with,
    without the image gradient) -- no private scratch, no dynamic stack, the fp32 kernel's two workgroups of 256 lanes per
    CU (occupancy of at least 2 waves per SIMD)."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    from tools import kernel_resources as KR
    kernels = KR.resources_of(UNIT)
    names = sorted(k["name"] for k in kernels)
    want = sorted("memc::fi_bwd_c3_mx<memc::%s, memc::%s, %d>" % (t, f, part)
                  for t in ("F16", "BF16") for f in ("F32", t) for part in (0, 2))
    assert names == want, names
    bad = [(k["name"], k.get("scratch"), k.get("dynstack"), k.get("occupancy")) for k in kernels
           if int(k.get("scratch", "0")) > 0 or k.get("dynstack", "False") != "False" or int(k.get("occupancy", "0")) < 2]
    assert not bad, bad
    assert UNIT in KR.SOURCES


def test_the_half_backward_library_keeps_its_kernels():
    """tests/test_lowp_grad_abi.py's own kernel check for libmemc_hip_lp_grad.so: the shared kernel body instantiates there
    what it did"""
    LPG.test_no_lowp_grad_kernel_spills()
