"""The mixed-precision library libmemc_hip_mx.so (include/memc_warp_mx.h: fp32 image and output beside fp16 / bf16 taps and
occlusions): loads without a GPU, exports exactly its header, rejects malformed descriptors with -1 and declines calls
outside its coverage with 1 before touching the device, and none of its kernels spills.  CPU only -- no kernel is launched
here (every call below is rejected, declined or empty)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_lowp_abi as LP      # noqa: E402  (Tensor4, desc, the export helpers and the half library's own count)

HEADER = os.path.join(ROOT, "include", "memc_warp_mx.h")
LIB = os.path.join(ROOT, "memc-net_amd", "lib", "libmemc_hip_mx.so")
UNIT = "mx_filter_interpolation.hip"
F32, F16, BF16 = 0, 1, 2
SYMBOLS = ["memc_mx_version", "memc_mx_last_kernel_path", "FilterInterpolationLayer_gpu_forward_mx",
           "FilterInterpolationBlendLayer_gpu_forward_mx"]
desc, P = LP.desc, ctypes.byref


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
    L.memc_mx_version.restype = ctypes.c_char_p
    L.memc_mx_last_kernel_path.restype = ctypes.c_char_p
    for name, n in (("FilterInterpolationLayer_gpu_forward_mx", 4), ("FilterInterpolationBlendLayer_gpu_forward_mx", 9)):
        f = getattr(L, name)
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(LP.Tensor4)] * n
    return L


def warp(lib, taps, flow, *t):
    return lib.FilterInterpolationLayer_gpu_forward_mx(None, taps, flow, *(P(a) for a in t))


def blend(lib, taps, flow, *t):
    return lib.FilterInterpolationBlendLayer_gpu_forward_mx(None, taps, flow, *(P(a) for a in t))


def test_loads_without_a_gpu_and_identifies_itself(lib):
    assert lib.memc_mx_version() == b"memc_hip_mx 0.1 gfx950"
    assert lib.memc_mx_last_kernel_path() == b""          # no call enqueued by this thread yet


def test_exports_exactly_the_header(lib):
    syms = LP._exported(LIB)
    c_surface = sorted(n for n in syms if not LP._is_hip_plumbing(n))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    assert any("fi_fwd_mx_tiled" in k for k in kernels) and any("fi_blend_mx_tiled" in k for k in kernels)
    # a library of its own: none of the fp32 product's entry points or kernels, none of the half libraries' entry points
    assert not [n for n in syms if "fi_fwd_tiled_fs4" in n or n == "FilterInterpolationLayer_gpu_forward"
                or n == "FilterInterpolationBlendLayer_gpu_forward" or n.endswith("_lp") or "memc_lp_" in n]


def test_the_python_loader_binds_the_library():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_mx as M
    assert M.LIB_PATH == LIB
    assert M.version() == "memc_hip_mx 0.1 gfx950"
    assert M.last_kernel_path() == ""
    assert callable(M.FilterInterpolationLayer_gpu_forward_mx) and callable(M.FilterInterpolationBlendLayer_gpu_forward_mx)


def test_the_half_library_keeps_its_kernels():
    """tests/test_lowp_abi.py's own count for libmemc_hip_lp.so: the shared kernel bodies instantiate there what they did"""
    LP.test_no_lowp_kernel_spills()


def test_forward_rejects_bad_descriptors(lib):
    x, flow, filt, out = desc((2, 3, 8, 8)), desc((2, 2, 8, 8)), desc((2, 16, 8, 8)), desc((2, 3, 8, 8))
    # tap dtype: fp32 (the fp32 library's business) or no dtype at all; flow neither fp32 nor the taps'
    for taps, fl in ((F32, F32), (3, F32), (-1, F16), (F16, BF16), (BF16, F16), (F16, 7)):
        assert warp(lib, taps, fl, x, flow, filt, out) == -1, (taps, fl)
    for taps, fl in ((F16, F32), (BF16, F32), (F16, F16), (BF16, BF16)):
        # flow with 3 channels, wrong batch, wrong height; taps of another size; output of another shape / layout
        assert warp(lib, taps, fl, x, desc((2, 3, 8, 8)), filt, out) == -1
        assert warp(lib, taps, fl, x, desc((1, 2, 8, 8)), filt, out) == -1
        assert warp(lib, taps, fl, x, desc((2, 2, 7, 8)), filt, out) == -1
        assert warp(lib, taps, fl, x, flow, desc((2, 16, 8, 9)), out) == -1
        assert warp(lib, taps, fl, x, flow, filt, desc((2, 3, 8, 4))) == -1
        assert warp(lib, taps, fl, x, flow, filt, desc((2, 3, 8, 8), strides=(400, 100, 10, 1))) == -1
        # w-stride != 1, a null pointer, strides beyond int32
        assert warp(lib, taps, fl, desc((2, 3, 8, 8), strides=(384, 128, 16, 2)), flow, filt, out) == -1
        assert warp(lib, taps, fl, desc((2, 3, 8, 8), data=0), flow, filt, out) == -1
        assert warp(lib, taps, fl, x, flow, desc((2, 16, 8, 8), data=0), out) == -1
        assert warp(lib, taps, fl, desc((2, 3, 8, 8), strides=(1 << 33, 64, 8, 1)), flow, filt, out) == -1
    assert lib.memc_mx_last_kernel_path() == b""


def test_blend_rejects_bad_descriptors(lib):
    x, fl, k, oc, out = desc((2, 3, 8, 8)), desc((2, 2, 8, 8)), desc((2, 16, 8, 8)), desc((2, 1, 8, 8)), desc((2, 3, 8, 8))
    assert blend(lib, F32, F32, x, x, fl, fl, k, k, oc, oc, out) == -1
    assert blend(lib, F16, BF16, x, x, fl, fl, k, k, oc, oc, out) == -1
    assert blend(lib, 9, F32, x, x, fl, fl, k, k, oc, oc, out) == -1
    assert blend(lib, F16, F32, x, x, fl, fl, k, k, desc((2, 3, 8, 8)), desc((2, 3, 8, 8)), out) == -1   # occlusion channels
    assert blend(lib, F16, F32, x, desc((2, 3, 8, 4)), fl, fl, k, k, oc, oc, out) == -1                 # input2 shape
    assert blend(lib, BF16, F32, x, x, fl, desc((2, 2, 8, 4)), k, k, oc, oc, out) == -1                 # flow1 shape
    assert blend(lib, BF16, BF16, x, x, fl, fl, k, desc((1, 16, 8, 8)), oc, oc, out) == -1              # filter1 batch
    assert blend(lib, F16, F16, x, x, fl, fl, k, k, oc, desc((2, 1, 8, 8), strides=(128, 128, 16, 1)), out) == -1   # layouts
    assert blend(lib, F16, F32, x, x, fl, fl, k, k, oc, oc, desc((2, 3, 8, 8), strides=(400, 100, 10, 1))) == -1
    assert blend(lib, F16, F32, x, x, fl, fl, k, k, desc((2, 1, 8, 8), data=0), oc, out) == -1          # null data
    assert blend(lib, BF16, F32, x, x, fl, fl, desc((2, 16, 8, 8), strides=(2048, 128, 16, 2)), k, oc, oc, out) == -1
    assert blend(lib, BF16, F32, x, x, desc((2, 2, 8, 8), strides=(1 << 33, 64, 8, 1)), fl, k, k, oc, oc, out) == -1
    assert lib.memc_mx_last_kernel_path() == b""


def uncovered():
    """(label, C, taps, W, taps' data pointer, taps' row stride or None): well-formed calls outside the coverage"""
    return [("C=4", 4, 16, 16, 0x1000, None), ("4 taps", 3, 4, 16, 0x1000, None), ("W=23", 3, 16, 23, 0x1000, None),
            ("W=4", 3, 16, 4, 0x1000, None), ("taps base 2 bytes off", 3, 16, 16, 0x1002, None),
            ("taps row stride W+2", 3, 16, 16, 0x1000, 18)]


@pytest.mark.parametrize("case", uncovered(), ids=[c[0] for c in uncovered()])
def test_calls_outside_the_coverage_are_declined(lib, case):
    _label, C, taps, W, tap_ptr, tap_row = case
    B, H = 2, 8
    row = tap_row or W
    x, fl, out, oc = desc((B, C, H, W)), desc((B, 2, H, W)), desc((B, C, H, W)), desc((B, 1, H, W))
    k = desc((B, taps, H, W), data=tap_ptr, strides=(taps * H * row, H * row, row, 1))
    for tdt, fdt in ((F16, F32), (F16, F16), (BF16, F32), (BF16, BF16)):
        assert warp(lib, tdt, fdt, x, fl, k, out) == 1
        assert blend(lib, tdt, fdt, x, x, fl, fl, k, k, oc, oc, out) == 1
    assert lib.memc_mx_last_kernel_path() == b""          # nothing was enqueued


def test_empty_batch_is_a_no_op(lib):
    e = lambda c: desc((0, c, 8, 8), data=0)      # noqa: E731
    for taps, fl in ((F16, F32), (F16, F16), (BF16, F32), (BF16, BF16)):
        assert warp(lib, taps, fl, e(3), e(2), e(16), e(3)) == 0
        assert blend(lib, taps, fl, e(3), e(3), e(2), e(2), e(16), e(16), e(1), e(1), e(3)) == 0


def test_no_mixed_kernel_spills():
    """The compiler's own resource remarks: the eight mixed instantiations, no private scratch, no dynamic stack, two
    workgroups of 256 lanes per CU (occupancy of at least 2 waves per SIMD) as their half twins."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    from tools import kernel_resources as KR
    kernels = KR.resources_of(UNIT)
    names = sorted(k["name"] for k in kernels)
    want = sorted("memc::%s<memc::%s, memc::%s>" % (k, t, f) for k in ("fi_fwd_mx_tiled", "fi_blend_mx_tiled")
                  for t in ("F16", "BF16") for f in ("F32", t))
    assert names == want, names
    bad = [(k["name"], k.get("scratch"), k.get("dynstack"), k.get("occupancy")) for k in kernels
           if int(k.get("scratch", "0")) > 0 or k.get("dynstack", "False") != "False" or int(k.get("occupancy", "0")) < 2]
    assert not bad, bad
    assert UNIT in KR.SOURCES
