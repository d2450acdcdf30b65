"""The fp16 / bf16 library libmemc_hip_lp.so (include/memc_warp_lp.h): loads without a GPU, exports exactly its header,
rejects malformed descriptors with -1 before touching the device, and none of its kernels spills.  CPU only -- no kernel
is launched here."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "memc_warp_lp.h")
LIB = os.path.join(ROOT, "memc-net_amd", "lib", "libmemc_hip_lp.so")
F32, F16, BF16 = 0, 1, 2


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(names) == sorted(["memc_lp_version", "memc_lp_last_kernel_path", "FilterInterpolationLayer_gpu_forward_lp",
                                    "FilterInterpolationBlendLayer_gpu_forward_lp"]), names
    return names


class Tensor4(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("size", ctypes.c_int64 * 4), ("stride", ctypes.c_int64 * 4)]


def desc(shape, data=0x1000, strides=None):
    t = Tensor4()
    t.data = data
    n, c, h, w = shape
    st = strides or (c * h * w, h * w, w, 1)
    for i in range(4):
        t.size[i] = shape[i]
        t.stride[i] = st[i]
    return t


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(LIB)
    L.memc_lp_version.restype = ctypes.c_char_p
    L.memc_lp_last_kernel_path.restype = ctypes.c_char_p
    for name, n in (("FilterInterpolationLayer_gpu_forward_lp", 4), ("FilterInterpolationBlendLayer_gpu_forward_lp", 9)):
        f = getattr(L, name)
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(Tensor4)] * n
    return L


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {p[2]: p[1] for p in (line.split() for line in out.splitlines()) if len(p) == 3}


def _is_hip_plumbing(name):
    return name.startswith("_ZN4memc") or name.startswith("__hip_")


def test_loads_without_a_gpu_and_identifies_itself(lib):
    assert lib.memc_lp_version().startswith(b"memc_hip_lp") and b"gfx950" in lib.memc_lp_version()
    assert lib.memc_lp_last_kernel_path() == b""          # no call made by this thread yet


def test_exports_exactly_the_header(lib):
    syms = _exported(LIB)
    c_surface = sorted(n for n in syms if not _is_hip_plumbing(n))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    assert any("fi_fwd_lp_tiled" in k for k in kernels) and any("fi_blend_lp_tiled" in k for k in kernels)
    # a library of its own: none of the fp32 product's kernels or entry points
    assert not [n for n in syms if "fi_fwd_tiled_fs4" in n or n == "FilterInterpolationLayer_gpu_forward"]


def test_forward_rejects_bad_descriptors(lib):
    P = ctypes.byref
    f = lib.FilterInterpolationLayer_gpu_forward_lp
    x, flow, filt, out = desc((2, 3, 8, 8)), desc((2, 2, 8, 8)), desc((2, 16, 8, 8)), desc((2, 3, 8, 8))
    # payload dtype: fp32 (the fp32 library's business) or no dtype at all; flow neither fp32 nor the payload's
    for payload, fl in ((F32, F32), (3, F32), (-1, F16), (F16, BF16), (BF16, F16), (F16, 7)):
        assert f(None, payload, fl, P(x), P(flow), P(filt), P(out)) == -1, (payload, fl)
    for payload, fl in ((F16, F32), (BF16, F32)):
        # flow with 3 channels, wrong batch, wrong height; taps of another size; output of another shape / layout
        assert f(None, payload, fl, P(x), P(desc((2, 3, 8, 8))), P(filt), P(out)) == -1
        assert f(None, payload, fl, P(x), P(desc((1, 2, 8, 8))), P(filt), P(out)) == -1
        assert f(None, payload, fl, P(x), P(desc((2, 2, 7, 8))), P(filt), P(out)) == -1
        assert f(None, payload, fl, P(x), P(flow), P(desc((2, 16, 8, 9))), P(out)) == -1
        assert f(None, payload, fl, P(x), P(flow), P(filt), P(desc((2, 3, 8, 4)))) == -1
        assert f(None, payload, fl, P(x), P(flow), P(filt), P(desc((2, 3, 8, 8), strides=(400, 100, 10, 1)))) == -1
        # w-stride != 1, a null pointer, strides beyond int32
        assert f(None, payload, fl, P(desc((2, 3, 8, 8), strides=(384, 128, 16, 2))), P(flow), P(filt), P(out)) == -1
        assert f(None, payload, fl, P(desc((2, 3, 8, 8), data=0)), P(flow), P(filt), P(out)) == -1
        assert f(None, payload, fl, P(desc((2, 3, 8, 8), strides=(1 << 33, 64, 8, 1))), P(flow), P(filt), P(out)) == -1


def test_blend_rejects_bad_descriptors(lib):
    P = ctypes.byref
    f = lib.FilterInterpolationBlendLayer_gpu_forward_lp
    x, fl, k, oc, out = desc((2, 3, 8, 8)), desc((2, 2, 8, 8)), desc((2, 16, 8, 8)), desc((2, 1, 8, 8)), desc((2, 3, 8, 8))

    def call(payload, flow_dt, *t):
        return f(None, payload, flow_dt, *(P(a) for a in t))

    assert call(F32, F32, x, x, fl, fl, k, k, oc, oc, out) == -1
    assert call(F16, BF16, x, x, fl, fl, k, k, oc, oc, out) == -1
    assert call(9, F32, x, x, fl, fl, k, k, oc, oc, out) == -1
    assert call(F16, F32, x, x, fl, fl, k, k, desc((2, 3, 8, 8)), desc((2, 3, 8, 8)), out) == -1     # occlusion channels
    assert call(F16, F32, x, desc((2, 3, 8, 4)), fl, fl, k, k, oc, oc, out) == -1                   # input2 shape
    assert call(BF16, F32, x, x, fl, desc((2, 2, 8, 4)), k, k, oc, oc, out) == -1                   # flow1 shape
    assert call(BF16, BF16, x, x, fl, fl, k, desc((1, 16, 8, 8)), oc, oc, out) == -1                # filter1 batch


def test_empty_batch_is_a_no_op(lib):
    P = ctypes.byref
    e = lambda c: desc((0, c, 8, 8), data=0)      # noqa: E731
    for payload, fl in ((F16, F32), (F16, F16), (BF16, F32), (BF16, BF16)):
        assert lib.FilterInterpolationLayer_gpu_forward_lp(None, payload, fl, P(e(3)), P(e(2)), P(e(16)), P(e(3))) == 0
        assert lib.FilterInterpolationBlendLayer_gpu_forward_lp(
            None, payload, fl, P(e(3)), P(e(3)), P(e(2)), P(e(2)), P(e(16)), P(e(16)), P(e(1)), P(e(1)), P(e(3))) == 0


def test_no_lowp_kernel_spills():
    """The compiler's own resource remarks for every kernel of the new source: no private scratch, no dynamic stack."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    sys.path.insert(0, ROOT)
    from tools import kernel_resources as KR
    kernels = KR.resources_of("lp_filter_interpolation.hip")
    names = [k["name"] for k in kernels]
    # 4 (payload, flow) pairs x (RGB, C % 4 == 0, ragged C) forward + blend, and the two one-lane-per-site kernels each
    assert len(kernels) == 4 * 6, names
    bad = [(k["name"], k.get("scratch"), k.get("dynstack")) for k in kernels
           if int(k.get("scratch", "0")) > 0 or k.get("dynstack", "False") != "False"]
    assert not bad, bad
