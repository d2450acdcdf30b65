"""The fp16 / bf16 backward library libmemc_hip_lp_grad.so (include/memc_warp_lp_grad.h): loads without a GPU, exports
exactly its header and none of the fp32 or forward libraries' entry points, rejects malformed descriptors with -1 and
declines uncovered shapes with 1 -- both before touching the device -- and its kernels do not spill.  CPU only: no kernel
is launched here (every descriptor points at a fake address, which only a launch would touch)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "memc_warp_lp_grad.h")
LIB = os.path.join(ROOT, "memc-net_amd", "lib", "libmemc_hip_lp_grad.so")
LIB_FP32 = os.path.join(ROOT, "memc-net_amd", "lib", "libmemc_hip.so")
LIB_LP = os.path.join(ROOT, "memc-net_amd", "lib", "libmemc_hip_lp.so")
F32, F16, BF16 = 0, 1, 2
NAMES = ["memc_lp_grad_version", "memc_lp_grad_last_kernel_path", "FilterInterpolationLayer_gpu_backward_lp"]


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(names) == sorted(NAMES), names
    return names


class Tensor4(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("size", ctypes.c_int64 * 4), ("stride", ctypes.c_int64 * 4)]


def desc(shape, data=0x10000, strides=None):
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
    L.memc_lp_grad_version.restype = ctypes.c_char_p
    L.memc_lp_grad_last_kernel_path.restype = ctypes.c_char_p
    f = L.FilterInterpolationLayer_gpu_backward_lp
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(Tensor4)] * 7
    return L


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {p[2]: p[1] for p in (line.split() for line in out.splitlines()) if len(p) == 3}


def _is_hip_plumbing(name):
    return name.startswith("_ZN4memc") or name.startswith("__hip_")


class Call:
    """One backward call: the tensors of a well-formed, covered 2 x C x H x W call, any of them replaceable."""

    def __init__(self, lib, C=3, H=8, W=16, taps=16):
        self.f = lib.FilterInterpolationLayer_gpu_backward_lp
        self.t = {"in1": desc((2, C, H, W)), "flow": desc((2, 2, H, W)), "taps": desc((2, taps, H, W)),
                  "gout": desc((2, C, H, W)), "g1": desc((2, C, H, W)), "g2": desc((2, 2, H, W)),
                  "g3": desc((2, taps, H, W))}

    def __call__(self, pd=F16, fd=F32, gd=F32, **repl):
        """pd / fd / gd: the payload, flow and gradoutput dtypes; keywords in1 .. g3 replace a tensor"""
        t = dict(self.t, **repl)
        P = lambda k: None if t[k] is None else ctypes.byref(t[k])      # noqa: E731
        return self.f(None, pd, fd, gd, *(P(k) for k in ("in1", "flow", "taps", "gout", "g1", "g2", "g3")))


def test_loads_without_a_gpu_and_identifies_itself(lib):
    v = lib.memc_lp_grad_version()
    assert v.startswith(b"memc_hip_lp_grad") and b"gfx950" in v
    assert lib.memc_lp_grad_last_kernel_path() == b""     # no call made by this thread yet


def test_exports_exactly_the_header(lib):
    syms = _exported(LIB)
    c_surface = sorted(n for n in syms if not _is_hip_plumbing(n))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    assert any("fi_bwd_c3_lp" in k for k in kernels), kernels
    # a library of its own: none of the fp32 library's or the half forward library's entry points or kernels
    others = {n for p in (LIB_FP32, LIB_LP) if os.path.exists(p) for n in _exported(p) if not _is_hip_plumbing(n)}
    assert "FilterInterpolationLayer_gpu_backward" in others and "FilterInterpolationLayer_gpu_forward_lp" in others
    assert not others & set(syms), others & set(syms)
    assert not [n for n in syms if "fi_bwd_c3_pk" in n or "fi_fwd_lp_tiled" in n]


def test_rejects_bad_descriptors(lib):
    call = Call(lib)
    # payload dtype not F16 / BF16; flow or gradoutput dtype neither F32 nor the payload's
    for payload, fl, go in ((F32, F32, F32), (3, F32, F32), (-1, F32, F32), (F16, BF16, F32), (BF16, F16, F32),
                            (F16, F32, BF16), (BF16, F32, F16), (F16, 7, F32), (F16, F32, 5)):
        assert call(payload, fl, go) == -1, (payload, fl, go)
    for payload, fl, go in ((F16, F32, F32), (BF16, BF16, BF16), (F16, F16, F32), (BF16, F32, BF16)):
        kw = dict(pd=payload, fd=fl, gd=go)
        # mismatched shapes: flow with 3 channels / wrong batch / height; taps of another size
        assert call(flow=desc((2, 3, 8, 16)), **kw) == -1
        assert call(flow=desc((1, 2, 8, 16)), g2=desc((1, 2, 8, 16)), **kw) == -1
        assert call(flow=desc((2, 2, 7, 16)), g2=desc((2, 2, 7, 16)), **kw) == -1
        assert call(taps=desc((2, 16, 8, 12)), g3=desc((2, 16, 8, 12)), **kw) == -1
        # gradients of another shape or layout than their inputs
        assert call(gout=desc((2, 3, 8, 12)), **kw) == -1
        assert call(gout=desc((2, 3, 8, 16), strides=(800, 200, 20, 1)), **kw) == -1
        assert call(g2=desc((2, 2, 8, 12)), **kw) == -1
        assert call(g3=desc((2, 9, 8, 16)), **kw) == -1
        assert call(g3=desc((2, 16, 8, 16), strides=(4096, 256, 32, 1)), **kw) == -1
        # a gradinput1 that is not of input1's shape (or layout)
        assert call(g1=desc((2, 3, 8, 12)), **kw) == -1
        assert call(g1=desc((2, 4, 8, 16)), **kw) == -1
        assert call(g1=desc((2, 3, 8, 16), strides=(800, 200, 20, 1)), **kw) == -1
        # a tap count that is not a square (with its gradient of the same shape)
        for k in (15, 8, 0):
            assert call(taps=desc((2, k, 8, 16)), g3=desc((2, k, 8, 16)), **kw) == -1, k
        # w-stride != 1, a null pointer, strides beyond int32
        assert call(in1=desc((2, 3, 8, 16), strides=(768, 256, 32, 2)), **kw) == -1
        assert call(taps=desc((2, 16, 8, 16), data=0), **kw) == -1
        assert call(in1=desc((2, 3, 8, 16), strides=(1 << 33, 128, 16, 1)), **kw) == -1
        assert call(g2=desc((2, 2, 8, 16), strides=(256, 1 << 32, 16, 1)), **kw) == -1
    assert lib.memc_lp_grad_last_kernel_path() == b""     # nothing was enqueued


def test_declines_uncovered_shapes(lib):
    """Return code 1: a well-formed call the kernel does not take -- nothing touched, the caller widens."""
    for payload, fl, go in ((F16, F32, F32), (BF16, BF16, BF16)):
        kw = dict(pd=payload, fd=fl, gd=go)
        assert Call(lib, C=4)(**kw) == 1                              # four channels
        assert Call(lib, W=157)(**kw) == 1                            # a ragged width
        assert Call(lib, W=4)(**kw) == 1                              # below 8
        assert Call(lib, taps=9)(**kw) == 1                           # a 3 x 3 filter
        assert Call(lib, C=4)(g1=None, **kw) == 1
        # a T view shifted by one element: its base is no longer 8-byte aligned
        c = Call(lib)
        shifted = desc((2, 3, 8, 16), data=0x10000 + 2)
        assert c(in1=shifted, **kw) == 1
        assert c(taps=desc((2, 16, 8, 16), data=0x10000 + 2), g1=None, **kw) == 1
        # ... and a row stride that is not a multiple of four elements (a T tensor)
        odd = (3 * 8 * 18, 8 * 18, 18, 1)
        assert c(in1=desc((2, 3, 8, 16), strides=odd), gout=desc((2, 3, 8, 16), strides=odd),
                 g1=desc((2, 3, 8, 16), strides=odd), **kw) == 1
    assert lib.memc_lp_grad_last_kernel_path() == b""     # nothing was enqueued


def test_empty_batch_is_a_no_op(lib):
    P = ctypes.byref
    e = lambda c: desc((0, c, 8, 16), data=0)      # noqa: E731
    for payload, fl, go in ((F16, F32, F32), (F16, F16, F16), (BF16, F32, BF16), (BF16, BF16, F32)):
        f = lib.FilterInterpolationLayer_gpu_backward_lp
        assert f(None, payload, fl, go, P(e(3)), P(e(2)), P(e(16)), P(e(3)), P(e(3)), P(e(2)), P(e(16))) == 0
        assert f(None, payload, fl, go, P(e(3)), P(e(2)), P(e(16)), P(e(3)), None, P(e(2)), P(e(16))) == 0
    assert lib.memc_lp_grad_last_kernel_path() == b""     # nothing was launched


def test_no_lowp_grad_kernel_spills():
    """The compiler's own resource remarks for every kernel of the new source: no private scratch, no dynamic stack, and
    the fp32 kernel's two workgroups per CU (at most 256 VGPRs for 256 lanes: occupancy 2)."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    sys.path.insert(0, ROOT)
    from tools import kernel_resources as KR
    kernels = KR.resources_of("lp_fi_bwd_c3.hip")
    names = [k["name"] for k in kernels]
    # 2 payloads x 2 flow dtypes x 2 gradoutput dtypes x (with, without the image gradient)
    assert len(kernels) == 2 * 2 * 2 * 2, names
    assert all("fi_bwd_c3_lp" in n for n in names), names
    bad = [(k["name"], k.get("scratch"), k.get("dynstack")) for k in kernels
           if int(k.get("scratch", "0")) > 0 or k.get("dynstack", "False") != "False"]
    assert not bad, bad
    assert all(int(k.get("occupancy", "0")) >= 2 for k in kernels), [(k["name"], k.get("occupancy")) for k in kernels]
