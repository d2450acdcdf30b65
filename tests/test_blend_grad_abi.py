"""The blend backward library libmemc_hip_blend_grad.so (include/memc_warp_blend_grad.h): loads without a GPU, exports
exactly its header and none of the other three libraries' entry points, rejects malformed descriptors with -1 and declines
uncovered shapes with 1 -- both before touching the device -- and its kernel does not spill.  CPU only: no kernel is
launched here (every descriptor points at a fake address, which only a launch would touch)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "memc_warp_blend_grad.h")
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
LIB = os.path.join(LIBDIR, "libmemc_hip_blend_grad.so")
OTHERS = [os.path.join(LIBDIR, n) for n in ("libmemc_hip.so", "libmemc_hip_lp.so", "libmemc_hip_lp_grad.so")]
NAMES = ["memc_blend_grad_version", "memc_blend_grad_last_kernel_path", "FilterInterpolationBlendLayer_gpu_backward"]
ORDER = ("in1", "flow", "taps", "occ", "gout", "gflow", "gtaps", "gocc")


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
    L.memc_blend_grad_version.restype = ctypes.c_char_p
    L.memc_blend_grad_last_kernel_path.restype = ctypes.c_char_p
    f = L.FilterInterpolationBlendLayer_gpu_backward
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(Tensor4)] * 8
    return L


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {p[2]: p[1] for p in (line.split() for line in out.splitlines()) if len(p) == 3}


def _is_hip_plumbing(name):
    return name.startswith("_ZN4memc") or name.startswith("__hip_")


class Call:
    """One call: the tensors of a well-formed, covered B x C x H x W call, any of them replaceable."""

    def __init__(self, lib, B=2, C=3, H=8, W=16, taps=16):
        self.f = lib.FilterInterpolationBlendLayer_gpu_backward
        self.t = {"in1": desc((B, C, H, W)), "flow": desc((B, 2, H, W)), "taps": desc((B, taps, H, W)),
                  "occ": desc((B, 1, H, W)), "gout": desc((B, C, H, W)), "gflow": desc((B, 2, H, W)),
                  "gtaps": desc((B, taps, H, W)), "gocc": desc((B, 1, H, W))}

    def __call__(self, **repl):
        t = dict(self.t, **repl)
        return self.f(None, *(None if t[k] is None else ctypes.byref(t[k]) for k in ORDER))


def test_loads_without_a_gpu_and_identifies_itself(lib):
    v = lib.memc_blend_grad_version()
    assert v.startswith(b"memc_hip_blend_grad") and b"gfx950" in v
    assert lib.memc_blend_grad_last_kernel_path() == b""     # no call enqueued by this thread yet


def test_exports_exactly_the_header(lib):
    syms = _exported(LIB)
    c_surface = sorted(n for n in syms if not _is_hip_plumbing(n))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    assert any("fi_blend_bwd_c3" in k for k in kernels), kernels
    assert not [n for n in syms if "fi_bwd_c3_pk" in n]
    # a library of its own: none of the other three libraries' C symbols
    present = [p for p in OTHERS if os.path.exists(p)]
    assert len(present) == len(OTHERS), present
    others = {n for p in present for n in _exported(p) if not _is_hip_plumbing(n)}
    assert {"FilterInterpolationLayer_gpu_backward", "FilterInterpolationBlendLayer_gpu_forward",
            "FilterInterpolationLayer_gpu_forward_lp", "FilterInterpolationLayer_gpu_backward_lp"} <= others
    assert not others & set(syms), others & set(syms)


def test_rejects_bad_descriptors_before_the_device(lib):
    call = Call(lib)
    # null data (each tensor in turn), a missing descriptor
    for k in ORDER:
        assert call(**{k: desc(tuple(call.t[k].size), data=0)}) == -1, k
        assert call(**{k: None}) == -1, k
    # negative or beyond-int32 sizes and strides
    assert call(in1=desc((2, 3, 8, 16), strides=(1 << 33, 128, 16, 1))) == -1
    assert call(gflow=desc((2, 2, 8, 16), strides=(256, 1 << 32, 16, 1))) == -1
    assert call(occ=desc((2, 1, 8, 16), strides=(128, 128, -16, 1))) == -1
    assert call(in1=desc((2, 3, -8, 16)), gout=desc((2, 3, -8, 16))) == -1
    assert call(in1=desc((1 << 32, 3, 8, 16)), gout=desc((1 << 32, 3, 8, 16))) == -1
    # w-stride != 1
    assert call(in1=desc((2, 3, 8, 16), strides=(768, 256, 32, 2)), gout=desc((2, 3, 8, 16), strides=(768, 256, 32, 2))) == -1
    assert call(occ=desc((2, 1, 8, 16), strides=(256, 256, 32, 2)), gocc=desc((2, 1, 8, 16), strides=(256, 256, 32, 2))) == -1
    # flow not [B, 2, H, W]
    assert call(flow=desc((2, 3, 8, 16)), gflow=desc((2, 3, 8, 16))) == -1
    assert call(flow=desc((1, 2, 8, 16)), gflow=desc((1, 2, 8, 16))) == -1
    assert call(flow=desc((2, 2, 7, 16)), gflow=desc((2, 2, 7, 16))) == -1
    assert call(flow=desc((2, 2, 8, 12)), gflow=desc((2, 2, 8, 12))) == -1
    # taps of another extent; a tap count that is not a square (with its gradient of the same shape)
    assert call(taps=desc((2, 16, 8, 12)), gtaps=desc((2, 16, 8, 12))) == -1
    for k in (15, 8, 0):
        assert call(taps=desc((2, k, 8, 16)), gtaps=desc((2, k, 8, 16))) == -1, k
    # occlusion not [B, 1, H, W]
    assert call(occ=desc((2, 2, 8, 16)), gocc=desc((2, 2, 8, 16))) == -1
    assert call(occ=desc((2, 3, 8, 16)), gocc=desc((2, 3, 8, 16))) == -1
    assert call(occ=desc((1, 1, 8, 16)), gocc=desc((1, 1, 8, 16))) == -1
    assert call(occ=desc((2, 1, 8, 12)), gocc=desc((2, 1, 8, 12))) == -1
    # gradoutput not of input's shape and layout
    assert call(gout=desc((2, 3, 8, 12))) == -1
    assert call(gout=desc((2, 4, 8, 16))) == -1
    assert call(gout=desc((2, 3, 8, 16), strides=(800, 200, 20, 1))) == -1
    # each gradient not of its input's shape and layout
    assert call(gflow=desc((2, 2, 8, 12))) == -1
    assert call(gflow=desc((2, 2, 8, 16), strides=(400, 200, 20, 1))) == -1
    assert call(gtaps=desc((2, 9, 8, 16))) == -1
    assert call(gtaps=desc((2, 16, 8, 16), strides=(4096, 256, 32, 1))) == -1
    assert call(gocc=desc((2, 2, 8, 16))) == -1
    assert call(gocc=desc((2, 1, 8, 16), strides=(200, 200, 20, 1))) == -1
    assert lib.memc_blend_grad_last_kernel_path() == b""     # nothing was enqueued


def test_declines_uncovered_shapes(lib):
    """Return code 1: a well-formed call the kernel does not take -- nothing touched, the caller composes."""
    assert Call(lib, C=5)() == 1                                  # five channels
    assert Call(lib, C=1)() == 1
    assert Call(lib, taps=9)() == 1                               # a 3 x 3 filter
    assert Call(lib, taps=25)() == 1
    assert Call(lib, W=23)() == 1                                 # a ragged width
    assert Call(lib, W=18)() == 1
    assert Call(lib, W=4)() == 1                                  # below 8
    # a plane beyond 32-bit byte offsets: rows 2^21 elements apart, 600 of them (4.7 GiB per plane)
    S, H = 1 << 21, 600
    huge = lambda c: desc((1, c, H, 16), strides=(0, H * S, S, 1))      # noqa: E731
    big = Call(lib, B=1, H=H)
    assert big(in1=huge(3), gout=huge(3)) == 1
    assert big(occ=huge(1), gocc=huge(1)) == 1
    assert big(taps=huge(16), gtaps=huge(16)) == 1
    assert big(flow=huge(2), gflow=huge(2)) == 1
    assert lib.memc_blend_grad_last_kernel_path() == b""     # nothing was enqueued


def test_empty_batch_is_a_no_op(lib):
    e = lambda c: desc((0, c, 8, 16), data=0)      # noqa: E731
    assert Call(lib)(in1=e(3), flow=e(2), taps=e(16), occ=e(1), gout=e(3), gflow=e(2), gtaps=e(16), gocc=e(1)) == 0
    assert lib.memc_blend_grad_last_kernel_path() == b""     # nothing was launched


def test_blend_grad_kernel_does_not_spill():
    """The compiler's own resource remarks for every kernel of the new source: no private scratch, no dynamic stack, and
    two workgroups of 256 lanes per CU (at most 256 VGPRs: occupancy 2), as for fi_bwd_c3_pk."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    sys.path.insert(0, ROOT)
    from tools import kernel_resources as KR
    kernels = KR.resources_of("fi_blend_bwd_c3.hip")
    names = [k["name"] for k in kernels]
    assert kernels and all("fi_blend_bwd_c3" in n for n in names), names
    bad = [(k["name"], k.get("scratch"), k.get("dynstack")) for k in kernels
           if int(k.get("scratch", "0")) > 0 or k.get("dynstack", "False") != "False"]
    assert not bad, bad
    assert all(int(k.get("occupancy", "0")) >= 2 for k in kernels), [(k["name"], k.get("occupancy")) for k in kernels]
    assert all(int(k.get("vgprs", "999")) <= 256 for k in kernels), [(k["name"], k.get("vgprs")) for k in kernels]
