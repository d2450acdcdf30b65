"""The fp16 / bf16 frame I/O library libmemc_hip_video_lp.so (include/memc_video_lp.h): loads without a GPU, names itself,
exports exactly its header and nothing of the other libraries (libmemc_hip_video.so among them), returns -1 for every failed
check and 0 for an empty call before touching the device; its Python door takes half CUDA planes only.  CPU only: no kernel
is launched (every pointer is a fake address, which only a launch would touch)."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "memc_video_lp.h")
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
LIB = os.path.join(LIBDIR, "libmemc_hip_video_lp.so")
NAMES = ["memc_video_lp_version", "memc_i420_decode_lp", "memc_rgb_quantise_lp"]
P, I, L64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
FAKE = 0x10000


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(LIB)
    L.memc_video_lp_version.restype = ctypes.c_char_p
    L.memc_i420_decode_lp.argtypes = [P, P, I, I, I, P, P, I, L64, L64, L64, I, I, I, I]
    L.memc_rgb_quantise_lp.argtypes = [P, P, I, L64, L64, L64, I, I, I, P]
    return L


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {p[2] for p in (line.split() for line in out.splitlines()) if len(p) == 3}


def _is_hip_plumbing(name):
    return name.startswith("_ZN4memc") or name.startswith("__hip_")


def test_loads_without_a_gpu_and_names_itself(lib):
    assert lib.memc_video_lp_version() == b"memc_hip_video_lp 0.1 gfx950"


def test_the_header_includes_no_other_header_of_its_directory():
    includes = re.findall(r'#\s*include\s*[<"]([^>"]+)[>"]', open(HEADER).read())
    assert sorted(includes) == ["stddef.h", "stdint.h"], includes


def test_exports_exactly_the_header(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+|size_t\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(NAMES), declared
    syms = _exported(LIB)
    assert sorted(n for n in syms if not _is_hip_plumbing(n)) == sorted(NAMES)
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    for k in ("i420_decode_lp", "rgb_quantise_lp"):
        assert sum(k in n for n in kernels) == 2, (k, kernels)         # one instance per dtype
    # a library of its own: no symbol, C or kernel, of any other library
    others = [p for p in glob.glob(os.path.join(LIBDIR, "libmemc_hip*.so")) if p != LIB]
    assert len(others) >= 10, others                                   # the product, the measurement build, the other nine satellites
    assert os.path.join(LIBDIR, "libmemc_hip_video.so") in others
    shared = {n for p in others for n in _exported(p) if not n.startswith("__hip_")} & syms
    assert not shared, shared


def test_the_python_loader_binds_the_library(lib):
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_video_lp as V
    assert V.LIB_PATH == LIB
    assert V.version() == "memc_hip_video_lp 0.1 gfx950"
    assert V.lib() is V.lib()
    assert sorted(V.__all__) == sorted(["LIB_PATH", "lib", "version", "frame_bytes", "i420_decode", "rgb_quantise"])


class Calls:
    """The two entry points on fake addresses, every argument replaceable by keyword."""

    def __init__(self, lib):
        self.lib = lib

    def decode(self, i420=FAKE, frames=2, h=6, w=10, rgb=FAKE, planes=FAKE, dtype=2, sf=3 * 70 * 138, sc=70 * 138, sr=138,
               pl=64, pr=64, pt=32, pb=32):
        return self.lib.memc_i420_decode_lp(None, i420, frames, h, w, rgb, planes, dtype, sf, sc, sr, pl, pr, pt, pb)

    def quantise(self, planes=FAKE, dtype=2, sf=3 * 70 * 138, sc=70 * 138, sr=138, frames=2, h=6, w=10, rgb=FAKE):
        return self.lib.memc_rgb_quantise_lp(None, planes, dtype, sf, sc, sr, frames, h, w, rgb)


def test_failed_checks_return_minus_one_before_the_device(lib):
    c = Calls(lib)
    for f in (c.decode, c.quantise):
        for bad in (dict(h=5), dict(w=9), dict(h=0), dict(w=0), dict(h=-6), dict(w=-10), dict(frames=-1),
                    dict(h=32770), dict(w=32770), dict(h=5, frames=0), dict(w=-10, frames=0)):
            assert f(**bad) == -1, (f.__name__, bad)
        # the dtype: 1 and 2 alone, checked before frames == 0 is let through and whatever the pointers are
        for dtype in (0, 3, -1):
            assert f(dtype=dtype) == -1, (f.__name__, dtype)
            assert f(dtype=dtype, frames=0) == -1, (f.__name__, dtype)
        assert f(dtype=0, planes=None, rgb=None) == -1
    assert c.decode(dtype=3, planes=None) == -1                    # without planes the dtype still has to be one
    # null pointers, each in turn
    assert c.decode(i420=None) == -1
    assert c.decode(rgb=None, planes=None) == -1                   # neither output
    for k in ("planes", "rgb"):
        assert c.quantise(**{k: None}) == -1, k
    # negative pads, each in turn (with and without the RGB output)
    for k in ("pl", "pr", "pt", "pb"):
        assert c.decode(**{k: -1}) == -1, k
        assert c.decode(rgb=None, **{k: -1}) == -1, k
        assert c.decode(frames=0, **{k: -1}) == -1, k
    # strides that cannot hold the extent
    assert c.decode(sr=137) == -1 and c.decode(sc=0) == -1 and c.decode(sf=-1) == -1 and c.decode(sf=0) == -1
    assert c.decode(sr=0) == -1 and c.decode(sc=-5) == -1
    assert c.quantise(sr=9) == -1 and c.quantise(sc=0) == -1 and c.quantise(sf=0) == -1 and c.quantise(sr=-138) == -1


def test_an_empty_call_is_a_no_op(lib):
    c = Calls(lib)
    for dtype in (1, 2):
        assert c.decode(frames=0, dtype=dtype) == 0 and c.decode(frames=0, rgb=None, dtype=dtype) == 0
        assert c.decode(frames=0, planes=None, dtype=dtype) == 0
        assert c.quantise(frames=0, dtype=dtype) == 0
        # an empty tensor has no address
        assert c.decode(frames=0, i420=None, rgb=None, planes=None, dtype=dtype) == 0
        assert c.quantise(frames=0, planes=None, rgb=None, dtype=dtype) == 0


def test_the_binding_takes_half_cuda_planes_only(lib):
    """every refusal is raised before the library is called: no tensor here lives on a device"""
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import torch
    import my_package._ext.my_lib_video_lp as V
    h, w = 2, 2
    i420 = torch.zeros(V.frame_bytes(h, w), dtype=torch.uint8)
    rgb = torch.zeros((1, h, w, 3), dtype=torch.uint8)
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        planes = torch.zeros((1, 3, h, w), dtype=dtype)
        with pytest.raises(TypeError):          # CPU tensors: the kernels have no CPU path
            V.i420_decode(i420, 1, h, w, planes=planes)
        with pytest.raises(TypeError):
            V.rgb_quantise(planes, rgb)
    with pytest.raises(TypeError):
        V.rgb_quantise(torch.zeros((3, h, w), dtype=torch.float16), rgb)        # not 4-D
    with pytest.raises(TypeError):
        V.rgb_quantise(None, rgb)
    # what comes after the device check, on stand-ins that say they live on one
    class OnDevice(torch.Tensor):
        is_cuda = True
    def on_device(t):
        return t.as_subclass(OnDevice)
    for dtype in (torch.float16, torch.bfloat16):
        good = on_device(torch.zeros((1, 3, h, w), dtype=dtype))
        assert V._planes(good, "planes", 1, h, w, None) == ({torch.float16: 1, torch.bfloat16: 2}[dtype], 3 * h * w, h * w, w)
        with pytest.raises(TypeError):          # a w-stride other than 1
            V._planes(on_device(torch.zeros((1, 3, h, 2 * w), dtype=dtype)[:, :, :, ::2]), "planes", 1, h, w, None)
        with pytest.raises(TypeError):
            V._planes(on_device(torch.zeros((1, 3, w, h), dtype=dtype).transpose(2, 3)), "planes", 1, h, w, None)
        with pytest.raises(ValueError):         # another shape than stated
            V._planes(good, "planes", 1, h + 2, w, None)
    with pytest.raises(TypeError):              # this door is half only
        V._planes(on_device(torch.zeros((1, 3, h, w), dtype=torch.float32)), "planes", 1, h, w, None)
    with pytest.raises(TypeError):
        V._planes(on_device(torch.zeros((1, 3, h, w), dtype=torch.float64)), "planes", 1, h, w, None)
