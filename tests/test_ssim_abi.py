"""The SSIM library libmemc_hip_ssim.so (include/memc_ssim.h): loads without a GPU, names itself, exports exactly its header
and nothing of the other libraries, returns -1 for every failed check and 0 for an empty call before touching the device,
and sizes its workspace monotonically.  Its per-window arithmetic (csrc/memc_ssim_math.hpp) is plain C++: built here with
the host compiler, it gives the bits of the numpy expression in networks/yuv_io.py on a sample of windows, and carries
that file's two constants bit for bit.  CPU only: no kernel is launched (every pointer is a fake address, which only a
launch would touch)."""
import ctypes
import glob
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "memc_ssim.h")
CSRC = os.path.join(ROOT, "memc-net_amd", "csrc")
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
LIB = os.path.join(LIBDIR, "libmemc_hip_ssim.so")
NAMES = ["memc_ssim_version", "memc_ssim_workspace_bytes", "memc_ssim_u8", "memc_ssim_luma_rgb"]
KERNELS = ["ssim_luma_planes", "ssim_tiles", "ssim_final"]
P, I, L64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
FAKE = 0x10000


def _yuv_io():
    spec = importlib.util.spec_from_file_location("_ssim_abi_yuv_io", os.path.join(ROOT, "memc-net_amd", "networks", "yuv_io.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(LIB)
    L.memc_ssim_version.restype = ctypes.c_char_p
    L.memc_ssim_workspace_bytes.argtypes = [I, I, I]
    L.memc_ssim_workspace_bytes.restype = ctypes.c_size_t
    L.memc_ssim_u8.argtypes = [P, P, P, L64, L64, I, I, I, P, P, ctypes.c_size_t]
    L.memc_ssim_luma_rgb.argtypes = [P, P, P, I, I, I, P, P, ctypes.c_size_t]
    return L


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {p[2] for p in (line.split() for line in out.splitlines()) if len(p) == 3}


def _is_hip_plumbing(name):
    return name.startswith("_ZN4memc") or name.startswith("__hip_")


def test_loads_without_a_gpu_and_names_itself(lib):
    assert lib.memc_ssim_version() == b"memc_hip_ssim 0.1 gfx950"


def test_exports_exactly_the_header(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+|size_t\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(NAMES), declared
    syms = _exported(LIB)
    assert sorted(n for n in syms if not _is_hip_plumbing(n)) == sorted(NAMES)
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    assert len(kernels) == len(KERNELS), kernels
    for k in KERNELS:
        assert any(k in n for n in kernels), (k, kernels)
    # a library of its own: no symbol, C or kernel, of any other library
    others = [p for p in glob.glob(os.path.join(LIBDIR, "libmemc_hip*.so")) if p != LIB]
    assert len(others) >= 8, others
    shared = {n for p in others for n in _exported(p) if not n.startswith("__hip_")} & syms
    assert not shared, shared


def test_the_python_loader_binds_the_library(lib):
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_ssim as S
    assert S.LIB_PATH == LIB
    assert S.version() == "memc_hip_ssim 0.1 gfx950"
    assert S.ssim_workspace_bytes(1, 720, 1280) == lib.memc_ssim_workspace_bytes(1, 720, 1280) > 0
    import torch
    planes, rgb = torch.zeros((1, 8, 10), dtype=torch.uint8), torch.zeros((1, 8, 10, 3), dtype=torch.uint8)
    out, work = torch.zeros(1, dtype=torch.float64), torch.zeros(S.ssim_workspace_bytes(1, 8, 10), dtype=torch.uint8)
    with pytest.raises(TypeError):              # CPU tensors: the kernels have no CPU path
        S.ssim_u8(planes, planes, out, work)
    with pytest.raises(TypeError):
        S.ssim_luma_rgb(rgb, rgb, 1, 8, 10, out, work)


class Calls:
    """The two entry points on fake addresses, every argument replaceable by keyword."""

    def __init__(self, lib):
        self.lib = lib

    def u8(self, a=FAKE, b=FAKE, sf=40 * 136, sr=136, frames=2, h=40, w=136, ssim=FAKE, work=FAKE, nbytes=1 << 30):
        return self.lib.memc_ssim_u8(None, a, b, sf, sr, frames, h, w, ssim, work, nbytes)

    def rgb(self, a=FAKE, b=FAKE, frames=2, h=40, w=136, ssim=FAKE, work=FAKE, nbytes=1 << 30):
        return self.lib.memc_ssim_luma_rgb(None, a, b, frames, h, w, ssim, work, nbytes)


def test_failed_checks_return_minus_one_before_the_device(lib):
    c = Calls(lib)
    need = lib.memc_ssim_workspace_bytes(2, 40, 136)
    for f in (c.u8, c.rgb):
        for bad in (dict(frames=-1), dict(h=6), dict(w=6), dict(h=0), dict(w=-136), dict(h=32769), dict(w=32769),
                    dict(frames=65536), dict(h=6, frames=0), dict(w=6, frames=0),
                    dict(nbytes=need - 1), dict(nbytes=0), dict(nbytes=8),
                    dict(a=None), dict(b=None), dict(ssim=None), dict(work=None),
                    dict(ssim=FAKE + 4), dict(work=FAKE + 2), dict(work=FAKE + 4)):
            assert f(**bad) == -1, (f.__name__, bad)
    # strides that cannot hold the extent (the planes' entry point alone takes strides)
    for bad in (dict(sr=135), dict(sr=0), dict(sr=-136), dict(sf=39 * 136 + 135), dict(sf=0), dict(sf=-1),
                dict(sr=149, sf=40 * 136), dict(sr=135, frames=0), dict(sr=(1 << 46) + 1, sf=1 << 62), dict(sf=(1 << 46) + 1)):
        assert c.u8(**bad) == -1, bad
    # the order: a failed size check wins over an empty call, an empty call over a null pointer
    assert c.u8(frames=0, h=6) == -1 and c.rgb(frames=0, w=6) == -1
    assert c.u8(frames=0, a=None) == 0 and c.rgb(frames=0, ssim=None) == 0


def test_an_empty_call_is_a_no_op(lib):
    c = Calls(lib)
    assert c.u8(frames=0) == 0 and c.rgb(frames=0) == 0
    # an empty tensor has no address; odd sizes are allowed
    assert c.u8(frames=0, a=None, b=None, ssim=None, work=None, nbytes=lib.memc_ssim_workspace_bytes(0, 40, 136)) == 0
    assert c.rgb(frames=0, a=None, b=None, ssim=None, work=None, nbytes=lib.memc_ssim_workspace_bytes(0, 40, 136)) == 0
    assert c.u8(frames=0, h=7, w=7, sr=7, sf=49) == 0 and c.rgb(frames=0, h=9, w=301) == 0
    assert c.u8(frames=0, sf=0) == 0                                # one frame or none: the frame stride is not read


def test_the_workspace_size_is_positive_and_monotone(lib):
    size = lib.memc_ssim_workspace_bytes
    shapes = [(7, 7), (34, 130), (128, 256), (130, 128), (720, 1280), (1080, 1920), (4096, 4096), (32768, 32768)]
    for h, w in shapes:
        sizes = [size(n, h, w) for n in (0, 1, 2, 3, 8, 64)]
        assert sizes[0] > 0 and all(s % 8 == 0 for s in sizes) and sizes == sorted(sizes), (h, w, sizes)
    for n in (1, 4):
        for grow in (lambda h, w, k: (h + k, w), lambda h, w, k: (h, w + k)):
            sizes = [size(n, *grow(7, 7, k)) for k in range(0, 3000, 7)]
            assert sizes == sorted(sizes) and sizes[0] > 0 and all(s % 8 == 0 for s in sizes)
    # the two luma planes of a frame and a scratch block, not more
    assert 2 * 720 * 1280 <= size(1, 720, 1280) < 2 * 720 * 1280 + (1 << 20)
    # test_video_abi's shapes below the window, and every other failed check
    for bad in ((1, 2, 2), (1, 6, 10), (1, 10, 6), (-1, 40, 136), (65536, 40, 136), (1, 32769, 7), (1, 7, 32769), (1, 0, 7)):
        assert size(*bad) == 0, bad


def test_the_header_of_the_arithmetic_carries_yuv_io_s_constants():
    """kC1 and kC2 of csrc/memc_ssim_math.hpp are the float64 values Python computes for their expressions, which are
    networks/yuv_io.py's SSIM_C1 and SSIM_C2"""
    Y = _yuv_io()
    text = open(os.path.join(CSRC, "memc_ssim_math.hpp")).read()
    for name, want, mine in (("kC1", (0.01 * 255) ** 2 * 49 ** 2, Y.SSIM_C1), ("kC2", (0.03 * 255) ** 2 * 49 * 48, Y.SSIM_C2)):
        got = float.fromhex(re.search(name + r"\s*=\s*(0x[0-9a-f.]+p[+-]\d+)\s*;", text).group(1))
        assert got.hex() == want.hex() == mine.hex(), (name, got.hex(), want.hex(), mine.hex())


SAMPLE = 1 << 16            # random windows of the arithmetic test, beside the special ones


def _windows():
    """pairs of 7 x 7 byte windows [n, 2, 49]: all-0, all-255, 24 of 49 at 255 (against itself, its complement, all-0 and
    all-255), equal random windows, exact negatives y = 255 - x, near-equal ones, and SAMPLE iid ones"""
    rng = np.random.default_rng(1749)
    zero, full = np.zeros(49, dtype=np.uint8), np.full(49, 255, dtype=np.uint8)
    part = np.where(np.arange(49) % 2 == 1, 255, 0).astype(np.uint8)          # 24 of 49 at 255
    assert int((part == 255).sum()) == 24
    special = [(zero, zero), (full, full), (zero, full), (full, zero), (part, part), (part, 255 - part), (part, zero),
               (part, full), (255 - part, full)]
    x = rng.integers(0, 256, (SAMPLE, 49), dtype=np.uint8)
    y = rng.integers(0, 256, (SAMPLE, 49), dtype=np.uint8)
    k = SAMPLE // 4
    y[:k] = x[:k]                                                             # equal
    y[k:2 * k] = 255 - x[k:2 * k]                                             # exact negatives
    y[2 * k:3 * k] = np.clip(x[2 * k:3 * k].astype(np.int16) + rng.integers(-3, 4, (k, 49)), 0, 255).astype(np.uint8)
    both = np.stack((x, y), axis=1)
    return np.concatenate([np.stack([np.stack(p) for p in special]), both]), len(special), k


def test_the_arithmetic_on_the_host_gives_numpy_s_bits(tmp_path):
    """memc_ssim_math.hpp under the host compiler against the numpy expression of S (networks/yuv_io.py::ssim_from_planes') on
    9 special and SAMPLE = 2^16 random 7 x 7 windows: the same float64 bits, and exactly 1.0 wherever the windows are equal."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "host.cpp"
    src.write_text("""
#include "memc_ssim_math.hpp"
#include <cstdio>
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    int s[5];
    while (fread(s, sizeof(int), 5, in) == 5) {
        const double v = memc_ssim::window_ssim(s[0], s[1], s[2], s[3], s[4]);
        fwrite(&v, sizeof(double), 1, out);
    }
    fclose(out);
    return 0;
}
""")
    exe = str(tmp_path / "host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, "-o", exe, str(src)], check=True)
    Y = _yuv_io()
    win, n_special, k = _windows()
    x, y = win[:, 0].astype(np.int64), win[:, 1].astype(np.int64)
    sx, sy, sxx, syy, sxy = x.sum(1), y.sum(1), (x * x).sum(1), (y * y).sum(1), (x * y).sum(1)
    assert sx.max() == 12495 and sxx.max() == 3186225                          # the largest sums are among them
    np.stack((sx, sy, sxx, syy, sxy), axis=1).astype(np.int32).tofile(str(tmp_path / "in.bin"))
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.fromfile(str(tmp_path / "out.bin"), dtype=np.float64)
    vxx, vyy, vxy = 49 * sxx - sx * sx, 49 * syy - sy * sy, 49 * sxy - sx * sy
    assert max(np.abs(v).max() for v in (vxx, vyy, vxy)) <= 255 * 255 * 600
    want = ((2 * sx * sy + Y.SSIM_C1) * (2 * vxy + Y.SSIM_C2)) / ((sx * sx + sy * sy + Y.SSIM_C1) * (vxx + vyy + Y.SSIM_C2))
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    equal = (win[:, 0] == win[:, 1]).all(axis=1)
    assert equal.sum() >= k + 3 and np.all(got[equal] == 1.0)
    assert np.all(got <= 1.0) and np.all(got >= -1.0)
    # a single window is a 7 x 7 plane: the host rule is this number
    for i in list(range(n_special)) + [n_special + 1, n_special + k + 1, len(win) - 1]:
        assert Y.ssim_from_planes(win[i, 0].reshape(7, 7), win[i, 1].reshape(7, 7)) == got[i]
