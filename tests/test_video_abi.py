"""The frame I/O library libmemc_hip_video.so (include/memc_video.h): loads without a GPU, names itself, exports exactly its
header and nothing of the other libraries, returns -1 for every failed check and 0 for an empty call before touching the
device, and sizes its workspace monotonically.  Its per-pixel arithmetic (csrc/memc_video_math.hpp) is plain C++: built
here with the host compiler, it gives numpy's bytes for every triple of a sample of the 2^24 and carries the matrices of
networks/yuv_io.py bit for bit.  CPU only: no kernel is launched (every pointer is a fake address, which only a launch
would touch)."""
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
HEADER = os.path.join(ROOT, "include", "memc_video.h")
CSRC = os.path.join(ROOT, "memc-net_amd", "csrc")
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
LIB = os.path.join(LIBDIR, "libmemc_hip_video.so")
NAMES = ["memc_video_version", "memc_i420_decode", "memc_rgb_quantise", "memc_i420_encode",
         "memc_luma_score_workspace_bytes", "memc_luma_score"]
P, I, L64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
FAKE = 0x10000


def _yuv_io():
    spec = importlib.util.spec_from_file_location("_video_abi_yuv_io", os.path.join(ROOT, "memc-net_amd", "networks", "yuv_io.py"))
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
    L.memc_video_version.restype = ctypes.c_char_p
    L.memc_i420_decode.argtypes = [P, P, I, I, I, P, P, L64, L64, L64, I, I, I, I]
    L.memc_rgb_quantise.argtypes = [P, P, L64, L64, L64, I, I, I, P]
    L.memc_i420_encode.argtypes = [P, P, I, I, I, P]
    L.memc_luma_score.argtypes = [P, P, P, I, I, I, P, P, ctypes.c_size_t]
    L.memc_luma_score_workspace_bytes.argtypes = [I, I, I]
    L.memc_luma_score_workspace_bytes.restype = ctypes.c_size_t
    return L


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {p[2] for p in (line.split() for line in out.splitlines()) if len(p) == 3}


def _is_hip_plumbing(name):
    return name.startswith("_ZN4memc") or name.startswith("__hip_")


def test_loads_without_a_gpu_and_names_itself(lib):
    assert lib.memc_video_version() == b"memc_hip_video 0.1 gfx950"


def test_exports_exactly_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+|size_t\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(NAMES), declared
    syms = _exported(LIB)
    assert sorted(n for n in syms if not _is_hip_plumbing(n)) == sorted(NAMES)
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    for k in ("i420_decode", "rgb_quantise", "i420_encode", "luma_partial", "luma_final"):
        assert any(k in n for n in kernels), (k, kernels)
    # a library of its own: no symbol, C or kernel, of any other library
    others = [p for p in glob.glob(os.path.join(LIBDIR, "libmemc_hip*.so")) if p != LIB]
    assert len(others) >= 7, others
    shared = {n for p in others for n in _exported(p) if not n.startswith("__hip_")} & syms
    assert not shared, shared


def test_the_python_loader_binds_the_library():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_video as V
    assert V.LIB_PATH == LIB
    assert V.version() == "memc_hip_video 0.1 gfx950"
    assert V.luma_score_workspace_bytes(1, 720, 1280) > 0
    import torch
    with pytest.raises(TypeError):              # a CPU tensor: the kernels have no CPU path
        V.i420_encode(torch.zeros(2 * 2 * 3, dtype=torch.uint8), 1, 2, 2, torch.zeros(6, dtype=torch.uint8))


class Calls:
    """The four entry points on fake addresses, every argument replaceable by keyword."""

    def __init__(self, lib):
        self.lib = lib

    def decode(self, i420=FAKE, frames=2, h=6, w=10, rgb=FAKE, planes=FAKE, sf=3 * 70 * 138, sc=70 * 138, sr=138, pl=64, pr=64,
               pt=32, pb=32):
        return self.lib.memc_i420_decode(None, i420, frames, h, w, rgb, planes, sf, sc, sr, pl, pr, pt, pb)

    def quantise(self, planes=FAKE, sf=3 * 70 * 138, sc=70 * 138, sr=138, frames=2, h=6, w=10, rgb=FAKE):
        return self.lib.memc_rgb_quantise(None, planes, sf, sc, sr, frames, h, w, rgb)

    def encode(self, rgb=FAKE, frames=2, h=6, w=10, i420=FAKE):
        return self.lib.memc_i420_encode(None, rgb, frames, h, w, i420)

    def score(self, a=FAKE, b=FAKE, frames=2, h=6, w=10, sums=FAKE, work=FAKE, nbytes=1 << 30):
        return self.lib.memc_luma_score(None, a, b, frames, h, w, sums, work, nbytes)


def test_failed_checks_return_minus_one_before_the_device(lib):
    c = Calls(lib)
    for f in (c.decode, c.quantise, c.encode, c.score):
        for bad in (dict(h=5), dict(w=9), dict(h=0), dict(w=0), dict(h=-6), dict(w=-10), dict(frames=-1),
                    dict(h=5, frames=0), dict(w=-10, frames=0)):
            assert f(**bad) == -1, (f.__name__, bad)
    # null pointers, each in turn
    for k in ("i420",):
        assert c.decode(**{k: None}) == -1
    assert c.decode(rgb=None, planes=None) == -1                   # neither output
    for k in ("planes", "rgb"):
        assert c.quantise(**{k: None}) == -1, k
    for k in ("rgb", "i420"):
        assert c.encode(**{k: None}) == -1, k
    for k in ("a", "b", "sums", "work"):
        assert c.score(**{k: None}) == -1, k
    # negative pads, each in turn (with and without the RGB output)
    for k in ("pl", "pr", "pt", "pb"):
        assert c.decode(**{k: -1}) == -1, k
        assert c.decode(rgb=None, **{k: -1}) == -1, k
        assert c.decode(frames=0, **{k: -1}) == -1, k
    # strides that cannot hold the extent; misaligned sums or workspace; a workspace too small
    assert c.decode(sr=137) == -1 and c.decode(sc=0) == -1 and c.decode(sf=-1) == -1
    assert c.quantise(sr=9) == -1 and c.quantise(sc=0) == -1 and c.quantise(sf=0) == -1
    assert c.score(sums=FAKE + 4) == -1 and c.score(work=FAKE + 2) == -1
    assert c.score(nbytes=lib.memc_luma_score_workspace_bytes(2, 6, 10) - 1) == -1
    assert c.score(nbytes=0) == -1


def test_an_empty_call_is_a_no_op(lib):
    c = Calls(lib)
    assert c.decode(frames=0) == 0 and c.decode(frames=0, rgb=None) == 0 and c.decode(frames=0, planes=None) == 0
    assert c.quantise(frames=0) == 0
    assert c.encode(frames=0) == 0
    assert c.score(frames=0) == 0
    # an empty tensor has no address
    assert c.decode(frames=0, i420=None, rgb=None, planes=None) == 0
    assert c.quantise(frames=0, planes=None, rgb=None) == 0
    assert c.encode(frames=0, rgb=None, i420=None) == 0
    assert c.score(frames=0, a=None, b=None, sums=None, work=None) == 0


def test_the_workspace_size_is_positive_and_monotone(lib):
    size = lib.memc_luma_score_workspace_bytes
    shapes = [(2, 2), (6, 10), (34, 130), (128, 256), (130, 128), (720, 1280), (1080, 1920), (4096, 4096), (32768, 32768)]
    for h, w in shapes:
        sizes = [size(n, h, w) for n in (0, 1, 2, 3, 8, 64)]
        assert sizes[0] > 0 and sizes[0] % 8 == 0 and sizes == sorted(sizes), (h, w, sizes)
    for n in (1, 4):
        for grow in (lambda h, w, k: (h + 2 * k, w), lambda h, w, k: (h, w + 2 * k)):
            sizes = [size(n, *grow(2, 2, k)) for k in range(0, 3000, 7)]
            assert sizes == sorted(sizes) and sizes[0] > 0
    assert size(1, 720, 1280) < 1 << 20                            # a scratch block, not a frame
    assert size(-1, 6, 10) == 0 and size(1, 5, 10) == 0 and size(1, 6, 0) == 0


def test_the_header_of_the_arithmetic_carries_yuv_io_s_matrices():
    """the float64 matrices of csrc/memc_video_math.hpp are networks/yuv_io.py's, bit for bit -- the inverse included, as this
    machine's numpy computes it"""
    Y = _yuv_io()
    text = open(os.path.join(CSRC, "memc_video_math.hpp")).read()
    for name, want in (("kYuvFromRgb", Y.YUV_FROM_RGB), ("kRgbFromYuv", Y.RGB_FROM_YUV)):
        body = re.search(name + r"\[9\]\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
        got = [float.fromhex(t) for t in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", body)]
        assert len(got) == 9
        assert np.array_equal(np.array(got).reshape(3, 3), want), name


def test_the_arithmetic_on_the_host_gives_numpy_s_bytes(tmp_path):
    """memc_video_math.hpp under the host compiler against yuv_io on 2^18 (Y, U, V) and (R, G, B) triples: every level of
    each component against every 4th of the others, the order-sensitive Y samples among them -- the chain is numpy's."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    src = tmp_path / "host.cpp"
    src.write_text("""
#include "memc_video_math.hpp"
#include <cstdio>
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    uint8_t t[3], o[6];
    while (fread(t, 1, 3, in) == 3) {
        uint8_t rgb[3];
        memc_video::decode_pixel(t[0], t[1], t[2], rgb);
        o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
        o[3] = memc_video::luma_of(t[0], t[1], t[2]);
        memc_video::chroma_of(t[0], t[1], t[2], o[4], o[5]);
        fwrite(o, 1, 6, out);
    }
    fclose(out);
    return 0;
}
""")
    exe = str(tmp_path / "host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, "-o", exe, str(src)], check=True)
    Y = _yuv_io()
    a, b = np.arange(256), np.arange(0, 256, 4)
    grids = [np.stack(np.meshgrid(*(a if i == k else b for i in range(3)), indexing="ij"), -1).reshape(-1, 3) for k in range(3)]
    t = np.concatenate(grids).astype(np.uint8).reshape(-1, 256, 3)
    t.tofile(str(tmp_path / "in.bin"))
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.fromfile(str(tmp_path / "out.bin"), dtype=np.uint8).reshape(t.shape[0], 256, 6)
    yuv = np.stack((t[..., 0] / 255.0, t[..., 1] / 255.0 - 0.5, t[..., 2] / 255.0 - 0.5), axis=-1)
    assert np.array_equal(got[..., :3], (255.0 * np.clip(Y.yuv_to_rgb(yuv), 0.0, 1.0)).astype(np.uint8))
    enc = Y.rgb_to_yuv(t / 255.0)
    assert np.array_equal(got[..., 3], (255.0 * enc[..., 0]).astype(np.uint8))
    assert np.array_equal(got[..., 4], (255.0 * np.clip(enc[..., 1] + 0.5, 0.0, 1.0)).astype(np.uint8))
    assert np.array_equal(got[..., 5], (255.0 * np.clip(enc[..., 2] + 0.5, 0.0, 1.0)).astype(np.uint8))
