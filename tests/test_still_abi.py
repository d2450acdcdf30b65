"""The still-image frame I/O library libmemc_hip_still.so (include/memc_still.h): loads without a GPU, names itself, exports
exactly its header and nothing of the other libraries, returns -1 for every failed check -- in the header's order -- and 0
for an empty call before touching the device, sizes its workspace monotonically, and admits odd heights and widths (the
point of the library: libmemc_hip_video.so refuses them).  CPU only: no kernel is launched (every pointer is a fake
address, which only a launch would touch; a call that passes every check is never made with frames > 0)."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "memc_still.h")
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
LIB = os.path.join(LIBDIR, "libmemc_hip_still.so")
NAMES = ["memc_still_version", "memc_rgb8_decode", "memc_rgb8_quantise", "memc_rgb8_score_workspace_bytes", "memc_rgb8_score"]
P, I, L64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
FAKE = 0x10000
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(LIB)
    L.memc_still_version.restype = ctypes.c_char_p
    L.memc_rgb8_decode.argtypes = [P, P, I, I, I, P, I, L64, L64, L64, I, I, I, I]
    L.memc_rgb8_quantise.argtypes = [P, P, I, L64, L64, L64, I, I, I, P]
    L.memc_rgb8_score.argtypes = [P, P, P, I, I, I, P, P, P, ctypes.c_size_t]
    L.memc_rgb8_score_workspace_bytes.argtypes = [I, I, I]
    L.memc_rgb8_score_workspace_bytes.restype = ctypes.c_size_t
    return L


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {p[2] for p in (line.split() for line in out.splitlines()) if len(p) == 3}


def _is_hip_plumbing(name):
    return name.startswith("_ZN4memc") or name.startswith("__hip_")


def test_loads_without_a_gpu_and_names_itself(lib):
    assert lib.memc_still_version() == b"memc_hip_still 0.1 gfx950"


def test_exports_exactly_the_header():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+|size_t\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(declared) == sorted(NAMES), declared
    assert not re.findall(r'#include\s+"', text)                   # no other header of include/
    syms = _exported(LIB)
    assert sorted(n for n in syms if not _is_hip_plumbing(n)) == sorted(NAMES)
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    for k in ("rgb8_decode", "rgb8_quantise", "rgb8_partial", "rgb8_final"):
        assert any(k in n for n in kernels), (k, kernels)
    # a library of its own: no symbol, C or kernel, of any other library
    others = [p for p in glob.glob(os.path.join(LIBDIR, "libmemc_hip*.so")) if p != LIB]
    assert len(others) >= 10, others
    shared = {n for p in others for n in _exported(p) if not n.startswith("__hip_")} & syms
    assert not shared, shared


def test_the_python_loader_binds_the_library():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_still as S
    assert S.LIB_PATH == LIB
    assert S.version() == "memc_hip_still 0.1 gfx950"
    assert S.rgb8_score_workspace_bytes(1, 255, 447) > 0
    import torch
    with pytest.raises(TypeError):              # a CPU tensor: the kernels have no CPU path
        S.rgb8_decode(torch.zeros((1, 3, 5, 3), dtype=torch.uint8), torch.zeros((1, 3, 3, 5)))
    with pytest.raises(TypeError):
        S.rgb8_quantise(torch.zeros((1, 3, 3, 5)), torch.zeros((1, 3, 5, 3), dtype=torch.uint8))
    with pytest.raises(TypeError):
        S.rgb8_score(torch.zeros((1, 3, 5, 3), dtype=torch.uint8), torch.zeros((1, 3, 5, 3), dtype=torch.uint8),
                     torch.zeros((1, 2), dtype=torch.int64), torch.zeros(64, dtype=torch.uint8))


class Calls:
    """The three entry points on fake addresses, every argument replaceable by keyword.  Odd h and w throughout."""

    def __init__(self, lib):
        self.lib = lib

    def decode(self, rgb=FAKE, frames=2, h=7, w=9, planes=FAKE, dtype=0, sf=3 * 71 * 137, sc=71 * 137, sr=137, pl=63, pr=65,
               pt=31, pb=33):
        return self.lib.memc_rgb8_decode(None, rgb, frames, h, w, planes, dtype, sf, sc, sr, pl, pr, pt, pb)

    def quantise(self, planes=FAKE, dtype=0, sf=3 * 71 * 137, sc=71 * 137, sr=137, frames=2, h=7, w=9, rgb=FAKE):
        return self.lib.memc_rgb8_quantise(None, planes, dtype, sf, sc, sr, frames, h, w, rgb)

    def score(self, a=FAKE, b=FAKE, frames=2, h=7, w=9, sums=FAKE, diff=FAKE, work=FAKE, nbytes=BIG):
        return self.lib.memc_rgb8_score(None, a, b, frames, h, w, sums, diff, work, nbytes)


def test_every_failed_check_returns_minus_one_before_the_device(lib):
    c = Calls(lib)
    for f in (c.decode, c.quantise, c.score):
        for bad in (dict(frames=-1), dict(h=0), dict(w=0), dict(h=-7), dict(w=-9), dict(h=32769), dict(w=32769),
                    dict(h=0, frames=0), dict(w=32769, frames=0)):
            assert f(**bad) == -1, (f.__name__, bad)
    for f in (c.decode, c.quantise):
        for dtype in (-1, 3, 7):
            assert f(dtype=dtype) == -1 and f(dtype=dtype, frames=0) == -1, (f.__name__, dtype)
    for k in ("pl", "pr", "pt", "pb"):
        for v in (-1, 32769):
            assert c.decode(**{k: v}) == -1 and c.decode(frames=0, **{k: v}) == -1, (k, v)
    # strides that cannot hold the extent (decode: the padded one, 9 + 63 + 65 = 137 wide)
    assert c.decode(sr=136) == -1 and c.decode(sc=0) == -1 and c.decode(sf=-1) == -1 and c.decode(sr=136, frames=0) == -1
    assert c.quantise(sr=8) == -1 and c.quantise(sc=0) == -1 and c.quantise(sf=0) == -1 and c.quantise(sr=8, frames=0) == -1
    # the score's grid, its workspace
    assert c.score(frames=65536) == -1
    need = lib.memc_rgb8_score_workspace_bytes(2, 7, 9)
    assert c.score(nbytes=need - 1) == -1 and c.score(nbytes=0) == -1 and c.score(nbytes=0, frames=0) == -1
    # null pointers, each in turn; misaligned sums or workspace
    for k in ("rgb", "planes"):
        assert c.decode(**{k: None}) == -1 and c.quantise(**{k: None}) == -1, k
    for k in ("a", "b", "sums", "work"):
        assert c.score(**{k: None}) == -1, k
        assert c.score(diff=None, **{k: None}) == -1, k
    assert c.score(sums=FAKE + 4) == -1 and c.score(work=FAKE + 2) == -1 and c.score(sums=FAKE + 1, diff=None) == -1


def test_the_checks_run_in_the_header_s_order(lib):
    """With frames = 0 a call that passes the checks 1 to 7 returns 0 at check 8, before the pointers are looked at: so an
    argument that fails one of 1 to 7 turns that 0 into -1 whatever the pointers are, and bad pointers alone do not."""
    c = Calls(lib)
    null = dict(rgb=None, planes=None)
    assert c.decode(frames=0, **null) == 0 and c.quantise(frames=0, **null) == 0
    assert c.score(frames=0, a=None, b=None, sums=FAKE + 1, work=FAKE + 1, diff=None) == 0      # 8 before 9 and 10
    for bad in (dict(h=0), dict(dtype=3), dict(pl=-1), dict(sr=1)):                             # 2 to 5 before 8
        assert c.decode(frames=0, **null, **bad) == -1, bad
    for bad in (dict(w=0), dict(dtype=-1), dict(sc=0)):
        assert c.quantise(frames=0, **null, **bad) == -1, bad
    assert c.score(frames=0, h=0, a=None) == -1 and c.score(frames=0, nbytes=0, a=None) == -1   # 2 and 7 before 8
    # 1 before everything: a negative frame count with every other argument bad as well
    assert c.decode(frames=-1, h=0, dtype=9, pl=-1, sr=0, **null) == -1
    # 9 before 10, and both after 7: a misaligned workspace that is large enough beside a null picture is still -1
    assert c.score(a=None, work=FAKE + 2) == -1


def test_an_empty_call_is_a_no_op(lib):
    c = Calls(lib)
    assert c.decode(frames=0) == 0 and c.quantise(frames=0) == 0 and c.score(frames=0) == 0
    for dtype in (0, 1, 2):
        assert c.decode(frames=0, dtype=dtype) == 0 and c.quantise(frames=0, dtype=dtype) == 0
    # an empty tensor has no address
    assert c.decode(frames=0, rgb=None, planes=None) == 0
    assert c.quantise(frames=0, planes=None, rgb=None) == 0
    assert c.score(frames=0, a=None, b=None, sums=None, work=None, diff=None) == 0


def test_odd_heights_and_widths_pass_the_checks(lib):
    c = Calls(lib)
    for h, w in ((1, 1), (3, 5), (7, 9), (33, 47), (255, 447), (32767, 32767), (32768, 1)):
        wide = w + 128
        assert c.decode(frames=0, h=h, w=w, sr=wide, sc=wide * (h + 64), sf=3 * wide * (h + 64)) == 0, (h, w)
        assert c.quantise(frames=0, h=h, w=w, sr=wide, sc=wide * h, sf=3 * wide * h) == 0, (h, w)
        assert c.score(frames=0, h=h, w=w) == 0, (h, w)
        assert lib.memc_rgb8_score_workspace_bytes(1, h, w) > 0, (h, w)


def test_the_workspace_size_is_positive_a_multiple_of_8_and_monotone(lib):
    size = lib.memc_rgb8_score_workspace_bytes
    shapes = [(1, 1), (3, 5), (7, 9), (34, 130), (33, 47), (255, 447), (256, 448), (480, 640), (1025, 1367), (4096, 4096),
              (32768, 32768)]
    for h, w in shapes:
        sizes = [size(n, h, w) for n in (0, 1, 2, 3, 8, 64, 65535)]
        assert sizes[0] > 0 and all(s % 8 == 0 for s in sizes) and sizes == sorted(sizes), (h, w, sizes)
    for n in (1, 4):
        for grow in (lambda h, w, k: (h + k, w), lambda h, w, k: (h, w + k)):
            sizes = [size(n, *grow(1, 1, k)) for k in range(0, 3000, 7)]
            assert sizes == sorted(sizes) and sizes[0] > 0 and all(s % 8 == 0 for s in sizes)
    assert size(16, 256, 448) < 1 << 20                            # a scratch block, not a frame
    assert size(-1, 7, 9) == 0 and size(1, 0, 9) == 0 and size(1, 7, 32769) == 0 and size(65536, 7, 9) == 0
