"""The half-precision SPyNet pyramid-level library libmemc_hip_spynet_lp.so (include/memc_spynet_lp.h): loads without a GPU,
exports exactly its header and shares no exported symbol with any other library, rejects malformed descriptors and dtype codes
with -1 and declines with 1 the three kinds of call it does not take (a w-stride other than 1, a plane beyond 32-bit in-plane
offsets, `out` overlapping an input -- in bytes of 2-byte elements), both before the device is touched; the binding refuses what
the C side cannot see; no kernel uses private scratch.  CPU only -- no kernel is launched here: the data pointers are made-up
numbers, which a refused or declined call never dereferences."""
import ctypes
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "memc_spynet_lp.h")
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
LIB = os.path.join(LIBDIR, "libmemc_hip_spynet_lp.so")
ENTRY = "SpyNetLevelLayer_gpu_forward_lp"
ERR, DECLINED = -1, 1
F32, F16, BF16 = 0, 1, 2                       # memc_dtype of include/memc_warp_lp.h
HALVES = (F16, BF16)
B, H, W = 2, 25, 40                            # a padded row over a coarse flow of 12 x 20


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(names) == sorted(["memc_spynet_lp_version", "memc_spynet_lp_last_kernel_path", ENTRY]), names
    return names


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {p[2] for p in (line.split() for line in out.splitlines()) if len(p) == 3}


class Tensor4(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("size", ctypes.c_int64 * 4), ("stride", ctypes.c_int64 * 4)]


def desc(shape, data, strides=None):
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
    L.memc_spynet_lp_version.restype = ctypes.c_char_p
    L.memc_spynet_lp_last_kernel_path.restype = ctypes.c_char_p
    f = getattr(L, ENTRY)
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.POINTER(Tensor4)] * 4 + [ctypes.c_int] * 2
    return L


BASES = {"first": 0x1000000, "second": 0x2000000, "coarse": 0x3000000, "out": 0x4000000}      # 16 MiB apart


def tensors(b=B, h=H, w=W, ch=None, cw=None):
    ch, cw = h // 2 if ch is None else ch, w // 2 if cw is None else cw
    shapes = {"first": (b, 3, h, w), "second": (b, 3, h, w), "coarse": (b, 2, ch, cw), "out": (b, 8, h, w)}
    return {k: desc(s, BASES[k] if b else 0) for k, s in shapes.items()}


def call(lib, dtype=BF16, flags=(0, 0), **over):
    """the entry point on a well-formed call with single things changed (a value of None: a null descriptor)"""
    size = {k: over.pop(k) for k in ("b", "h", "w", "ch", "cw") if k in over}
    t = tensors(**size)
    t.update(over)
    P = lambda d: None if d is None else ctypes.byref(d)       # noqa: E731
    return getattr(lib, ENTRY)(None, dtype, P(t["first"]), P(t["second"]), P(t["coarse"]), P(t["out"]), *flags)


def test_loads_without_a_gpu_and_identifies_itself(lib):
    assert lib.memc_spynet_lp_version() == b"memc_hip_spynet_lp 0.1 gfx950"
    assert lib.memc_spynet_lp_last_kernel_path() == b""   # no call enqueued by this thread


def test_exports_exactly_the_header_and_shares_no_symbol(lib):
    syms = exported(LIB)
    c_surface = sorted(n for n in syms if not (n.startswith("_ZN4memc") or n.startswith("__hip_")))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    kernels = sorted(n for n in syms if n.startswith("_ZN4memc"))
    assert len(kernels) == 4 and all("spynet_level_lpI" in k for k in kernels), kernels       # its own kernels only
    assert sorted(re.search(r"INS_\d(\w+?)ELb(\d)", k).groups() for k in kernels) == [
        ("BF16", "0"), ("BF16", "1"), ("F16", "0"), ("F16", "1")], kernels
    # a library of its own: no exported symbol, C or kernel, of any other library
    others = [p for p in glob.glob(os.path.join(LIBDIR, "libmemc_hip*.so")) if p != LIB]
    assert len(others) >= 19, others                       # fp32, measure, eighteen satellites
    theirs = {n for p in others for n in exported(p) if not n.startswith("__hip_")}
    for name in ("SpyNetLevelLayer_gpu_forward", "SpyNetLevelLayer_gpu_backward", "memc_spynet_version"):
        assert name in theirs, name
    assert not theirs & syms, theirs & syms


def test_an_empty_batch_passes_every_check_and_launches_nothing(lib):
    """the base call of the lists below is well formed and covered: with B == 0 it returns 0 for both dtypes, every flag pair
    and every size rule, so the codes below are due to the one thing each case changes"""
    for dtype in HALVES:
        for flags in ((0, 0), (1, 1), (0, 1), (1, 0)):
            assert call(lib, dtype, flags, b=0) == 0
        for h, w in ((24, 40), (25, 40), (24, 41), (25, 41), (2, 2), (3, 3), (2, 5), (6, 5), (8, 8)):
            assert call(lib, dtype, b=0, h=h, w=w) == 0, (h, w)
    assert lib.memc_spynet_lp_last_kernel_path() == b""


def test_rejects_other_dtype_codes(lib):
    for code in (F32, 3, -1):
        assert call(lib, code) == ERR, code
        assert call(lib, code, b=0) == ERR, code           # malformed comes before empty
        # ... and before declined
        strided = desc((B, 3, H, W), BASES["first"], strides=(3 * H * W * 2, H * W * 2, W * 2, 2))
        assert call(lib, code, first=strided) == ERR, code
    assert lib.memc_spynet_lp_last_kernel_path() == b""


@pytest.mark.parametrize("dtype", HALVES)
def test_declines_the_three_kinds_of_call_it_does_not_take(lib, dtype):
    # a w-stride other than 1, on each tensor
    shapes = {"first": (B, 3, H, W), "second": (B, 3, H, W), "coarse": (B, 2, H // 2, W // 2), "out": (B, 8, H, W)}
    for name, (n, c, h, w) in shapes.items():
        strided = desc((n, c, h, w), BASES[name], strides=(c * h * w * 2, h * w * 2, w * 2, 2))
        assert call(lib, dtype, **{name: strided}) == DECLINED, name
        transposed = desc((n, c, h, w), BASES[name], strides=(c * h * w, h * w, 1, h))
        assert call(lib, dtype, **{name: transposed}) == DECLINED, name
    # a plane beyond 32-bit in-plane offsets: (h - 1) * row stride + w > INT32_MAX; one row stride less is inside
    for name, (n, c, h, w) in shapes.items():
        row = (2 ** 31 - 1 - w) // (h - 1) + 1
        assert row <= 2 ** 31 - 1
        far = desc((n, c, h, w), BASES[name], strides=(0, 0, row, 1))
        assert call(lib, dtype, **{name: far}) == DECLINED, name
    # `out` overlapping an input: the same storage, its last element on the input's first, the input's last on its first
    out_bytes = 2 * B * 8 * H * W
    for name in ("first", "second", "coarse"):
        n, c, h, w = shapes[name]
        in_bytes = 2 * n * c * h * w
        assert call(lib, dtype, out=desc((B, 8, H, W), BASES[name])) == DECLINED, name
        assert call(lib, dtype, out=desc((B, 8, H, W), BASES[name] - out_bytes + 2)) == DECLINED, name
        assert call(lib, dtype, out=desc((B, 8, H, W), BASES[name] + in_bytes - 2)) == DECLINED, name
    assert lib.memc_spynet_lp_last_kernel_path() == b""   # nothing was enqueued


@pytest.mark.parametrize("dtype", HALVES)
def test_the_overlap_test_counts_two_byte_elements(lib, dtype):
    """The byte spans are those of 2-byte elements.  An `out` whose first byte is an input's LAST byte is declined, and so is
    one whose last byte is an input's first.  One byte further either way `out` lies clear of the input and the call is
    accepted -- which means enqueued: nothing stands between the overlap test and the launch, so a test that launches no
    kernel cannot ask for it.  The accepted side is asked on the device, on real storage:
    tests/test_gpu_spynet_level_lp.py::test_out_directly_behind_or_in_front_of_an_input_is_accepted places `out` at exactly
    an input's last byte + 1, which spans computed with sizeof(float) would decline."""
    n_in, n_out = B * 3 * H * W, B * 8 * H * W
    for name in ("first", "second"):
        base = BASES[name]
        assert call(lib, dtype, out=desc((B, 8, H, W), base + 2 * n_in - 1)) == DECLINED, name
        assert call(lib, dtype, out=desc((B, 8, H, W), base - 2 * n_out + 1)) == DECLINED, name
    n_c = B * 2 * (H // 2) * (W // 2)
    assert call(lib, dtype, out=desc((B, 8, H, W), BASES["coarse"] + 2 * n_c - 1)) == DECLINED
    assert call(lib, dtype, out=desc((B, 8, H, W), BASES["coarse"] - 2 * n_out + 1)) == DECLINED
    assert lib.memc_spynet_lp_last_kernel_path() == b""


def test_rejects_bad_descriptors(lib):
    # a null descriptor, a null data pointer
    for name in ("first", "second", "coarse", "out"):
        assert call(lib, **{name: None}) == ERR, name
    assert call(lib, first=desc((B, 3, H, W), 0)) == ERR
    assert call(lib, out=desc((B, 8, H, W), 0)) == ERR
    # channel counts
    assert call(lib, first=desc((B, 4, H, W), BASES["first"])) == ERR
    assert call(lib, second=desc((B, 1, H, W), BASES["second"])) == ERR
    assert call(lib, coarse=desc((B, 3, H // 2, W // 2), BASES["coarse"])) == ERR
    assert call(lib, out=desc((B, 6, H, W), BASES["out"])) == ERR
    # batch and sizes that do not match
    assert call(lib, second=desc((B + 1, 3, H, W), BASES["second"])) == ERR
    assert call(lib, second=desc((B, 3, H, W + 1), BASES["second"])) == ERR
    assert call(lib, coarse=desc((1, 2, H // 2, W // 2), BASES["coarse"])) == ERR
    assert call(lib, out=desc((B, 8, H + 1, W), BASES["out"])) == ERR
    assert call(lib, out=desc((B - 1, 8, H, W), BASES["out"])) == ERR
    # H not in {2h, 2h + 1}, W not in {2w, 2w + 1}; H or W below 2
    assert call(lib, ch=H // 2 - 1) == ERR                 # H == 2h + 3
    assert call(lib, ch=H // 2 + 1) == ERR                 # H == 2h - 1
    assert call(lib, cw=W // 2 + 1) == ERR
    assert call(lib, cw=W // 2 - 1) == ERR
    assert call(lib, h=1, ch=0) == ERR
    assert call(lib, w=1, cw=0) == ERR
    assert call(lib, b=0, h=1, ch=0) == ERR                # malformed comes before empty
    # sizes and strides negative or beyond int32
    assert call(lib, first=desc((B, 3, H, W), BASES["first"], strides=(1 << 33, H * W, W, 1))) == ERR
    assert call(lib, out=desc((B, 8, H, W), BASES["out"], strides=(8 * H * W, H * W, -W, 1))) == ERR
    # malformed and declined at once: malformed
    assert call(lib, first=desc((B, 4, H, W), BASES["first"], strides=(8 * H * W, 2 * H * W, 2 * W, 2))) == ERR
    assert lib.memc_spynet_lp_last_kernel_path() == b""


def test_binding_refuses_what_the_c_side_cannot_see():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_spynet_lp as L
    x = torch.zeros(1, 3, 8, 8, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="CUDA"):
        L.SpyNetLevelLayer_gpu_forward_lp(x, x, torch.zeros(1, 2, 4, 4, dtype=torch.bfloat16),
                                          torch.zeros(1, 8, 8, 8, dtype=torch.bfloat16), 0, 0)
    with pytest.raises(TypeError, match="torch.Tensor"):
        L.SpyNetLevelLayer_gpu_forward_lp(x.float().numpy(), x, x, x, 0, 0)
    assert L.__all__ == ["LIB_PATH", "lib", "version", "last_kernel_path", ENTRY]


def test_layer_keeps_the_torch_expression_on_the_cpu_whatever_native_half_says():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    from my_package.functions.SpyNetLevelLayer import SpyNetLevelLayer, _composed
    assert SpyNetLevelLayer.native_half is False
    g = torch.Generator().manual_seed(1)
    first, second = torch.rand(1, 3, 7, 9, generator=g), torch.rand(1, 3, 7, 9, generator=g)
    coarse = torch.randn(1, 2, 3, 4, generator=g)
    for dtype in (torch.bfloat16, torch.float32):
        f, s, c = first.to(dtype), second.to(dtype), coarse.to(dtype)
        layer = SpyNetLevelLayer(False, True)
        layer.native_half = True
        got = layer(f, s, c)
        assert got.dtype == dtype and torch.equal(got, _composed(f, s, c, False, True))


def test_spynet_hands_the_switch_to_the_layer(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    from networks import _spynet
    seen = []

    class Module(_spynet.SpyNetLevelModule):
        def forward(self, first, second, coarse):
            seen.append((self.f.fused, self.f.native_backward, self.f.native_half))
            return super().forward(first, second, coarse)
    monkeypatch.setattr(_spynet, "SpyNetLevelModule", Module)
    net = _spynet.SPyNet().eval()
    assert net.fused_level_half is False
    x = torch.rand(1, 3, 32, 32)
    with torch.no_grad():
        net(x, x)
        net.fused_level_half = True
        net(x, x)
    assert seen == [(True, False, False), (True, False, True)]


def test_binding_imports_without_loading_the_library():
    """in a fresh interpreter: after the import of the binding, the layer and the module no libmemc_hip_spynet_lp.so is mapped"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import my_package._ext.my_lib_spynet_lp as L\n"
            "import my_package.functions.SpyNetLevelLayer, my_package.modules.SpyNetLevelModule\n"
            "assert 'libmemc_hip_spynet' not in open('/proc/self/maps').read()\n"
            "assert L.version() == 'memc_hip_spynet_lp 0.1 gfx950'\n"
            "assert 'libmemc_hip_spynet_lp' in open('/proc/self/maps').read()\n" % os.path.join(ROOT, "memc-net_amd"))
    subprocess.run([sys.executable, "-c", code], check=True)


def test_kernels_use_no_scratch():
    """The compiler's own resource remarks: no private scratch, no dynamic stack, no LDS; at least four waves per SIMD."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    sys.path.insert(0, ROOT)
    from tools import kernel_resources as KR
    kernels = KR.resources_of("lp_spynet_level.hip")
    assert len(kernels) == 4, [k["name"] for k in kernels]
    for k in kernels:
        assert int(k.get("scratch", "0")) == 0 and k.get("dynstack", "False") == "False", k
        assert int(k.get("lds", "0")) == 0 and int(k["occupancy"]) >= 4, k
