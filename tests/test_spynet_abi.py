"""The SPyNet pyramid-level library libmemc_hip_spynet.so (include/memc_spynet.h): loads without a GPU, exports exactly its
header, rejects malformed descriptors with -1 and declines with 1 the three kinds of call it does not take (a plane beyond
32-bit in-plane offsets, a w-stride other than 1, `out` overlapping an input), both before the device is touched; the
binding refuses what the C side cannot see; neither kernel uses private scratch.  CPU only -- no kernel is launched here: the
data pointers are made-up numbers, which a refused or declined call never dereferences."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "memc_spynet.h")
LIB = os.path.join(ROOT, "memc-net_amd", "lib", "libmemc_hip_spynet.so")
ENTRY = "SpyNetLevelLayer_gpu_forward"
ERR, DECLINED = -1, 1
B, H, W = 2, 25, 40                            # a padded row over a coarse flow of 12 x 20


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(names) == sorted(["memc_spynet_version", "memc_spynet_last_kernel_path", ENTRY]), names
    return names


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
    L.memc_spynet_version.restype = ctypes.c_char_p
    L.memc_spynet_last_kernel_path.restype = ctypes.c_char_p
    f = getattr(L, ENTRY)
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(Tensor4)] * 4 + [ctypes.c_int] * 2
    return L


BASES = {"first": 0x1000000, "second": 0x2000000, "coarse": 0x3000000, "out": 0x4000000}      # 16 MiB apart


def tensors(b=B, h=H, w=W, ch=None, cw=None):
    ch, cw = h // 2 if ch is None else ch, w // 2 if cw is None else cw
    shapes = {"first": (b, 3, h, w), "second": (b, 3, h, w), "coarse": (b, 2, ch, cw), "out": (b, 8, h, w)}
    return {k: desc(s, BASES[k] if b else 0) for k, s in shapes.items()}


def call(lib, flags=(0, 0), **over):
    """the entry point on a well-formed call with single things changed (a value of None: a null descriptor)"""
    size = {k: over.pop(k) for k in ("b", "h", "w", "ch", "cw") if k in over}
    t = tensors(**size)
    t.update(over)
    P = lambda d: None if d is None else ctypes.byref(d)       # noqa: E731
    return getattr(lib, ENTRY)(None, P(t["first"]), P(t["second"]), P(t["coarse"]), P(t["out"]), *flags)


def test_loads_without_a_gpu_and_identifies_itself(lib):
    assert lib.memc_spynet_version().startswith(b"memc_hip_spynet") and b"gfx950" in lib.memc_spynet_version()
    assert lib.memc_spynet_last_kernel_path() == b""      # no call enqueued by this thread


def test_exports_exactly_the_header(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    syms = {p[2] for p in (line.split() for line in out.splitlines()) if len(p) == 3}
    c_surface = sorted(n for n in syms if not (n.startswith("_ZN4memc") or n.startswith("__hip_")))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    assert any("spynet_level" in n for n in syms)
    # a library of its own: none of the fp32 product's kernels or entry points
    assert not [n for n in syms if "flow_upsample4" in n or "bl_fwd" in n or n == "InterpolationLayer_gpu_forward"]


def test_an_empty_batch_passes_every_check_and_launches_nothing(lib):
    """the base call of the lists below is well formed and covered: with B == 0 it returns 0 for every flag pair and every
    size rule (H in {2h, 2h + 1}, W in {2w, 2w + 1}), so the codes below are due to the one thing each case changes"""
    for flags in ((0, 0), (1, 1), (0, 1), (1, 0)):
        assert call(lib, flags, b=0) == 0
    for h, w in ((24, 40), (25, 40), (24, 41), (25, 41), (2, 2), (3, 3), (2, 5), (6, 5), (8, 8)):
        assert call(lib, b=0, h=h, w=w) == 0, (h, w)
    assert lib.memc_spynet_last_kernel_path() == b""


def test_declines_the_three_kinds_of_call_it_does_not_take(lib):
    # a w-stride other than 1, on each tensor
    shapes = {"first": (B, 3, H, W), "second": (B, 3, H, W), "coarse": (B, 2, H // 2, W // 2), "out": (B, 8, H, W)}
    for name, (n, c, h, w) in shapes.items():
        strided = desc((n, c, h, w), BASES[name], strides=(c * h * w * 2, h * w * 2, w * 2, 2))
        assert call(lib, **{name: strided}) == DECLINED, name
        transposed = desc((n, c, h, w), BASES[name], strides=(c * h * w, h * w, 1, h))
        assert call(lib, **{name: transposed}) == DECLINED, name
    # a plane beyond 32-bit in-plane offsets: (h - 1) * row stride + w > INT32_MAX
    for name, (n, c, h, w) in shapes.items():
        row = (2 ** 31 - 1 - w) // (h - 1) + 1
        assert row <= 2 ** 31 - 1
        far = desc((n, c, h, w), BASES[name], strides=(0, 0, row, 1))
        assert call(lib, **{name: far}) == DECLINED, name
    # `out` overlapping an input: the same storage, its last element on the input's first, the input's last on its first
    out_bytes = 4 * B * 8 * H * W
    for name in ("first", "second", "coarse"):
        n, c, h, w = shapes[name]
        in_bytes = 4 * n * c * h * w
        assert call(lib, out=desc((B, 8, H, W), BASES[name])) == DECLINED, name
        assert call(lib, out=desc((B, 8, H, W), BASES[name] - out_bytes + 4)) == DECLINED, name
        assert call(lib, out=desc((B, 8, H, W), BASES[name] + in_bytes - 4)) == DECLINED, name
    assert lib.memc_spynet_last_kernel_path() == b""      # nothing was enqueued


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
    assert lib.memc_spynet_last_kernel_path() == b""


def test_binding_refuses_what_the_c_side_cannot_see():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_spynet as L
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(TypeError, match="CUDA"):
        L.SpyNetLevelLayer_gpu_forward(x, x, torch.zeros(1, 2, 4, 4), torch.zeros(1, 8, 8, 8), 0, 0)
    with pytest.raises(TypeError, match="torch.Tensor"):
        L.SpyNetLevelLayer_gpu_forward(x.numpy(), x, x, x, 0, 0)


def test_layer_takes_the_torch_expression_on_the_cpu_and_for_other_dtypes():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    from my_package.functions.SpyNetLevelLayer import SpyNetLevelLayer, _composed
    from my_package.modules.SpyNetLevelModule import SpyNetLevelModule
    g = torch.Generator().manual_seed(1)
    first, second = torch.rand(1, 3, 7, 9, generator=g), torch.rand(1, 3, 7, 9, generator=g)
    coarse = torch.randn(1, 2, 3, 4, generator=g)
    for flags in ((False, False), (True, True), (False, True)):
        want = _composed(first, second, coarse, *flags)
        assert want.shape == (1, 8, 7, 9)
        assert torch.equal(SpyNetLevelLayer(*flags)(first, second, coarse), want)
        assert torch.equal(SpyNetLevelModule(*flags)(first, second, coarse), want)
        assert torch.equal(want[:, 0:3], first)
        assert SpyNetLevelLayer(*flags)(first.double(), second.double(), coarse.double()).dtype == torch.float64
    c = coarse.clone().requires_grad_(True)
    SpyNetLevelLayer()(first, second, c).sum().backward()
    assert c.grad is not None and c.grad.shape == coarse.shape


def test_binding_imports_without_loading_the_library():
    """in a fresh interpreter: after the import of the binding, the layer and the module no libmemc_hip_spynet.so is mapped"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import my_package._ext.my_lib_spynet as L\n"
            "import my_package.functions.SpyNetLevelLayer, my_package.modules.SpyNetLevelModule\n"
            "assert 'libmemc_hip_spynet' not in open('/proc/self/maps').read()\n"
            "assert L.version().startswith('memc_hip_spynet')\n"
            "assert 'libmemc_hip_spynet' in open('/proc/self/maps').read()\n" % os.path.join(ROOT, "memc-net_amd"))
    subprocess.run([sys.executable, "-c", code], check=True)


def test_kernels_use_no_scratch():
    """The compiler's own resource remarks: no private scratch, no dynamic stack, no LDS; at least four waves per SIMD."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    sys.path.insert(0, ROOT)
    from tools import kernel_resources as KR
    kernels = KR.resources_of("spynet_level.hip")
    assert len(kernels) == 2, [k["name"] for k in kernels]
    for k in kernels:
        assert int(k.get("scratch", "0")) == 0 and k.get("dynstack", "False") == "False", k
        assert int(k.get("lds", "0")) == 0 and int(k["occupancy"]) >= 4, k
