"""The SPyNet level backward library libmemc_hip_spynet_grad.so (include/memc_spynet_grad.h): loads without a GPU, exports
exactly its header, rejects malformed descriptors with -1 and declines with 1 the three kinds of call it does not take (a
plane beyond 32-bit in-plane offsets, a w-stride other than 1, `gradcoarse` overlapping an input), both before the device is
touched and in the forward's order (malformed, empty, declined); the binding refuses what the C side cannot see and loads
nothing at import; the kernel uses no private scratch and the LDS its box bound says; on the CPU the layer keeps the torch
expression whatever `native_backward` says.  CPU only -- no kernel is launched here: the data pointers are made-up numbers,
which a refused or declined call never dereferences."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "memc_spynet_grad.h")
LIB = os.path.join(ROOT, "memc-net_amd", "lib", "libmemc_hip_spynet_grad.so")
ENTRY = "SpyNetLevelLayer_gpu_backward"
ERR, DECLINED = -1, 1
B, H, W = 2, 25, 40                            # a padded row over a coarse flow of 12 x 20
NAMES = ("second", "coarse", "gradoutput", "gradcoarse")


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(names) == sorted(["memc_spynet_grad_version", "memc_spynet_grad_last_kernel_path", ENTRY]), names
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
    L.memc_spynet_grad_version.restype = ctypes.c_char_p
    L.memc_spynet_grad_last_kernel_path.restype = ctypes.c_char_p
    f = getattr(L, ENTRY)
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(Tensor4)] * 4 + [ctypes.c_int] * 2
    return L


BASES = {"second": 0x1000000, "coarse": 0x2000000, "gradoutput": 0x3000000, "gradcoarse": 0x4000000}      # 16 MiB apart


def shapes(b=B, h=H, w=W, ch=None, cw=None):
    ch, cw = h // 2 if ch is None else ch, w // 2 if cw is None else cw
    return {"second": (b, 3, h, w), "coarse": (b, 2, ch, cw), "gradoutput": (b, 8, h, w), "gradcoarse": (b, 2, ch, cw)}


def call(lib, flags=(0, 0), **over):
    """the entry point on a well-formed call with single things changed (a value of None: a null descriptor)"""
    size = {k: over.pop(k) for k in ("b", "h", "w", "ch", "cw") if k in over}
    t = {k: desc(s, BASES[k] if s[0] else 0) for k, s in shapes(**size).items()}
    t.update(over)
    P = lambda d: None if d is None else ctypes.byref(d)       # noqa: E731
    return getattr(lib, ENTRY)(None, *(P(t[k]) for k in NAMES), *flags)


def test_loads_without_a_gpu_and_identifies_itself(lib):
    assert lib.memc_spynet_grad_version() == b"memc_hip_spynet_grad 0.1 gfx950"
    assert lib.memc_spynet_grad_last_kernel_path() == b""      # no call enqueued by this thread


def test_exports_exactly_the_header(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    syms = {p[2] for p in (line.split() for line in out.splitlines()) if len(p) == 3}
    c_surface = sorted(n for n in syms if not (n.startswith("_ZN4memc") or n.startswith("__hip_")))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    assert any("spynet_level_bwd_tiled" in n for n in syms)
    # a library of its own: none of the forward's kernels or entry points, nor the fp32 product's
    assert not [n for n in syms if "SpyNetLevelLayer_gpu_forward" in n or "12spynet_levelI" in n or "bl_fwd" in n]
    # and the forward library keeps its surface
    fwd = subprocess.run(["nm", "-D", "--defined-only", LIB.replace("_grad", "")], stdout=subprocess.PIPE, text=True,
                         check=True).stdout
    assert "SpyNetLevelLayer_gpu_forward" in fwd and "backward" not in fwd and "spynet_level_bwd" not in fwd


def test_an_empty_batch_passes_every_check_and_launches_nothing(lib):
    """the base call of the lists below is well formed and covered: with B == 0 it returns 0 for every flag pair and every
    size rule (H in {2h, 2h + 1}, W in {2w, 2w + 1}), so the codes below are due to the one thing each case changes"""
    for flags in ((0, 0), (1, 1), (0, 1), (1, 0)):
        assert call(lib, flags, b=0) == 0
    for h, w in ((24, 40), (25, 40), (24, 41), (25, 41), (2, 2), (3, 3), (2, 5), (6, 5), (8, 8), (37, 70), (2049, 2048)):
        assert call(lib, b=0, h=h, w=w) == 0, (h, w)
    assert lib.memc_spynet_grad_last_kernel_path() == b""


def test_declines_the_three_kinds_of_call_it_does_not_take(lib):
    # a w-stride other than 1, on each tensor
    for name, (n, c, h, w) in shapes().items():
        strided = desc((n, c, h, w), BASES[name], strides=(c * h * w * 2, h * w * 2, w * 2, 2))
        assert call(lib, **{name: strided}) == DECLINED, name
        transposed = desc((n, c, h, w), BASES[name], strides=(c * h * w, h * w, 1, h))
        assert call(lib, **{name: transposed}) == DECLINED, name
    # a plane beyond 32-bit in-plane offsets: (h - 1) * row stride + w > INT32_MAX
    for name, (n, c, h, w) in shapes().items():
        row = (2 ** 31 - 1 - w) // (h - 1) + 1
        assert row <= 2 ** 31 - 1
        far = desc((n, c, h, w), BASES[name], strides=(0, 0, row, 1))
        assert call(lib, **{name: far}) == DECLINED, name
    # `gradcoarse` overlapping an input: the same storage, its last element on the input's first, the input's last on its first
    gshape = shapes()["gradcoarse"]
    out_bytes = 4 * gshape[0] * gshape[1] * gshape[2] * gshape[3]
    for name in ("second", "coarse", "gradoutput"):
        n, c, h, w = shapes()[name]
        in_bytes = 4 * n * c * h * w
        assert call(lib, gradcoarse=desc(gshape, BASES[name])) == DECLINED, name
        assert call(lib, gradcoarse=desc(gshape, BASES[name] - out_bytes + 4)) == DECLINED, name
        assert call(lib, gradcoarse=desc(gshape, BASES[name] + in_bytes - 4)) == DECLINED, name
    assert lib.memc_spynet_grad_last_kernel_path() == b""      # nothing was enqueued


def test_rejects_bad_descriptors(lib):
    # a null descriptor, a null data pointer
    for name in NAMES:
        assert call(lib, **{name: None}) == ERR, name
        assert call(lib, **{name: desc(shapes()[name], 0)}) == ERR, name
    # channel counts
    assert call(lib, second=desc((B, 4, H, W), BASES["second"])) == ERR
    assert call(lib, coarse=desc((B, 3, H // 2, W // 2), BASES["coarse"])) == ERR
    assert call(lib, gradoutput=desc((B, 5, H, W), BASES["gradoutput"])) == ERR        # the slice 3..7 is not the tensor
    assert call(lib, gradcoarse=desc((B, 1, H // 2, W // 2), BASES["gradcoarse"])) == ERR
    # batch and sizes that do not match
    assert call(lib, coarse=desc((B + 1, 2, H // 2, W // 2), BASES["coarse"])) == ERR
    assert call(lib, gradoutput=desc((B, 8, H, W + 1), BASES["gradoutput"])) == ERR
    assert call(lib, gradoutput=desc((B - 1, 8, H, W), BASES["gradoutput"])) == ERR
    assert call(lib, gradcoarse=desc((B, 2, H // 2 + 1, W // 2), BASES["gradcoarse"])) == ERR
    assert call(lib, gradcoarse=desc((1, 2, H // 2, W // 2), BASES["gradcoarse"])) == ERR
    # H not in {2h, 2h + 1}, W not in {2w, 2w + 1}; H or W below 2
    assert call(lib, ch=H // 2 - 1) == ERR                 # H == 2h + 3
    assert call(lib, ch=H // 2 + 1) == ERR                 # H == 2h - 1
    assert call(lib, cw=W // 2 + 1) == ERR
    assert call(lib, cw=W // 2 - 1) == ERR
    assert call(lib, h=1, ch=0) == ERR
    assert call(lib, w=1, cw=0) == ERR
    assert call(lib, b=0, h=1, ch=0) == ERR                # malformed comes before empty
    # sizes and strides negative or beyond int32
    assert call(lib, second=desc((B, 3, H, W), BASES["second"], strides=(1 << 33, H * W, W, 1))) == ERR
    assert call(lib, gradcoarse=desc((B, 2, H // 2, W // 2), BASES["gradcoarse"], strides=(H * W, H * W // 4, -W, 1))) == ERR
    # malformed and declined at once: malformed
    assert call(lib, second=desc((B, 4, H, W), BASES["second"], strides=(8 * H * W, 2 * H * W, 2 * W, 2))) == ERR
    assert lib.memc_spynet_grad_last_kernel_path() == b""


def test_binding_refuses_what_the_c_side_cannot_see():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_spynet_grad as L
    x, c = torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 4, 4)
    with pytest.raises(TypeError, match="CUDA"):
        L.SpyNetLevelLayer_gpu_backward(x, c, torch.zeros(1, 8, 8, 8), torch.zeros(1, 2, 4, 4), 0, 0)
    with pytest.raises(TypeError, match="torch.Tensor"):
        L.SpyNetLevelLayer_gpu_backward(x.numpy(), c, x, c, 0, 0)


def test_on_the_cpu_the_layer_keeps_the_torch_expression_whatever_native_backward_says():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    from my_package.functions.SpyNetLevelLayer import SpyNetLevelLayer, _composed
    assert SpyNetLevelLayer.native_backward is False and SpyNetLevelLayer.fused is True      # the route ships off
    from networks._spynet import SPyNet
    assert SPyNet().fused_level_backward is False
    g = torch.Generator().manual_seed(1)
    first, second = torch.rand(1, 3, 7, 9, generator=g), torch.rand(1, 3, 7, 9, generator=g)
    coarse = torch.randn(1, 2, 3, 4, generator=g)
    for flags in ((False, False), (True, True), (False, True)):
        grads = []
        for native in (False, True):
            layer = SpyNetLevelLayer(*flags)
            layer.native_backward = native
            c = coarse.clone().requires_grad_(True)
            out = layer(first, second, c)
            assert out.grad_fn is not None and "SpyNetLevel" not in type(out.grad_fn).__name__      # torch's own graph
            assert torch.equal(out, _composed(first, second, coarse, *flags))
            out.square().sum().backward()
            grads.append(c.grad)
        assert torch.equal(*grads) and float(grads[0].abs().max()) > 0
    assert SpyNetLevelLayer.native_backward is False       # the instances' flags left the class alone


def test_binding_imports_without_loading_the_library():
    """in a fresh interpreter: after the import of the binding, the layer and the network no libmemc_hip_spynet_grad.so is
    mapped"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import my_package._ext.my_lib_spynet_grad as L\n"
            "import my_package.functions.SpyNetLevelLayer, my_package.modules.SpyNetLevelModule, networks\n"
            "assert 'libmemc_hip_spynet' not in open('/proc/self/maps').read()\n"
            "assert L.version() == 'memc_hip_spynet_grad 0.1 gfx950'\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libmemc_hip_spynet_grad' in maps and 'libmemc_hip_spynet.so' not in maps\n"
            % os.path.join(ROOT, "memc-net_amd"))
    subprocess.run([sys.executable, "-c", code], check=True)


def test_kernel_uses_no_scratch():
    """The compiler's own resource remarks: one kernel, no private scratch, no dynamic stack, the LDS of two planes of the
    staged box and nothing else; at least four waves per SIMD."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from tools import kernel_resources as KR
    import _spynet_grad_spec as SG
    kernels = KR.resources_of("spynet_level_bwd.hip")
    assert [k["name"].split("::")[-1] for k in kernels] == ["spynet_level_bwd_tiled"], [k["name"] for k in kernels]
    for k in kernels:
        assert int(k.get("scratch", "0")) == 0 and k.get("dynstack", "False") == "False", k
        assert int(k.get("lds", "0")) == 2 * SG.BOX * SG.BOX * 4 and int(k["occupancy"]) >= 4, k
    assert "spynet_level_bwd.hip" in KR.SOURCES            # and the project-wide scratch test sees it
