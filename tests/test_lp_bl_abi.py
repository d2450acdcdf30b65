"""The fp16 / bf16 bilinear warp library libmemc_hip_lp_bl.so (include/memc_warp_lp_bl.h: a half image and output beside a flow
of that dtype or float32, forward and RGB backward): loads without a GPU, exports exactly its header, its own kernels only
and none of the other libraries' entry points, answers malformed descriptors with -1 and backward calls outside its coverage
with 1 before the device is touched, none of its kernels uses private scratch, and the Python binding takes the half
patterns only.  CPU only -- no kernel is launched here (every call below is rejected, declined or empty)."""
import contextlib
import ctypes
import glob
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEADER = os.path.join(ROOT, "include", "memc_warp_lp_bl.h")
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
LIB = os.path.join(LIBDIR, "libmemc_hip_lp_bl.so")
UNIT = "lp_interpolation.hip"
VERSION = "memc_hip_lp_bl 0.1 gfx950"
F32, F16, BF16 = 0, 1, 2
HALVES = (F16, BF16)
FWD = ["InterpolationLayer_gpu_forward_lp", "InterpolationChLayer_gpu_forward_lp"]
BWD = ["InterpolationLayer_gpu_backward_lp", "InterpolationChLayer_gpu_backward_lp"]
SYMBOLS = ["memc_lp_bl_version", "memc_lp_bl_last_kernel_path"] + FWD + BWD
FWD_ORDER = ("x", "flow", "out")
BWD_ORDER = ("x", "flow", "gout", "gin1", "gin2")
IMAGE_LIKE = ("x", "out", "gout", "gin1")


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


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(names) == sorted(SYMBOLS), names
    return names


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {p[2]: p[1] for p in (line.split() for line in out.splitlines()) if len(p) == 3}


def is_hip_plumbing(name):
    return name.startswith("_ZN4memc") or name.startswith("__hip_")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(LIB)
    L.memc_lp_bl_version.restype = ctypes.c_char_p
    L.memc_lp_bl_last_kernel_path.restype = ctypes.c_char_p
    for names, n in ((FWD, 3), (BWD, 5)):
        for name in names:
            f = getattr(L, name)
            f.restype = ctypes.c_int
            f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] + [ctypes.POINTER(Tensor4)] * n
    return L


class Call:
    """One call: the tensors of a well-formed, covered B x C x H x W call, any of them replaceable"""

    def __init__(self, lib, name, B=2, C=3, H=8, W=16):
        self.f = getattr(lib, name)
        self.order = FWD_ORDER if name in FWD else BWD_ORDER
        self.shape = (B, C, H, W)
        self.t = {k: desc((B, 2, H, W) if k in ("flow", "gin2") else (B, C, H, W)) for k in self.order}

    def __call__(self, td=F16, ft=None, **repl):
        """td: the payload dtype; ft: the flow dtype (default: the payload's); keywords replace a tensor (None: NULL)"""
        t = dict(self.t, **repl)
        return self.f(None, td, td if ft is None else ft, *[None if t[k] is None else ctypes.byref(t[k]) for k in self.order])


def mutations(call):
    B, C, H, W = call.shape
    img = [k for k in call.order if k in IMAGE_LIKE]
    flo = [k for k in call.order if k not in IMAGE_LIKE]
    m = []
    for k in call.order:                                      # each tensor null, or with null data
        m += [{k: None}, {k: desc(tuple(call.t[k].size), data=0)}]
    # a w-stride of 2
    m.append({k: desc((B, C, H, W), strides=(2 * C * H * W, 2 * H * W, 2 * W, 2)) for k in img})
    m.append({k: desc((B, 2, H, W), strides=(4 * H * W, 2 * H * W, 2 * W, 2)) for k in flo})
    # a flow that is not [B, 2, H, W]
    for s in ((B, 3, H, W), (B, 1, H, W), (B - 1, 2, H, W), (B, 2, H - 1, W), (B, 2, H, W - 4)):
        m.append({k: desc(s) for k in flo})
    # output / gradoutput / gradinput1 (/ gradinput2) of another shape, or of another layout
    for k in call.order[2:]:
        base = (B, 2, H, W) if k == "gin2" else (B, C, H, W)
        for i in range(4):
            s = list(base)
            s[i] -= 1 if i < 3 else 4
            m.append({k: desc(tuple(s))})
        m.append({k: desc(base, strides=(base[1] * H * (W + 4), H * (W + 4), W + 4, 1))})
    # strides and sizes beyond int32, negative ones
    m += [dict(x=desc((B, C, H, W), strides=(1 << 33, H * W, W, 1))), dict(flow=desc((B, 2, H, W), strides=(2 * H * W, 1 << 32, W, 1))),
          {call.order[2]: desc((B, C, H, W), strides=(C * H * W, H * W, -W, 1))}, dict(x=desc((B, C, H, 1 << 32)))]
    return m


def test_loads_without_a_gpu_and_identifies_itself(lib):
    assert lib.memc_lp_bl_version() == VERSION.encode()
    assert lib.memc_lp_bl_last_kernel_path() == b""           # no call enqueued by this thread yet


def test_exports_exactly_the_header(lib):
    syms = exported(LIB)
    c_surface = sorted(n for n in syms if not is_hip_plumbing(n))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    assert len(c_surface) == 6
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    own = ("bl_fwd_lp_tiled", "bl_fwd_lpI", "bl_bwd_lp_c3_pk")
    assert kernels and all(any(o in k for o in own) for k in kernels), kernels          # its own kernels only
    # a library of its own: none of its C symbols in any other library, none of the fp32 library's here
    other_libs = [p for p in glob.glob(os.path.join(LIBDIR, "libmemc_hip*.so")) if p != LIB]
    assert len(other_libs) >= 13, other_libs               # fp32, measure, twelve satellites
    others = {n for p in other_libs for n in exported(p) if not is_hip_plumbing(n)}
    for name in ("InterpolationLayer_gpu_forward", "InterpolationChLayer_gpu_backward", "InterpolationLayer_gpu_forward_kernel",
                 "FilterInterpolationLayer_gpu_backward_lp", "FlowProjectionLayer_gpu_backward_lp"):
        assert name in others and name not in syms, name
    assert not others & set(syms), others & set(syms)


def test_the_header_compiles_as_c(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler (the oracle is built with one)"
    src = tmp_path / "use.c"
    src.write_text('#include "memc_warp_lp_bl.h"\n'
                   "int use(const memc_tensor4 *t) { return InterpolationLayer_gpu_forward_lp(0, MEMC_F16, MEMC_F32, t, t, t)\n"
                   "    + InterpolationChLayer_gpu_backward_lp(0, MEMC_BF16, MEMC_BF16, t, t, t, t, t); }\n")
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c",
                        str(src), "-o", str(tmp_path / "use.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


@pytest.mark.parametrize("name", FWD + BWD)
def test_rejects_other_dtypes(lib, name):
    call = Call(lib, name)
    for td in (F32, 3, -1, 7):                              # a payload that is not F16 / BF16
        assert call(td) == -1 and call(td, F32) == -1, td
    for td, ft in ((F16, BF16), (BF16, F16), (F16, 3), (BF16, -1)):      # a flow neither float32 nor the payload
        assert call(td, ft) == -1, (td, ft)
    assert lib.memc_lp_bl_last_kernel_path() == b""


@pytest.mark.parametrize("name", FWD + BWD)
def test_rejects_bad_descriptors_before_the_device(lib, name):
    call = Call(lib, name)
    muts = mutations(call)
    assert len(muts) >= (20 if name in FWD else 30)
    for td in HALVES:                                      # (the unmutated call is covered: never sent)
        for ft in (td, F32):
            for m in muts:
                assert call(td, ft, **m) == -1, (td, ft, sorted(m))
    assert lib.memc_lp_bl_last_kernel_path() == b""         # nothing was enqueued


def test_interpolation_insists_on_three_channels(lib):
    for name in (FWD[0], BWD[0]):
        for ch in (1, 2, 4, 8):
            for td in HALVES:
                assert Call(lib, name, C=ch)(td) == -1, (name, ch)
    # InterpolationCh does not: its backward declines what it does not cover instead
    for ch in (1, 2, 4, 8):
        for td in HALVES:
            assert Call(lib, BWD[1], C=ch)(td) == 1 and Call(lib, BWD[1], C=ch)(td, F32) == 1, ch
    assert lib.memc_lp_bl_last_kernel_path() == b""


def _rows(B, C, H, W, row, data=0x10000):
    return desc((B, C, H, W), data=data, strides=(C * H * row, H * row, row, 1))


UNCOVERED = [
    ("W=10", dict(W=10), lambda c, ft: {}),
    ("W=4", dict(W=4), lambda c, ft: {}),
    ("W=6", dict(W=6), lambda c, ft: {}),
    ("T row stride 18", {}, lambda c, ft: {k: _rows(2, 3, 8, 16, 18) for k in ("x", "gout", "gin1")}),
    ("image base 2 bytes off", {}, lambda c, ft: dict(x=desc((2, 3, 8, 16), data=0x10002))),
    ("gradoutput base 4 bytes off", {}, lambda c, ft: dict(gout=desc((2, 3, 8, 16), data=0x10004))),
    ("gradinput1 base 2 bytes off", {}, lambda c, ft: dict(gin1=desc((2, 3, 8, 16), data=0x10002))),
    ("flow base 2 bytes off", {}, lambda c, ft: dict(flow=desc((2, 2, 8, 16), data=0x10002))),
    ("gradinput2 base 2 bytes off", {}, lambda c, ft: dict(gin2=desc((2, 2, 8, 16), data=0x10002))),
    ("T channel stride H * W + 2", {}, lambda c, ft: {k: desc((2, 3, 8, 16), strides=(390, 130, 16, 1)) for k in ("x", "gout", "gin1")}),
]


@pytest.mark.parametrize("name", BWD)
@pytest.mark.parametrize("case", UNCOVERED, ids=[c[0] for c in UNCOVERED])
def test_backward_calls_outside_the_coverage_are_declined(lib, case, name):
    """well-formed calls that the tiled kernel does not take: return code 1, nothing touched"""
    _label, shape, repl = case
    c = Call(lib, name, **shape)
    for td in HALVES:
        for ft in (td, F32):
            assert c(td, ft, **repl(c, ft)) == 1, (td, ft)
    assert lib.memc_lp_bl_last_kernel_path() == b""         # nothing was enqueued


def test_a_half_flow_four_bytes_off_is_declined_a_float32_one_is_not_judged_by_quads(lib):
    """a base 4 bytes off its quads: a half flow is declined; the float32 flow's rule is dword alignment, so only the empty
    batch can show it here without a launch -- the half one must return 1"""
    c = Call(lib, BWD[0])
    for td in HALVES:
        assert c(td, td, flow=desc((2, 2, 8, 16), data=0x10004)) == 1
        assert c(td, td, gin2=desc((2, 2, 8, 16), data=0x10004)) == 1


def test_a_plane_beyond_32_bit_offsets_is_declined(lib):
    """rows 2^21 elements apart, 600 of them: the image's planes"""
    S, H = 1 << 21, 600
    huge = lambda ch: desc((1, ch, H, 16), strides=(0, H * S, S, 1))      # noqa: E731
    big = Call(lib, BWD[0], B=1, H=H)
    for td in HALVES:
        assert big(td, x=huge(3), gout=huge(3), gin1=huge(3)) == 1
    assert lib.memc_lp_bl_last_kernel_path() == b""


@pytest.mark.parametrize("name", FWD + BWD)
def test_empty_batch_is_a_no_op(lib, name):
    c = Call(lib, name)
    e = {k: desc((0, 2 if k in ("flow", "gin2") else 3, 8, 16), data=0) for k in c.order}
    for td in HALVES:
        assert c(td, **e) == 0 and c(td, F32, **e) == 0
    assert lib.memc_lp_bl_last_kernel_path() == b""         # nothing was launched


def test_no_kernel_uses_private_scratch_and_all_are_there():
    """The compiler's own resource remarks: every instantiation by name, no private scratch, no dynamic stack; the tiled
    forward within the 256 VGPRs of its two waves per SIMD, the backward within the 128 of its four"""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    from tools import kernel_resources as KR
    kernels = KR.resources_of(UNIT)
    pairs = [("F16", "F32"), ("F16", "F16"), ("BF16", "F32"), ("BF16", "BF16")]
    want = []
    for t, ft in pairs:
        want += ["memc::bl_fwd_lp_tiled<memc::%s, memc::%s, 3, 2496>" % (t, ft), "memc::bl_fwd_lp_tiled<memc::%s, memc::%s, 0, 3072>" % (t, ft),
                 "memc::bl_fwd_lp<memc::%s, memc::%s, 3>" % (t, ft), "memc::bl_fwd_lp<memc::%s, memc::%s, 0>" % (t, ft),
                 "memc::bl_bwd_lp_c3_pk<memc::%s, memc::%s>" % (t, ft)]
    assert sorted(k["name"] for k in kernels) == sorted(want)
    bad = [(k["name"], k.get("scratch"), k.get("dynstack"), k.get("vgprs")) for k in kernels
           if int(k.get("scratch", "0")) > 0 or k.get("dynstack", "False") != "False"
           or int(k.get("vgprs", "999")) > (128 if "bl_bwd" in k["name"] else 256)]
    assert not bad, bad
    assert UNIT in KR.SOURCES


# --------------------------------------------------------------------------------------------------------------
# the Python side
# --------------------------------------------------------------------------------------------------------------
def _binding():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_lp_bl as L
    return L


def _tensors(order, t, ft=None, **other):
    """the tensors on the CPU (no kernel is reached): dtypes by position, `other` replaces some"""
    import torch
    ft = t if ft is None else ft
    dt = dict(x=t, flow=ft, out=t, gout=t, gin1=torch.float32, gin2=ft)
    dt.update(other)
    return tuple(torch.zeros((1, 2 if k in ("flow", "gin2") else 3, 8, 16), dtype=dt[k]) for k in order)


def _no_device(monkeypatch, L, seen):
    """keep a CPU tensor from ending the call before the dtype check, and the C functions out of reach: they record the
    two leading dtype codes instead"""
    import types
    import my_package._ext._satellite as S
    monkeypatch.setattr(S, "describe", lambda t, symbol, position: Tensor4())
    monkeypatch.setattr(S.torch.cuda, "current_stream", lambda dev: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(S.torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(L._SAT, "_lib", types.SimpleNamespace(
        **{name: (lambda stream, *a: seen.append(a[:2]) or 0) for name in FWD + BWD}))


def test_importing_the_binding_and_the_layers_loads_no_library():
    """in a fresh interpreter: after the import of the binding and of the layers no libmemc_hip_lp_bl.so is mapped"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import my_package._ext.my_lib_lp_bl as L\n"
            "import my_package.functions.InterpolationLayer, my_package.functions.InterpolationChLayer\n"
            "import my_package.modules.InterpolationModule, my_package.modules.InterpolationChModule\n"
            "assert L._SAT._lib is None\n"
            "assert 'libmemc_hip_lp_bl' not in open('/proc/self/maps').read()\n" % os.path.join(ROOT, "memc-net_amd"))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_python_loader_binds_the_library(lib):
    L = _binding()
    assert L.LIB_PATH == LIB
    assert L.version() == VERSION
    assert L.last_kernel_path() == ""
    assert all(callable(getattr(L, n)) for n in FWD + BWD)


def test_the_binding_takes_the_four_half_patterns(monkeypatch):
    import torch
    L = _binding()
    seen = []
    _no_device(monkeypatch, L, seen)
    for t, code in ((torch.float16, F16), (torch.bfloat16, BF16)):
        for ft, fcode in ((t, code), (torch.float32, F32)):
            del seen[:]
            for name in FWD:
                assert getattr(L, name)(*_tensors(FWD_ORDER, t, ft)) == 0
            for name in BWD:
                assert getattr(L, name)(*_tensors(BWD_ORDER, t, ft)) == 0
            assert seen == [(code, fcode)] * 4, seen


def test_the_binding_rejects_every_other_dtype_pattern(monkeypatch):
    import torch
    L = _binding()
    seen = []
    _no_device(monkeypatch, L, seen)
    h, b, f32 = torch.float16, torch.bfloat16, torch.float32
    for name in FWD:
        for args in (_tensors(FWD_ORDER, f32), _tensors(FWD_ORDER, f32, h), _tensors(FWD_ORDER, torch.float64),    # a float32 image
                     _tensors(FWD_ORDER, h, b), _tensors(FWD_ORDER, b, h), _tensors(FWD_ORDER, h, torch.float64),  # mixed halves
                     _tensors(FWD_ORDER, h, out=f32), _tensors(FWD_ORDER, b, out=h)):
            with pytest.raises(TypeError):
                getattr(L, name)(*args)
    for name in BWD:
        for args in (_tensors(BWD_ORDER, f32), _tensors(BWD_ORDER, f32, h), _tensors(BWD_ORDER, h, b), _tensors(BWD_ORDER, b, h),
                     _tensors(BWD_ORDER, h, gout=f32), _tensors(BWD_ORDER, h, gout=b),
                     _tensors(BWD_ORDER, h, gin1=h), _tensors(BWD_ORDER, b, gin1=b),                  # gradinput1 is float32
                     _tensors(BWD_ORDER, h, gin2=f32), _tensors(BWD_ORDER, h, f32, gin2=h), _tensors(BWD_ORDER, b, gin2=h)):
            with pytest.raises(TypeError):
                getattr(L, name)(*args)
        with pytest.raises(TypeError):
            getattr(L, name)(None, *_tensors(BWD_ORDER, h)[1:])
    assert not seen


def test_the_binding_refuses_cpu_tensors(monkeypatch):
    import types
    import torch
    L = _binding()
    monkeypatch.setattr(L._SAT, "_lib", types.SimpleNamespace(
        **{name: (lambda *a: pytest.fail("the library was called")) for name in FWD + BWD}))
    with pytest.raises(TypeError, match="expected a CUDA"):
        L.InterpolationLayer_gpu_forward_lp(*_tensors(FWD_ORDER, torch.float16))
    with pytest.raises(TypeError, match="expected a CUDA"):
        L.InterpolationChLayer_gpu_backward_lp(*_tensors(BWD_ORDER, torch.bfloat16))
