"""The fp16 / bf16 depth projection backward library libmemc_hip_lp_dproj_grad.so (include/memc_warp_lp_dproj_grad.h: a half
flow, depth, gradoutput and gradients beside the float32 count and forward output): loads without a GPU, exports exactly
its header, its own kernels only and none of the other libraries' entry points, answers malformed descriptors with -1 and
calls outside its coverage with 1 before the device is touched, neither of its two kernels spills or loses the fp32 depth
kernel's workgroups per CU, and the Python binding takes the two half patterns only.  CPU only -- no kernel is launched
here (every call below is rejected, declined or empty)."""
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

HEADER = os.path.join(ROOT, "include", "memc_warp_lp_dproj_grad.h")
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
LIB = os.path.join(LIBDIR, "libmemc_hip_lp_dproj_grad.so")
UNIT = "lp_depth_flow_projection_bwd.hip"
VERSION = "memc_hip_lp_dproj_grad 0.1 gfx950"
ENTRY = "DepthFlowProjectionLayer_gpu_backward_lp"
F32, F16, BF16 = 0, 1, 2
HALVES = (F16, BF16)
SYMBOLS = ["memc_lp_dproj_grad_version", "memc_lp_dproj_grad_last_kernel_path", ENTRY]
ORDER = ("flow", "depth", "count", "out", "gout", "gin1", "gin2")
CHANNELS = dict(zip(ORDER, (2, 1, 1, 2, 2, 2, 1)))
T_TENSORS = ("flow", "depth", "gout", "gin1", "gin2")
FLOW_LIKE = ("flow", "out", "gout", "gin1")          # of the flow's shape and layout
DEPTH_LIKE = ("depth", "gin2")


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
    L.memc_lp_dproj_grad_version.restype = ctypes.c_char_p
    L.memc_lp_dproj_grad_last_kernel_path.restype = ctypes.c_char_p
    f = getattr(L, ENTRY)
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.POINTER(Tensor4)] * 7
    return L


class Call:
    """One call: the tensors of a well-formed, covered B x 2 x H x W call, any of them replaceable"""

    def __init__(self, lib, B=2, H=8, W=16):
        self.f = getattr(lib, ENTRY)
        self.t = {k: desc((B, CHANNELS[k], H, W)) for k in ORDER}

    def __call__(self, td=F16, **repl):
        """td: the payload dtype; keywords flow, depth, count, out, gout, gin1, gin2 replace a tensor (None: NULL)"""
        t = dict(self.t, **repl)
        return self.f(None, td, *[None if t[k] is None else ctypes.byref(t[k]) for k in ORDER])


def _each(keys, make):
    return {k: make(CHANNELS[k]) for k in keys}


def mutations(call):
    m = []
    for k in ORDER:                                           # each of the seven tensors null, or with null data
        m += [{k: None}, {k: desc(tuple(call.t[k].size), data=0)}]
    # wrong channel counts: a flow of three channels or of one (and everything of its shape), a depth or a count of two
    m.append(_each(FLOW_LIKE, lambda c: desc((2, 3, 8, 16))))
    m.append(_each(FLOW_LIKE, lambda c: desc((2, 1, 8, 16))))
    m.append(_each(DEPTH_LIKE, lambda c: desc((2, 2, 8, 16))))
    m += [dict(count=desc(s)) for s in ((2, 2, 8, 16), (1, 1, 8, 16), (2, 1, 7, 16), (2, 1, 8, 12))]
    # a depth of another shape (with its gradient)
    m += [_each(DEPTH_LIKE, lambda c, s=s: desc(s)) for s in ((1, 1, 8, 16), (2, 1, 7, 16), (2, 1, 8, 12))]
    # a gradient, gradoutput or forward output not of its input's shape, or not of its layout
    m += [dict(gin1=desc(s)) for s in ((2, 2, 8, 12), (2, 2, 7, 16), (1, 2, 8, 16), (2, 3, 8, 16))]
    m += [dict(gout=desc(s)) for s in ((2, 2, 8, 12), (2, 2, 7, 16), (1, 2, 8, 16), (2, 1, 8, 16))]
    m += [dict(out=desc(s)) for s in ((2, 2, 8, 12), (2, 2, 7, 16), (1, 2, 8, 16), (2, 1, 8, 16))]
    m += [dict(gin2=desc(s)) for s in ((2, 1, 8, 12), (2, 1, 7, 16), (1, 1, 8, 16), (2, 2, 8, 16))]
    m += [dict(gin1=desc((2, 2, 8, 16), strides=(512, 256, 32, 1))), dict(gout=desc((2, 2, 8, 16), strides=(320, 160, 20, 1))),
          dict(out=desc((2, 2, 8, 16), strides=(512, 256, 32, 1))), dict(out=desc((2, 2, 8, 16), strides=(260, 130, 16, 1))),
          dict(gin2=desc((2, 1, 8, 16), strides=(256, 256, 32, 1))), dict(gin2=desc((2, 1, 8, 16), strides=(160, 160, 20, 1)))]
    # a w-stride of 2
    m.append(_each(FLOW_LIKE, lambda c: desc((2, 2, 8, 16), strides=(512, 256, 32, 2))))
    m.append(_each(DEPTH_LIKE, lambda c: desc((2, 1, 8, 16), strides=(256, 256, 32, 2))))
    m.append(dict(count=desc((2, 1, 8, 16), strides=(256, 256, 32, 2))))
    # strides and sizes beyond int32, negative ones
    m += [dict(flow=desc((2, 2, 8, 16), strides=(1 << 33, 128, 16, 1))), dict(gin1=desc((2, 2, 8, 16), strides=(256, 1 << 32, 16, 1))),
          dict(count=desc((2, 1, 8, 16), strides=(1 << 31, 128, 16, 1))), dict(gout=desc((2, 2, 8, 16), strides=(256, 128, -16, 1))),
          dict(depth=desc((2, 1, 8, 16), strides=(1 << 31, 128, 16, 1))), dict(out=desc((2, 2, 8, 16), strides=(256, 128, -16, 1))),
          dict(gin2=desc((2, 1, 8, 16), strides=(128, 1 << 32, 16, 1))), dict(flow=desc((2, 2, 8, 1 << 32)))]
    return m


def test_loads_without_a_gpu_and_identifies_itself(lib):
    assert lib.memc_lp_dproj_grad_version() == VERSION.encode()
    assert lib.memc_lp_dproj_grad_last_kernel_path() == b""     # no call enqueued by this thread yet


def test_exports_exactly_the_header(lib):
    syms = exported(LIB)
    c_surface = sorted(n for n in syms if not is_hip_plumbing(n))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    assert len(kernels) == 2 and all("dproj_bwd_lp_tiled" in k for k in kernels), kernels     # its own kernels only
    assert sorted(re.search(r"INS_\d(\w+?)E", k).group(1) for k in kernels) == ["BF16", "F16"], kernels
    assert not [n for n in syms if "proj_bwd_tiledI" in n or "17proj_bwd_lp_tiled" in n or "proj_scatter" in n
                or "proj_owner" in n or "fi_" in n]
    # a library of its own: none of its C symbols in any other library
    other_libs = [p for p in glob.glob(os.path.join(LIBDIR, "libmemc_hip*.so")) if p != LIB]
    assert len(other_libs) >= 15, other_libs              # fp32, measure, thirteen satellites
    others = {n for p in other_libs for n in exported(p) if not is_hip_plumbing(n)}
    for name in ("DepthFlowProjectionLayer_gpu_backward", "DepthFlowProjectionLayer_gpu_forward",
                 "FlowProjectionLayer_gpu_backward_lp", "InterpolationLayer_gpu_backward_lp"):
        assert name in others, name
    assert not others & set(syms), others & set(syms)


def test_rejects_other_payload_dtypes(lib):
    call = Call(lib)
    for td in (F32, 3, -1, 7):
        assert call(td) == -1, td
    assert lib.memc_lp_dproj_grad_last_kernel_path() == b""


def test_rejects_bad_descriptors_before_the_device(lib):
    call = Call(lib)
    muts = mutations(call)
    assert len(muts) >= 30
    for td in HALVES:                                      # (the unmutated call is covered: never sent)
        for m in muts:
            assert call(td, **m) == -1, (td, sorted(m), [tuple(v.size) + tuple(v.stride) for v in m.values() if v is not None])
    assert lib.memc_lp_dproj_grad_last_kernel_path() == b""    # nothing was enqueued


def _rows(B, C, H, W, row, data=0x10000):
    return desc((B, C, H, W), data=data, strides=(C * H * row, H * row, row, 1))


def _off(k, by):
    return lambda: {k: desc((2, CHANNELS[k], 8, 16), data=0x10000 + by)}


UNCOVERED = [
    ("W=10", dict(W=10), lambda: {}),
    ("W=4", dict(W=4), lambda: {}),
    ("W=6", dict(W=6), lambda: {}),
    # (the forward output has the flow's element strides by the layout rule, whatever its storage)
    ("row stride 18", {}, lambda: dict(_each(FLOW_LIKE, lambda c: _rows(2, 2, 8, 16, 18)), **_each(DEPTH_LIKE, lambda c: _rows(2, 1, 8, 16, 18)))),
    ("flow base 2 bytes off", {}, _off("flow", 2)),
    ("flow base 4 bytes off", {}, _off("flow", 4)),
    ("depth base 2 bytes off", {}, _off("depth", 2)),
    ("depth base 4 bytes off", {}, _off("depth", 4)),
    ("gradoutput base 2 bytes off", {}, _off("gout", 2)),
    ("gradoutput base 4 bytes off", {}, _off("gout", 4)),
    ("gradinput1 base 2 bytes off", {}, _off("gin1", 2)),
    ("gradinput1 base 4 bytes off", {}, _off("gin1", 4)),
    ("gradinput2 base 2 bytes off", {}, _off("gin2", 2)),
    ("gradinput2 base 4 bytes off", {}, _off("gin2", 4)),
    ("flow channel stride H * W + 2", {}, lambda: _each(FLOW_LIKE, lambda c: desc((2, 2, 8, 16), strides=(260, 130, 16, 1)))),
    ("depth batch stride H * W + 2", {}, lambda: _each(DEPTH_LIKE, lambda c: desc((2, 1, 8, 16), strides=(130, 130, 16, 1)))),
    ("count base 2 bytes off", {}, _off("count", 2)),
    ("output base 2 bytes off", {}, _off("out", 2)),
]


@pytest.mark.parametrize("case", UNCOVERED, ids=[c[0] for c in UNCOVERED])
def test_calls_outside_the_coverage_are_declined(lib, case):
    """well-formed calls that the tiled kernel does not take: return code 1 for both dtypes, nothing touched"""
    _label, shape, repl = case
    c = Call(lib, **shape)
    for td in HALVES:
        assert c(td, **repl()) == 1, td
    assert lib.memc_lp_dproj_grad_last_kernel_path() == b""    # nothing was enqueued


def test_a_plane_beyond_32_bit_offsets_is_declined(lib):
    """rows 2^21 elements apart, 600 of them: the flow's planes, the depth's, or the count's"""
    S, H = 1 << 21, 600
    huge = lambda ch: desc((1, ch, H, 16), strides=(0, H * S, S, 1))      # noqa: E731
    big = Call(lib, B=1, H=H)
    for td in HALVES:
        assert big(td, **_each(FLOW_LIKE, lambda c: huge(2))) == 1
        assert big(td, **_each(DEPTH_LIKE, lambda c: huge(1))) == 1
        assert big(td, count=huge(1)) == 1
    assert lib.memc_lp_dproj_grad_last_kernel_path() == b""


def test_empty_batch_is_a_no_op(lib):
    for td in HALVES:
        assert Call(lib)(td, **_each(ORDER, lambda c: desc((0, c, 8, 16), data=0))) == 0
        assert Call(lib)(td, **_each(ORDER, lambda c: desc((2, c, 0, 16), data=0))) == 0
    assert lib.memc_lp_dproj_grad_last_kernel_path() == b""    # nothing was launched


def test_neither_kernel_spills_or_loses_the_fp32_kernel_s_occupancy():
    """The compiler's own resource remarks: the two instantiations by name, no private scratch, no dynamic stack, and
    registers for at least the workgroups of 256 lanes per CU (waves per SIMD) that the fp32 depth kernel
    proj_bwd_tiled<true, 2496, false> has -- four, what its 40000 bytes of LDS admit."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    from tools import kernel_resources as KR
    kernels = KR.resources_of(UNIT)
    assert sorted(k["name"] for k in kernels) == sorted("memc::dproj_bwd_lp_tiled<memc::%s>" % t for t in ("F16", "BF16"))
    bad = [(k["name"], k.get("scratch"), k.get("dynstack"), k.get("occupancy"), k.get("vgprs")) for k in kernels
           if int(k.get("scratch", "0")) > 0 or k.get("dynstack", "False") != "False" or int(k.get("occupancy", "0")) < 4
           or int(k.get("vgprs", "999")) > 128]
    assert not bad, bad
    assert UNIT in KR.SOURCES
    fp32 = [k for k in KR.resources_of("flow_projection.hip") if k["name"] == "memc::proj_bwd_tiled<true, 2496, false>"]
    assert len(fp32) == 1 and int(fp32[0]["occupancy"]) == 4, fp32
    assert all(int(k["occupancy"]) >= int(fp32[0]["occupancy"]) for k in kernels), (fp32, kernels)


# --------------------------------------------------------------------------------------------------------------
# the Python side
# --------------------------------------------------------------------------------------------------------------
def _binding():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_lp_dproj_grad as L
    return L


def _dtypes(t):
    import torch
    return dict(zip(ORDER, (t, t, torch.float32, torch.float32, t, t, t)))


def _tensors(t, **other):
    """the seven tensors on the CPU (no kernel is reached): dtypes by position, `other` replaces some"""
    import torch
    dt = dict(_dtypes(t), **other)
    return tuple(torch.zeros((1, CHANNELS[k], 8, 16), dtype=dt[k]) for k in ORDER)


def _no_device(monkeypatch, L, seen):
    """keep a CPU tensor from ending the call before the dtype check, and the C function out of reach: it records the
    leading dtype code instead"""
    import types
    import my_package._ext._satellite as S
    monkeypatch.setattr(S, "describe", lambda t, symbol, position: Tensor4())
    monkeypatch.setattr(S.torch.cuda, "current_stream", lambda dev: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(S.torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(L._SAT, "_lib", types.SimpleNamespace(**{ENTRY: lambda stream, *a: seen.append(a[0]) or 0}))


def test_importing_the_binding_loads_no_library():
    """in a fresh interpreter: after the import of the binding and of the layer no libmemc_hip_lp_dproj_grad.so is mapped"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import my_package._ext.my_lib_lp_dproj_grad as L\n"
            "import my_package.functions.DepthFlowProjectionLayer\n"
            "assert L._SAT._lib is None\n"
            "assert 'libmemc_hip_lp_dproj_grad' not in open('/proc/self/maps').read()\n" % os.path.join(ROOT, "memc-net_amd"))
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_python_loader_binds_the_library(lib):
    L = _binding()
    assert L.LIB_PATH == LIB
    assert L.version() == VERSION
    assert L.last_kernel_path() == ""
    assert callable(L.DepthFlowProjectionLayer_gpu_backward_lp)


def test_the_binding_takes_the_two_half_patterns(monkeypatch):
    import torch
    L = _binding()
    seen = []
    _no_device(monkeypatch, L, seen)
    for t, code in ((torch.float16, F16), (torch.bfloat16, BF16)):
        del seen[:]
        assert L.DepthFlowProjectionLayer_gpu_backward_lp(*_tensors(t)) == 0
        assert seen == [code], seen                       # the payload dtype, derived from the flow


def test_the_binding_rejects_every_other_dtype_pattern(monkeypatch):
    import torch
    L = _binding()
    seen = []
    _no_device(monkeypatch, L, seen)
    h, b, f32 = torch.float16, torch.bfloat16, torch.float32
    patterns = [_tensors(f32), _tensors(torch.float64)]                    # input1 neither float16 nor bfloat16
    for t, other in ((h, b), (b, h)):
        for k in T_TENSORS[1:]:                                            # one T tensor float32, or of the other half dtype
            patterns += [_tensors(t, **{k: f32}), _tensors(t, **{k: other})]
        for k in ("count", "out"):                                         # a half or float64 count / forward output
            patterns += [_tensors(t, **{k: t}), _tensors(t, **{k: torch.float64})]
    assert len(patterns) == 2 + 2 * (8 + 4)
    for args in patterns:
        with pytest.raises(TypeError):
            L.DepthFlowProjectionLayer_gpu_backward_lp(*args)
    with pytest.raises(TypeError):
        L.DepthFlowProjectionLayer_gpu_backward_lp(None, *_tensors(h)[1:])
    assert not seen


def test_the_binding_refuses_cpu_tensors_and_other_ranks(monkeypatch):
    """the sibling bindings' refusals, before the library is reached: a CPU tensor; with the device check out of the way, a
    tensor that is not 4-D"""
    import types
    import torch
    L = _binding()
    monkeypatch.setattr(L._SAT, "_lib", types.SimpleNamespace(**{ENTRY: lambda *a: pytest.fail("the library was called")}))
    with pytest.raises(TypeError, match="expected a CUDA"):
        L.DepthFlowProjectionLayer_gpu_backward_lp(*_tensors(torch.float16))
    import my_package._ext._satellite as S

    class OnDevice(torch.Tensor):                          # a CPU tensor that says it is on the device
        is_cuda = True
    flat = torch.zeros((2, 8, 16), dtype=torch.float16).as_subclass(OnDevice)
    with pytest.raises(TypeError, match="4-D"):
        S.describe(flat, ENTRY, 0)
    with pytest.raises(TypeError, match="4-D"):
        L.DepthFlowProjectionLayer_gpu_backward_lp(flat, *_tensors(torch.float16)[1:])
