"""The pure fp16 / bf16 blend backward library libmemc_hip_lp_blend_grad.so (include/memc_warp_lp_blend_grad.h: a half
image, taps and occlusion, the flow and gradoutput in fp32 or that type): loads without a GPU, exports exactly its header
and none of the other libraries' entry points, answers malformed descriptors as its mixed sibling
libmemc_hip_mx_blend_grad.so answers them live (-1), declines calls outside its coverage with 1 before touching the
device, none of its eight kernels spills, and the Python binding takes the eight half patterns only -- a binding of its
own, which my_lib_blend_grad's door never reaches.  CPU only -- no kernel is launched here (every call below is rejected,
declined or empty)."""
import contextlib
import ctypes
import glob
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_blend_grad_abi as BG      # noqa: E402  (Tensor4, desc, the export helpers)

HEADER = os.path.join(ROOT, "include", "memc_warp_lp_blend_grad.h")
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
LIB = os.path.join(LIBDIR, "libmemc_hip_lp_blend_grad.so")
MX_LIB = os.path.join(LIBDIR, "libmemc_hip_mx_blend_grad.so")
UNIT = "lp_fi_blend_bwd_c3.hip"
VERSION = "memc_hip_lp_blend_grad 0.1 gfx950"
F32, F16, BF16 = 0, 1, 2
TRIPLES = tuple((t, f, g) for t in (F16, BF16) for f in (F32, t) for g in (F32, t))      # (payload, flow, gradoutput)
SYMBOLS = ["memc_lp_blend_grad_version", "memc_lp_blend_grad_last_kernel_path",
           "FilterInterpolationBlendLayer_gpu_backward_lp"]
ORDER = BG.ORDER                      # in1, flow, taps, occ, gout, gflow, gtaps, gocc
desc = BG.desc


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(names) == sorted(SYMBOLS), names
    return names


@pytest.fixture(scope="module")
def libs():
    """(the library under test, its mixed sibling)"""
    if not (os.path.exists(LIB) and os.path.exists(MX_LIB)):
        import __graft_entry__
        __graft_entry__.build()
    L, M = ctypes.CDLL(LIB), ctypes.CDLL(MX_LIB)
    L.memc_lp_blend_grad_version.restype = ctypes.c_char_p
    L.memc_lp_blend_grad_last_kernel_path.restype = ctypes.c_char_p
    M.memc_mx_blend_grad_last_kernel_path.restype = ctypes.c_char_p
    for f, ints in ((L.FilterInterpolationBlendLayer_gpu_backward_lp, 3), (M.FilterInterpolationBlendLayer_gpu_backward_mx, 2)):
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * ints + [ctypes.POINTER(BG.Tensor4)] * 8
    return L, M


@pytest.fixture(scope="module")
def lib(libs):
    return libs[0]


class Call:
    """One call: the tensors of a well-formed, covered B x C x H x W call, any of them replaceable; the same descriptors
    go to the mixed sibling (a descriptor holds no dtype)."""

    def __init__(self, libs, B=2, C=3, H=8, W=16, taps=16):
        self.lp = libs[0].FilterInterpolationBlendLayer_gpu_backward_lp
        self.mx = libs[1].FilterInterpolationBlendLayer_gpu_backward_mx
        self.t = {"in1": desc((B, C, H, W)), "flow": desc((B, 2, H, W)), "taps": desc((B, taps, H, W)),
                  "occ": desc((B, 1, H, W)), "gout": desc((B, C, H, W)), "gflow": desc((B, 2, H, W)),
                  "gtaps": desc((B, taps, H, W)), "gocc": desc((B, 1, H, W))}

    def _args(self, repl):
        t = dict(self.t, **repl)
        return [None if t[k] is None else ctypes.byref(t[k]) for k in ORDER]

    def __call__(self, td=F16, fd=F32, gd=F32, **repl):
        """td / fd / gd: the payload, flow and gradoutput dtypes; keywords in1 .. gocc replace a tensor (None: NULL)"""
        return self.lp(None, td, fd, gd, *self._args(repl))

    def sibling(self, td=F16, fd=F32, **repl):
        """the mixed library on the same descriptors (its image and gradoutput are fp32)"""
        return self.mx(None, td, fd, *self._args(repl))


def mutations(call):
    """the descriptor mutations tests/test_mx_blend_grad_abi.py::test_rejects_bad_descriptors lists"""
    m = []
    for k in ORDER:                                           # each of the eight tensors null, or with null data
        m += [{k: None}, {k: desc(tuple(call.t[k].size), data=0)}]
    m += [dict(flow=desc(s), gflow=desc(s)) for s in ((2, 3, 8, 16), (1, 2, 8, 16), (2, 2, 7, 16), (2, 2, 8, 12))]
    m.append(dict(occ=desc((2, 2, 8, 16)), gocc=desc((2, 2, 8, 16))))
    m += [dict(taps=desc((2, k, 8, 16)), gtaps=desc((2, k, 8, 16))) for k in (15, 8, 0)]
    m += [dict(gout=desc((2, 3, 8, 12))), dict(gout=desc((2, 4, 8, 16))),
          dict(gout=desc((2, 3, 8, 16), strides=(800, 200, 20, 1))),
          dict(gflow=desc((2, 2, 8, 12))), dict(gflow=desc((2, 2, 8, 16), strides=(512, 256, 32, 1))),
          dict(gtaps=desc((2, 9, 8, 16))), dict(gtaps=desc((2, 16, 8, 16), strides=(4096, 256, 32, 1))),
          dict(gocc=desc((2, 2, 8, 16))), dict(gocc=desc((2, 1, 8, 16), strides=(256, 256, 32, 1)))]
    w2 = (768, 256, 32, 2)
    m.append(dict(in1=desc((2, 3, 8, 16), strides=w2), gout=desc((2, 3, 8, 16), strides=w2)))
    w2 = (256, 256, 32, 2)
    m.append(dict(occ=desc((2, 1, 8, 16), strides=w2), gocc=desc((2, 1, 8, 16), strides=w2)))
    m += [dict(in1=desc((2, 3, 8, 16), strides=(1 << 33, 128, 16, 1))),
          dict(gflow=desc((2, 2, 8, 16), strides=(256, 1 << 32, 16, 1)))]
    return m


def test_loads_without_a_gpu_and_identifies_itself(lib):
    assert lib.memc_lp_blend_grad_version() == VERSION.encode()
    assert lib.memc_lp_blend_grad_last_kernel_path() == b""     # no call enqueued by this thread yet


def test_exports_exactly_the_header(lib):
    syms = BG._exported(LIB)
    c_surface = sorted(n for n in syms if not BG._is_hip_plumbing(n))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    kernels = [n for n in syms if n.startswith("_ZN4memc")]
    assert any("fi_blend_bwd_c3_lp" in k for k in kernels), kernels
    # its own kernels only: neither the fp32 nor the mixed instantiation of the shared body, not the warp's backward kernels
    assert not [n for n in syms if "fi_blend_bwd_c3I" in n or "fi_blend_bwd_c3_mx" in n or "fi_bwd_c3_" in n]
    # a library of its own: none of its C symbols in any other product library
    other_libs = [p for p in glob.glob(os.path.join(LIBDIR, "libmemc_hip*.so")) if p != LIB]
    assert len(other_libs) >= 8, other_libs               # fp32, measure, lp, lp_grad, blend_grad, mx, mx_grad, mx_blend_grad
    others = {n for p in other_libs for n in BG._exported(p) if not BG._is_hip_plumbing(n)}
    for name in ("FilterInterpolationBlendLayer_gpu_backward", "FilterInterpolationBlendLayer_gpu_backward_mx",
                 "FilterInterpolationBlendLayer_gpu_forward_lp", "FilterInterpolationLayer_gpu_backward_lp"):
        assert name in others, name
    assert not others & set(syms), others & set(syms)


def test_rejects_bad_dtypes(libs):
    call = Call(libs)
    # payload: fp32 (the fp32 library's business) or no dtype at all; flow / gradoutput neither fp32 nor the payload's
    for td, fd, gd in ((F32, F32, F32), (3, F32, F32), (-1, F16, F16), (F16, BF16, F32), (BF16, F16, F32), (F16, 7, F16),
                       (F16, F32, BF16), (BF16, BF16, F16), (F16, F16, 5), (F32, F16, F16)):
        assert call(td, fd, gd) == -1, (td, fd, gd)
    assert libs[0].memc_lp_blend_grad_last_kernel_path() == b""


def test_bad_descriptors_get_the_mixed_library_s_codes(libs):
    """every mutation, every one of the eight dtype triples: the code libmemc_hip_mx_blend_grad.so returns, asked now, for
    the same descriptors with the triple's payload and flow dtypes -- all -1, before the device is touched"""
    call = Call(libs)
    muts = mutations(call)
    assert len(muts) >= 36
    for td, fd, gd in TRIPLES:                             # (the unmutated call is covered: never sent)
        for m in muts:
            want = call.sibling(td, fd, **m)
            assert want == -1, (sorted(m), want)
            assert call(td, fd, gd, **m) == want, (td, fd, gd, sorted(m))
    assert libs[0].memc_lp_blend_grad_last_kernel_path() == b""     # nothing was enqueued
    assert libs[1].memc_mx_blend_grad_last_kernel_path() == b""


def _tap_layout(B, taps, H, W, row=None, data=0x10000):
    row = row or W
    return desc((B, taps, H, W), data=data, strides=(taps * H * row, H * row, row, 1))


UNCOVERED = [("C=4", dict(C=4), {}), ("25 taps", dict(taps=25), {}), ("W=6", dict(W=6), {}), ("W=10", dict(W=10), {}),
             ("taps base 2 bytes off", {}, dict(taps=_tap_layout(2, 16, 8, 16, data=0x10002))),
             ("tap gradient base 2 bytes off", {}, dict(gtaps=_tap_layout(2, 16, 8, 16, data=0x10002))),
             ("image base 4 bytes off", {}, dict(in1=desc((2, 3, 8, 16), data=0x10004))),
             ("taps row stride W+2", {}, dict(taps=_tap_layout(2, 16, 8, 16, row=18), gtaps=_tap_layout(2, 16, 8, 16, row=18))),
             ("image row stride W+2", {}, dict(in1=desc((2, 3, 8, 16), strides=(432, 144, 18, 1)),
                                                gout=desc((2, 3, 8, 16), strides=(432, 144, 18, 1)))),
             # channel 1 of a [B, 2, H, W] half tensor whose planes lie H * W + 2 elements apart: strides that are
             # multiples of four elements, a base four bytes off a quad
             ("occlusion an odd channel slice", {}, dict(occ=desc((2, 1, 8, 16), data=0x10000 + 2 * 130, strides=(260, 130, 16, 1)),
                                                         gocc=desc((2, 1, 8, 16), strides=(260, 130, 16, 1))))]


@pytest.mark.parametrize("case", UNCOVERED, ids=[c[0] for c in UNCOVERED])
def test_calls_outside_the_coverage_are_declined(libs, case):
    """well-formed calls that the tiled kernel does not take: return code 1 for every dtype triple, nothing touched"""
    _label, shape, repl = case
    c = Call(libs, **shape)
    for td, fd, gd in TRIPLES:
        assert c(td, fd, gd, **repl) == 1, (td, fd, gd)
    assert libs[0].memc_lp_blend_grad_last_kernel_path() == b""     # nothing was enqueued


def test_flow_and_gradoutput_alignment_follows_their_storage(libs):
    """a half flow or gradoutput needs 8-byte quads, an fp32 one dwords: a half flow four bytes off a quad and a
    gradoutput two bytes off a dword are declined whatever the rest; so is a plane beyond 32-bit byte offsets"""
    c = Call(libs)
    off4 = dict(flow=desc((2, 2, 8, 16), data=0x10004), gflow=desc((2, 2, 8, 16), data=0x10004))
    off2 = dict(gout=desc((2, 3, 8, 16), data=0x10002))
    for t in (F16, BF16):
        assert c(t, t, F32, **off4) == 1 and c(t, t, t, **off4) == 1      # a half flow four bytes off a quad
        assert c(t, F32, F32, **off2) == 1 and c(t, F32, t, **off2) == 1  # gradoutput two bytes off
    # a plane beyond 32-bit byte offsets: rows 2^21 elements apart, 600 of them
    S, H = 1 << 21, 600
    huge = lambda ch: desc((1, ch, H, 16), strides=(0, H * S, S, 1))      # noqa: E731
    big = Call(libs, B=1, H=H)
    for td, fd, gd in TRIPLES:
        assert big(td, fd, gd, in1=huge(3), gout=huge(3)) == 1
        assert big(td, fd, gd, taps=huge(16), gtaps=huge(16)) == 1
    assert libs[0].memc_lp_blend_grad_last_kernel_path() == b""     # nothing was enqueued


def test_empty_batch_is_a_no_op(libs):
    e = lambda c: desc((0, c, 8, 16), data=0)      # noqa: E731
    for td, fd, gd in TRIPLES:
        assert Call(libs)(td, fd, gd, in1=e(3), flow=e(2), taps=e(16), occ=e(1), gout=e(3), gflow=e(2), gtaps=e(16),
                          gocc=e(1)) == 0
    assert libs[0].memc_lp_blend_grad_last_kernel_path() == b""     # nothing was launched


def test_no_half_blend_backward_kernel_spills():
    """The compiler's own resource remarks: the eight instantiations by name -- 2 payload dtypes x 2 flow dtypes x 2
    gradoutput dtypes -- no private scratch, no dynamic stack, the fp32 kernel's two workgroups of 256 lanes per CU
    (occupancy of at least 2 waves per SIMD, at most 256 VGPRs)."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    from tools import kernel_resources as KR
    kernels = KR.resources_of(UNIT)
    names = sorted(k["name"] for k in kernels)
    want = sorted("memc::fi_blend_bwd_c3_lp<memc::%s, memc::%s, memc::%s>" % (t, f, g)
                  for t in ("F16", "BF16") for f in ("F32", t) for g in ("F32", t))
    assert names == want, names
    bad = [(k["name"], k.get("scratch"), k.get("dynstack"), k.get("occupancy"), k.get("vgprs")) for k in kernels
           if int(k.get("scratch", "0")) > 0 or k.get("dynstack", "False") != "False" or int(k.get("occupancy", "0")) < 2
           or int(k.get("vgprs", "999")) > 256]
    assert not bad, bad
    assert UNIT in KR.SOURCES


# --------------------------------------------------------------------------------------------------------------
# the Python side: a binding of its own
# --------------------------------------------------------------------------------------------------------------
def _bindings():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    import my_package._ext.my_lib_blend_grad as B
    import my_package._ext.my_lib_lp_blend_grad as L
    return B, L


def _tensors(t, ft, gt, **other):
    """the eight tensors of one direction on the CPU (no kernel is reached): dtypes by position, `other` replaces some"""
    import torch
    dt = dict(zip(ORDER, (t, ft, t, t, gt, ft, t, t)), **other)
    shapes = dict(zip(ORDER, (3, 2, 16, 1, 3, 2, 16, 1)))
    return tuple(torch.zeros((1, shapes[k], 8, 16), dtype=dt[k]) for k in ORDER)


def _no_device(monkeypatch, L, seen):
    """keep a CPU tensor from ending the call before the dtype check, and the C function out of reach: it records the
    leading dtype codes instead"""
    import types
    import my_package._ext._satellite as S
    monkeypatch.setattr(S, "describe", lambda t, symbol, position: BG.Tensor4())
    monkeypatch.setattr(S.torch.cuda, "current_stream", lambda dev: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(S.torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(L._SAT, "_lib", types.SimpleNamespace(
        FilterInterpolationBlendLayer_gpu_backward_lp=lambda stream, *a: seen.append(a[:3]) or 0))


def test_the_python_loader_binds_the_library():
    _B, L = _bindings()
    assert L.LIB_PATH == LIB
    assert L.version() == VERSION
    assert L.last_kernel_path() == ""
    assert callable(L.FilterInterpolationBlendLayer_gpu_backward_lp)


def test_the_binding_takes_the_eight_half_patterns(monkeypatch):
    import torch
    _B, L = _bindings()
    seen = []
    _no_device(monkeypatch, L, seen)
    code = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}
    for t in (torch.float16, torch.bfloat16):
        for ft in (torch.float32, t):
            for gt in (torch.float32, t):
                del seen[:]
                assert L.FilterInterpolationBlendLayer_gpu_backward_lp(*_tensors(t, ft, gt)) == 0
                assert seen == [(code[t], code[ft], code[gt])], seen      # the dtype triple, derived from the tensors


def test_the_binding_rejects_fp32_and_mixed_patterns(monkeypatch):
    import torch
    _B, L = _bindings()
    seen = []
    _no_device(monkeypatch, L, seen)
    h, b, f32 = torch.float16, torch.bfloat16, torch.float32
    for args in (_tensors(f32, f32, f32),                                  # the float32 library's call
                 _tensors(h, f32, f32, in1=f32), _tensors(b, b, f32, in1=f32),      # the mixed pattern: a float32 image
                 _tensors(h, b, h), _tensors(b, h, f32), _tensors(h, f32, b),       # another half dtype beside the payload
                 _tensors(h, f32, h, taps=b), _tensors(h, f32, h, occ=f32), _tensors(h, h, h, gflow=f32),
                 _tensors(b, f32, b, gtaps=f32), _tensors(b, f32, b, gocc=h), _tensors(f32, h, h),
                 _tensors(h, f32, h, in1=torch.float64)):
        with pytest.raises(TypeError):
            L.FilterInterpolationBlendLayer_gpu_backward_lp(*args)
    assert not seen


def test_the_blend_backward_door_never_reaches_this_binding(monkeypatch):
    """my_lib_blend_grad's function stays the door of the float32 and mixed kernels only: pure-half tensors are its
    TypeError as before, and nothing of this binding is called"""
    import types
    import torch
    B, L = _bindings()
    reached = []
    monkeypatch.setattr(L, "FilterInterpolationBlendLayer_gpu_backward_lp", lambda *a: reached.append(a) or 0)
    monkeypatch.setattr(L._SAT, "call", lambda *a, **kw: reached.append(a) or 0)
    import my_package._ext._satellite as S
    monkeypatch.setattr(S, "describe", lambda t, symbol, position: BG.Tensor4())
    monkeypatch.setattr(B._SAT, "_lib", types.SimpleNamespace(
        FilterInterpolationBlendLayer_gpu_backward=lambda *a: pytest.fail("the float32 library was called")))
    for t in (torch.float16, torch.bfloat16):
        for ft in (torch.float32, t):
            for gt in (torch.float32, t):
                with pytest.raises(TypeError, match="expected float32"):
                    B.FilterInterpolationBlendLayer_gpu_backward(*_tensors(t, ft, gt))
    assert not reached
    assert not hasattr(B, "my_lib_lp_blend_grad")
