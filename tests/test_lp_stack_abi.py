"""The stacked half-precision adaptive-warp library libmemc_hip_lp_stack.so (include/memc_warp_lp_stack.h): loads without a
GPU, exports exactly its header, rejects malformed descriptors and dtype codes with -1 and declines every call outside its
coverage with 1, both before the device is touched, and no kernel spills or falls below two workgroups per CU.  CPU only --
no kernel is launched here: the data pointers are made-up numbers, which a refused or declined call never dereferences."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "memc_warp_lp_stack.h")
LIB = os.path.join(ROOT, "memc-net_amd", "lib", "libmemc_hip_lp_stack.so")
ENTRY = "FilterInterpolationStackLayer_gpu_forward_lp"
ERR, DECLINED = -1, 1
F32, F16, BF16 = 0, 1, 2                       # memc_dtype of include/memc_warp_lp.h
N, B, H, W = 6, 2, 16, 24                      # six neighbours of two batch elements


def declared_symbols():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    names = re.findall(r"^\s*(?:const\s+char\s*\*\s*|int\s+)(\w+)\s*\(", text, flags=re.M)
    assert sorted(names) == sorted(["memc_lp_stack_version", "memc_lp_stack_last_kernel_path", ENTRY]), names
    return names


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


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    L = ctypes.CDLL(LIB)
    L.memc_lp_stack_version.restype = ctypes.c_char_p
    L.memc_lp_stack_last_kernel_path.restype = ctypes.c_char_p
    f = getattr(L, ENTRY)
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 2 + [ctypes.POINTER(Tensor4)] * 4 + [ctypes.c_int] * 5
    return L


def call(lib, c=3, ntaps=16, w=W, ctot=64, n=N, c_base=0, skip=3, flow_base=-1, tap_base=-1, payload=BF16, flowt=BF16,
         **over):
    """the entry point on a well-formed, covered call -- VE's shapes in small -- with single things changed"""
    t = {"input1": desc((N * B, c, H, w)), "flow": desc((N * B, 2, H, w)), "taps": desc((N * B, ntaps, H, w)),
         "out": desc((B, ctot, H, w))}
    t.update(over)
    P = ctypes.byref
    return getattr(lib, ENTRY)(None, payload, flowt, P(t["input1"]), P(t["flow"]), P(t["taps"]), P(t["out"]), n, c_base,
                               skip, flow_base, tap_base)


def test_loads_without_a_gpu_and_identifies_itself(lib):
    assert lib.memc_lp_stack_version().startswith(b"memc_hip_lp_stack") and b"gfx950" in lib.memc_lp_stack_version()
    assert lib.memc_lp_stack_last_kernel_path() == b""    # no call enqueued by this thread


def test_exports_exactly_the_header(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], stdout=subprocess.PIPE, text=True, check=True).stdout
    syms = {p[2] for p in (line.split() for line in out.splitlines()) if len(p) == 3}
    c_surface = sorted(n for n in syms if not (n.startswith("_ZN4memc") or n.startswith("__hip_")))
    assert c_surface == sorted(declared_symbols()), set(c_surface) ^ set(declared_symbols())
    assert any("fi_fwd_stack_lp_tiled" in n for n in syms)
    # a library of its own: none of the fp32 stacked library's, the half library's or the fp32 product's kernels and entry points
    assert not [n for n in syms if "fi_fwd_stack_tiledI" in n or "fi_fwd_lp_tiled" in n or "fi_fwd_tiled_fs4" in n
                or n in ("FilterInterpolationStackLayer_gpu_forward", "FilterInterpolationLayer_gpu_forward_lp",
                         "FilterInterpolationLayer_gpu_forward")]


@pytest.mark.parametrize("payload,flowt", [(F16, F16), (F16, F32), (BF16, BF16), (BF16, F32)])
def test_declines_what_the_kernel_does_not_cover(lib, payload, flowt):
    dt = dict(payload=payload, flowt=flowt)
    # overlapping slices: the flow slice inside the warps', the tap slice on the flows', the warps on the taps'
    assert call(lib, flow_base=10, tap_base=40, **dt) == DECLINED      # warps: 0..8 and 12..20 (centre slot 9..11 free)
    assert call(lib, flow_base=21, tap_base=30, ctot=128, **dt) == DECLINED            # flows 21..32, taps 30..125
    assert call(lib, c_base=100, flow_base=0, tap_base=12, ctot=128, **dt) == DECLINED # taps 12..107, warps 100..120
    assert call(lib, skip=-1, flow_base=17, tap_base=40, ctot=160, **dt) == DECLINED   # no centre slot: warps 0..17
    # a slice past Ctot (or before channel 0)
    assert call(lib, ctot=20, **dt) == DECLINED                        # warps need 21 channels with the centre's slot
    assert call(lib, skip=-1, ctot=17, **dt) == DECLINED
    assert call(lib, flow_base=60, ctot=64, **dt) == DECLINED
    assert call(lib, tap_base=32, ctot=127, **dt) == DECLINED
    assert call(lib, c_base=-3, **dt) == DECLINED
    # channel counts, widths, alignment, filter sizes
    assert call(lib, c=5, ctot=64, **dt) == DECLINED
    assert call(lib, c=2, **dt) == DECLINED
    assert call(lib, w=70, ctot=64, **dt) == DECLINED                   # W % 4 != 0
    assert call(lib, w=22, **dt) == DECLINED
    assert call(lib, w=4, **dt) == DECLINED                             # W < 8
    for name, shape in (("input1", (N * B, 3, H, W)), ("flow", (N * B, 2, H, W)), ("taps", (N * B, 16, H, W)),
                        ("out", (B, 64, H, W))):
        assert call(lib, **{name: desc(shape, data=0x10008 + 2)}, **dt) == DECLINED, name  # 8-byte offset + 2 bytes
        assert call(lib, **{name: desc(shape, data=0x10004)}, **dt) == DECLINED, name      # a base that is not 8-byte aligned
        n, c, h, w = shape
        assert call(lib, **{name: desc(shape, strides=(c * h * (w + 2), h * (w + 2), w + 2, 1))}, **dt) == DECLINED, name
    assert call(lib, ntaps=36, **dt) == DECLINED                        # filter size 6
    assert lib.memc_lp_stack_last_kernel_path() == b""                 # nothing was enqueued


def test_what_is_covered_would_reach_the_device(lib):
    """the same calls just inside the coverage pass every host check: with empty tensors they return 0, so the declines
    above are due to the one thing each of them changes"""
    e = lambda shape: desc(shape[:2] + (0, W), data=0)      # noqa: E731
    P = ctypes.byref
    f = getattr(lib, ENTRY)
    args = (P(e((N * B, 3))), P(e((N * B, 2))), P(e((N * B, 16))), P(e((B, 64))))
    for payload, flowt in ((F16, F16), (F16, F32), (BF16, BF16), (BF16, F32)):
        assert f(None, payload, flowt, *args, N, 0, 3, 21, 33) == 0
        assert f(None, payload, flowt, *args, N, 0, -1, 18, 30) == 0


def test_rejects_bad_descriptors_dtypes_and_arguments(lib):
    # dtype codes: a payload that is not a half type, a code that is no dtype, a flow that is neither T nor fp32
    assert call(lib, payload=F32, flowt=F32) == ERR
    assert call(lib, payload=3, flowt=F32) == ERR
    assert call(lib, payload=-1, flowt=F32) == ERR
    assert call(lib, payload=BF16, flowt=7) == ERR
    assert call(lib, payload=BF16, flowt=F16) == ERR
    assert call(lib, payload=F16, flowt=BF16) == ERR
    # the dtype check comes first: a bad code with an empty tensor is still an error
    e = lambda shape: desc(shape[:2] + (0, W), data=0)      # noqa: E731
    P = ctypes.byref
    assert getattr(lib, ENTRY)(None, F32, F32, P(e((N * B, 3))), P(e((N * B, 2))), P(e((N * B, 16))), P(e((B, 64))),
                               N, 0, 3, 21, 33) == ERR
    # N*B not divisible by n_neighbours; no neighbours; out's batch not rows / n_neighbours
    assert call(lib, n=5) == ERR
    assert call(lib, n=0) == ERR
    assert call(lib, n=-6) == ERR
    assert call(lib, n=4) == ERR                                        # 12 rows / 4 = 3 != out's batch of 2
    assert call(lib, out=desc((3, 64, H, W))) == ERR
    # skip outside [-1, n], bases below -1
    assert call(lib, skip=-2) == ERR
    assert call(lib, skip=7) == ERR
    assert call(lib, flow_base=-2) == ERR
    assert call(lib, tap_base=-5) == ERR
    # shapes: the flow, the taps, out's height and width; a tap count that is not a square
    assert call(lib, flow=desc((N * B, 3, H, W))) == ERR
    assert call(lib, flow=desc((N * B - 1, 2, H, W))) == ERR
    assert call(lib, taps=desc((N * B, 16, H, W + 4))) == ERR
    assert call(lib, ntaps=12) == ERR
    assert call(lib, out=desc((B, 64, H + 1, W))) == ERR
    assert call(lib, out=desc((B, 64, H, W - 4))) == ERR
    # a null pointer, a w-stride other than 1, strides beyond int32
    assert call(lib, input1=desc((N * B, 3, H, W), data=0)) == ERR
    assert call(lib, out=desc((B, 64, H, W), data=0)) == ERR
    assert call(lib, out=desc((B, 64, H, W), strides=(64 * H * W * 2, H * W * 2, W * 2, 2))) == ERR
    assert call(lib, taps=desc((N * B, 16, H, W), strides=(1 << 33, H * W, W, 1))) == ERR
    x = desc((N * B, 3, H, W))
    assert getattr(lib, ENTRY)(None, BF16, BF16, P(x), None, P(x), P(x), N, 0, 3, -1, -1) == ERR
    assert lib.memc_lp_stack_last_kernel_path() == b""


def test_binding_imports_without_loading_the_library():
    """in a fresh interpreter: after the import of the binding, the layer and the module no libmemc_hip_lp_stack.so is mapped"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import my_package._ext.my_lib_lp_stack as L\n"
            "import my_package.functions.FilterInterpolationStackLayer, my_package.modules.FilterInterpolationStackModule\n"
            "assert my_package.functions.FilterInterpolationStackLayer.FilterInterpolationStackLayer.native_half in (True, False)\n"
            "assert 'libmemc_hip_lp_stack' not in open('/proc/self/maps').read()\n"
            "assert L.version().startswith('memc_hip_lp_stack')\n"
            "assert L.last_kernel_path() == ''\n"
            "assert 'libmemc_hip_lp_stack' in open('/proc/self/maps').read()\n" % os.path.join(ROOT, "memc-net_amd"))
    subprocess.run([sys.executable, "-c", code], check=True)


def test_kernels_fit_two_workgroups_per_cu_without_scratch():
    """The compiler's own resource remarks: eight instantiations (two payload types, two flow types, RGB or many channels),
    no private scratch, no dynamic stack, at most 256 VGPRs (two workgroups of four waves per CU beside 2 x 49216 bytes
    of LDS)."""
    if not shutil.which("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    sys.path.insert(0, ROOT)
    from tools import kernel_resources as KR
    kernels = KR.resources_of("lp_fi_stack.hip")
    assert len(kernels) == 8, [k["name"] for k in kernels]
    for k in kernels:
        assert int(k.get("scratch", "0")) == 0 and k.get("dynstack", "False") == "False", k
        assert int(k["vgprs"]) <= 256 and int(k["occupancy"]) >= 2, k
