"""The far side of every guarded row stride, per tensor group, on the CPU: for every (entry point, group) of
tests/_far_views.py's table -- DESIGN.md's "Addressing audit", the guarded rows -- a call whose group sits one quantum
beyond its limit, every other tensor dense, returns the entry point's code (1: not covered, the satellites; -1: refused,
libmemc_hip.so) and enqueues nothing.  The data pointers are made-up numbers, which a refused call never dereferences; the
near stride is not tried here (it would launch): tests/test_gpu_far_views.py runs it on the device.  A guard that forgets
one tensor of one entry point fails its case here."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _far_views as V                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
TAIL_TYPES = {"i": ctypes.c_int, "f": ctypes.c_float, "p": ctypes.c_void_p, "z": ctypes.c_size_t}


class Tensor4(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("size", ctypes.c_int64 * 4), ("stride", ctypes.c_int64 * 4)]


def desc(shape, strides, address):
    t = Tensor4()
    t.data = address
    t.size[:] = shape
    t.stride[:] = strides
    return t


@pytest.fixture(scope="module")
def libs():
    if not os.path.exists(os.path.join(LIBDIR, "libmemc_hip_spynet_grad.so")):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    out = {}
    for name in sorted({e.lib for e in V.ENTRIES.values()}):
        L = ctypes.CDLL(os.path.join(LIBDIR, "libmemc_hip_%s.so" % name if name else "libmemc_hip.so"))
        L.path = getattr(L, "memc_%s_last_kernel_path" % name if name else "memc_last_kernel_path")
        L.path.restype = ctypes.c_char_p
        out[name] = L
    for e in V.ENTRIES.values():
        f = getattr(out[e.lib], e.symbol)
        f.restype = ctypes.c_int
        f.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * len(e.lead) + [ctypes.POINTER(Tensor4)] * len(e.tensors) +
                      [TAIL_TYPES[c] for c in e.tail_types])
    return out


def call(libs, key, layout):
    """(the return code, whether the calling thread's path string is what it was before the call)"""
    e = V.ENTRIES[key]
    d = [desc(*t) for t in layout]
    before = libs[e.lib].path()
    code = getattr(libs[e.lib], e.symbol)(None, *e.lead, *(ctypes.byref(t) for t in d), *e.tail)
    return code, libs[e.lib].path() == before


@pytest.mark.parametrize("key,group", V.GUARDED, ids=["%s-%s" % kg for kg in V.GUARDED])
def test_a_group_beyond_its_limit_is_declined_before_the_device(libs, key, group):
    code, same_path = call(libs, key, V.abi_layout(key, group, "far"))
    assert code == V.ENTRIES[key].code, "%s with its %s tensors at the far stride returned %d" % (key, group, code)
    assert same_path                          # nothing was enqueued: this thread's path string did not change


EMPTY_OK = ["memc.fi_fwd", "memc.fi_bwd", "memc.fi_ctx"]        # (their launchers return 0 for an empty batch)


@pytest.mark.parametrize("key", EMPTY_OK)
def test_the_refusal_is_due_to_the_stride(libs, key):
    """libmemc_hip.so refuses before it looks at the sizes, so an EMPTY call (batch 0: 0, nothing to do) tells the two
    strides apart without a launch: every group under the int rule returns 0 at its near stride, -1 at its far stride.  (The
    context forward's u32 groups are checked by its launcher, behind the empty test.)"""
    groups = [g for g in V.ENTRIES[key].groups if V.rule_of(key, g) is V.fits_int]
    assert len(groups) >= 3
    for group in groups:
        for side, want in (("near", 0), ("far", -1)):
            layout = [((0,) + shape[1:], strides, address) for shape, strides, address in V.abi_layout(key, group, side)]
            code, same_path = call(libs, key, layout)
            assert (code, same_path) == (want, True), (key, group, side, code)
