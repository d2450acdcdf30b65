"""float64 front-end of the CPU checker built once more with every `float` a `double` (oracle/Makefile: libmemc_oracle64.so).

TEST INFRASTRUCTURE ONLY, and CPU tests only: tests/test_exact_inputs.py uses it to prove that the exact-arithmetic inputs
of tests/_exact.py round nowhere -- the fp32 build and this one must then return the same numbers.  Same functions and
argument order as oracle/memc_oracle.py; arrays go in as float64 (element strides, as the C side takes them) and come
back as float64.  The GPU tests never load it.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libmemc_oracle64.so")
_lib = None

_D = ctypes.POINTER(ctypes.c_double)


def build(force=False):
    src = os.path.join(_HERE, "memc_oracle.c")
    if not force and os.path.exists(_LIB_PATH) and os.path.getmtime(_LIB_PATH) >= os.path.getmtime(src):
        return _LIB_PATH
    subprocess.run(["make", "-C", _HERE, "-B", "libmemc_oracle64.so"], check=True, stdout=subprocess.DEVNULL)
    return _LIB_PATH


def lib():
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(_LIB_PATH)
    return _lib


def _prep(a):
    a = np.ascontiguousarray(np.asarray(a), dtype=np.float64)
    if a.ndim != 4:
        raise ValueError("expected a 4-D NCHW array")
    return a


def _ptr(a):
    return a.ctypes.data_as(_D)


def _str(a):
    return (ctypes.c_int64 * 4)(*[s // 8 for s in a.strides])


def _dims(a):
    return [ctypes.c_int(int(v)) for v in a.shape]


def _check(err, name):
    if err != 0:
        raise RuntimeError("%s (float64 build) returned %d" % (name, err))


def filter_interpolation_forward(x, flow, filt):
    x, flow, filt = _prep(x), _prep(flow), _prep(filt)
    out = np.zeros(x.shape, np.float64)
    B, C, H, W = _dims(x)
    _check(lib().memc_oracle_filter_interpolation_forward(
        B, C, H, W, ctypes.c_int(filt.shape[1]), _ptr(x), _str(x), _ptr(flow), _str(flow), _ptr(filt), _str(filt),
        _ptr(out), _str(out)), "filter_interpolation_forward")
    return out


def filter_interpolation_backward(x, flow, filt, gout):
    x, flow, filt, gout = _prep(x), _prep(flow), _prep(filt), _prep(gout)
    g1, g2, g3 = np.zeros(x.shape, np.float64), np.zeros(flow.shape, np.float64), np.zeros(filt.shape, np.float64)
    B, C, H, W = _dims(x)
    _check(lib().memc_oracle_filter_interpolation_backward(
        B, C, H, W, ctypes.c_int(filt.shape[1]), _ptr(x), _str(x), _ptr(flow), _str(flow), _ptr(filt), _str(filt),
        _ptr(gout), _ptr(g1), _ptr(g2), _ptr(g3)), "filter_interpolation_backward")
    return g1, g2, g3


def _bilinear_forward(name, x, flow):
    x, flow = _prep(x), _prep(flow)
    out = np.zeros(x.shape, np.float64)
    B, C, H, W = _dims(x)
    _check(getattr(lib(), name)(B, C, H, W, _ptr(x), _str(x), _ptr(flow), _str(flow), _ptr(out), _str(out)), name)
    return out


def _bilinear_backward(name, x, flow, gout):
    x, flow, gout = _prep(x), _prep(flow), _prep(gout)
    g1, g2 = np.zeros(x.shape, np.float64), np.zeros(flow.shape, np.float64)
    B, C, H, W = _dims(x)
    _check(getattr(lib(), name)(B, C, H, W, _ptr(x), _str(x), _ptr(flow), _str(flow), _ptr(gout), _ptr(g1), _ptr(g2)), name)
    return g1, g2


def interpolation_forward(x, flow):
    return _bilinear_forward("memc_oracle_interpolation_forward", x, flow)


def interpolation_backward(x, flow, gout):
    return _bilinear_backward("memc_oracle_interpolation_backward", x, flow, gout)


def interpolation_ch_forward(x, flow):
    return _bilinear_forward("memc_oracle_interpolation_ch_forward", x, flow)


def interpolation_ch_backward(x, flow, gout):
    return _bilinear_backward("memc_oracle_interpolation_ch_backward", x, flow, gout)


def _projection_forward(name, flow, depth, fillhole):
    flow = _prep(flow)
    out = np.zeros(flow.shape, np.float64)
    count = np.zeros((flow.shape[0], 1, flow.shape[2], flow.shape[3]), np.float64)
    B, C, H, W = _dims(flow)
    mid = () if depth is None else (_ptr(depth), _str(depth))
    _check(getattr(lib(), name)(B, C, H, W, _ptr(flow), _str(flow), *mid, _ptr(count), _str(count), _ptr(out), _str(out),
                                ctypes.c_int(int(fillhole))), name)
    return out, count


def flow_projection_forward(flow, fillhole=0):
    return _projection_forward("memc_oracle_flow_projection_forward", flow, None, fillhole)


def depth_flow_projection_forward(flow, depth, fillhole=0):
    return _projection_forward("memc_oracle_depth_flow_projection_forward", flow, _prep(depth), fillhole)


def flow_projection_backward(flow, count, gout):
    flow, count, gout = _prep(flow), _prep(count), _prep(gout)
    g1 = np.zeros(flow.shape, np.float64)
    B, C, H, W = _dims(flow)
    _check(lib().memc_oracle_flow_projection_backward(
        B, C, H, W, _ptr(flow), _str(flow), _ptr(count), _str(count), _ptr(gout), _ptr(g1)), "flow_projection_backward")
    return g1


def depth_flow_projection_backward(flow, depth, count, out, gout):
    flow, depth, count, out, gout = _prep(flow), _prep(depth), _prep(count), _prep(out), _prep(gout)
    g1, g2 = np.zeros(flow.shape, np.float64), np.zeros(depth.shape, np.float64)
    B, C, H, W = _dims(flow)
    _check(lib().memc_oracle_depth_flow_projection_backward(
        B, C, H, W, _ptr(flow), _str(flow), _ptr(depth), _str(depth), _ptr(count), _str(count), _ptr(out), _ptr(gout),
        _ptr(g1), _ptr(g2)), "depth_flow_projection_backward")
    return g1, g2
