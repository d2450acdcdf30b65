"""What the ctypes bindings of the seven warp libraries among the eleven satellites share (my_lib_lp, my_lib_lp_grad,
my_lib_blend_grad, my_lib_mx, my_lib_mx_grad, my_lib_mx_blend_grad, my_lib_lp_blend_grad; my_lib_video, my_lib_ssim,
my_lib_video_lp and my_lib_still take planes, not NCHW descriptors, and bind themselves): the tensor descriptor, the dtype codes and one loader.  Importing this
loads nothing."""
import ctypes
import os
import threading

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# memc_dtype of include/memc_warp_lp.h
DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


class Tensor4(ctypes.Structure):
    """memc_tensor4 of include/memc_warp.h"""
    _fields_ = [("data", ctypes.c_void_p),
                ("size", ctypes.c_int64 * 4),
                ("stride", ctypes.c_int64 * 4)]


def describe(t, symbol, position):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s arg %d: expected a torch.Tensor, got %s" % (symbol, position, type(t).__name__))
    if not t.is_cuda:
        raise TypeError("%s arg %d: expected a CUDA (HIP) tensor; these operators have no CPU path" % (symbol, position))
    if t.dtype not in DTYPES:
        raise TypeError("%s arg %d: expected float16, bfloat16 or float32, got %s" % (symbol, position, t.dtype))
    if t.dim() != 4:
        raise TypeError("%s arg %d: expected a 4-D NCHW tensor, got %d-D" % (symbol, position, t.dim()))
    d = Tensor4()
    d.data = t.data_ptr()
    d.size[:] = t.shape
    d.stride[:] = t.stride()
    return d


class Satellite:
    """One library: lib/<file_name>, whose version and path functions are <prefix>_version / <prefix>_last_kernel_path and
    whose entry points {symbol: (leading ints, tensors)} take a stream, that many memc_dtype and that many descriptors.
    `no_fallback` ends the message of a call without the library; `dtype_name` spells an expected dtype in a TypeError."""

    def __init__(self, file_name, prefix, no_fallback, entry_points, dtype_name=str):
        self.file_name, self.prefix, self.no_fallback, self.entry_points = file_name, prefix, no_fallback, entry_points
        self.dtype_name = dtype_name
        self.path = os.path.join(_PKG_ROOT, "lib", file_name)
        self._lib = None
        self._lock = threading.Lock()

    def lib(self):
        """The loaded library (loaded once, on first use)."""
        if self._lib is None:
            with self._lock:
                if self._lib is None:
                    if not os.path.exists(self.path):
                        raise RuntimeError(
                            "%s not found at %s -- build it with `make -C %s` (or `python -c 'import "
                            "__graft_entry__ as g; g.build()'` at the repo root); %s"
                            % (self.file_name, self.path, os.path.join(_PKG_ROOT, "csrc"), self.no_fallback))
                    L = ctypes.CDLL(self.path)
                    getattr(L, self.prefix + "_version").restype = ctypes.c_char_p
                    getattr(L, self.prefix + "_last_kernel_path").restype = ctypes.c_char_p
                    for name, (ints, tensors) in self.entry_points.items():
                        f = getattr(L, name)
                        f.restype = ctypes.c_int
                        f.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * ints + [ctypes.POINTER(Tensor4)] * tensors
                    self._lib = L
        return self._lib

    def version(self):
        return getattr(self.lib(), self.prefix + "_version")().decode()

    def last_kernel_path(self):
        return getattr(self.lib(), self.prefix + "_last_kernel_path")().decode()

    def call(self, symbol, leading, tensors, optional=(), dtypes=None):
        """symbol(current stream, the dtype codes of the tensors `leading`, the tensors' descriptors).  A None at a position
        in `optional` goes as NULL.  Where `dtypes` is given, tensors[i] must be of dtypes[i]: the C side sees bytes and
        cannot tell.  (The loop runs per call and per tensor: what only some bindings need stays out of it.)"""
        cfunc = getattr(self._lib or self.lib(), symbol)
        dev = tensors[0].device
        cargs = [None] * len(tensors)
        present = enumerate(tensors)
        if optional:
            present = [(i, t) for i, t in present if t is not None or i not in optional]
        for i, t in present:
            cargs[i] = ctypes.byref(describe(t, symbol, i))
            if t.device != dev:
                raise TypeError("%s: all tensors must live on the same device" % symbol)
        if dtypes is not None:
            for i, t in enumerate(tensors):
                if t is not None and t.dtype != dtypes[i]:
                    raise TypeError("%s arg %d: expected %s, got %s" % (symbol, i, self.dtype_name(dtypes[i]), t.dtype))
        with torch.cuda.device(dev):
            return int(cfunc(torch.cuda.current_stream(dev).cuda_stream, *[DTYPES[t.dtype] for t in leading], *cargs))
