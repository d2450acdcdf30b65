"""What the ctypes bindings of the nineteen satellite libraries share.  All of them: one loader (Library).  The seven warp
libraries (my_lib_lp, my_lib_lp_grad, my_lib_blend_grad, my_lib_mx, my_lib_mx_grad, my_lib_mx_blend_grad,
my_lib_lp_blend_grad), the half projection backwards (my_lib_lp_proj_grad, my_lib_lp_dproj_grad), the half bilinear warp (my_lib_lp_bl) and the stacked
warps and the SPyNet level, its backward and its half forward (my_lib_stack, my_lib_lp_stack, my_lib_spynet, my_lib_spynet_grad and my_lib_spynet_lp, whose entry points take their ints behind the descriptors and make their own calls): the tensor descriptor, the dtype codes and the call through descriptors (Satellite).  The four that
take planes, not NCHW descriptors (my_lib_video, my_lib_ssim, my_lib_video_lp, my_lib_still): the tensor checks and the call
on plain pointers (check, bytes4, planes, call); the sentences that differ between them are handed in.  Importing this loads
nothing."""
import ctypes
import os
import threading

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# memc_dtype of include/memc_warp_lp.h
DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


class Library:
    """One library: lib/<file_name>, loaded once, on first use.  `version_symbol` names its version function, `table` lists
    (symbol, restype, argtypes or None) of its other functions; `no_fallback` ends the message of a call without the library."""

    def __init__(self, file_name, version_symbol, no_fallback, table):
        self.file_name, self.version_symbol, self.no_fallback, self.table = file_name, version_symbol, no_fallback, table
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
                    for name, restype, argtypes in [(self.version_symbol, ctypes.c_char_p, [])] + list(self.table):
                        f = getattr(L, name)
                        f.restype = restype
                        if argtypes is not None:
                            f.argtypes = argtypes
                    self._lib = L
        return self._lib

    def version(self):
        return getattr(self.lib(), self.version_symbol)().decode()


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


class Satellite(Library):
    """A warp library: its version and path functions are <prefix>_version / <prefix>_last_kernel_path and its entry points
    {symbol: (leading ints, tensors)} take a stream, that many memc_dtype and that many descriptors.  `dtype_name` spells an
    expected dtype in a TypeError."""

    def __init__(self, file_name, prefix, no_fallback, entry_points, dtype_name=str):
        table = [(prefix + "_last_kernel_path", ctypes.c_char_p, None)] + [
            (name, ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_int] * ints + [ctypes.POINTER(Tensor4)] * tensors)
            for name, (ints, tensors) in entry_points.items()]
        super().__init__(file_name, prefix + "_version", no_fallback, table)
        self.prefix, self.entry_points, self.dtype_name = prefix, entry_points, dtype_name

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


# ---- the plane bindings: what the C side cannot see of a tensor, checked before data_ptr() and the numbers go over ----

FRAME_IO = "the frame I/O kernels"                 # whose tensors these are, in the message of a CPU tensor


def check(t, name, dtype, numel=None, dev=None, contiguous=True, kernels=FRAME_IO):
    """a (contiguous) CUDA tensor of `dtype` (of `numel` elements, on `dev`)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch.Tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise TypeError("%s: expected a CUDA (HIP) tensor; %s have no CPU path" % (name, kernels))
    if t.dtype != dtype:
        raise TypeError("%s: expected %s, got %s" % (name, dtype, t.dtype))
    if contiguous and not t.is_contiguous():
        raise TypeError("%s: expected a contiguous tensor" % name)
    if numel is not None and t.numel() != numel:
        raise ValueError("%s: expected %d elements, got %d" % (name, numel, t.numel()))
    if dev is not None and t.device != dev:
        raise TypeError("%s: all tensors must live on the same device" % name)


def bytes4(t, name, shape=None, dev=None):
    """a contiguous uint8 CUDA tensor [frames, h, w, 3] (of `shape`, on `dev`) -> its shape"""
    check(t, name, torch.uint8, None, dev)
    if t.dim() != 4 or t.shape[3] != 3 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError("%s: expected shape %s, got %s" % (name, shape or "[frames, h, w, 3]", tuple(t.shape)))
    return tuple(t.shape)


def planes(t, name, shape, dev, dtypes, expected):
    """a CUDA view of `shape` = (frames, 3, rows, cols) with w-stride 1 whose dtype is a key of `dtypes` (on `dev`) ->
    (its value there, the (frame, channel, row) element strides).  `expected` spells those dtypes in the TypeError."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in dtypes:
        raise TypeError("%s: expected a %s" % (name, expected))
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s: expected shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    if dev is not None and t.device != dev:
        raise TypeError("%s: all tensors must live on the same device" % name)
    sf, sc, sr, sw = t.stride()
    if sw != 1 or min(sf, sc, sr) <= 0:
        raise TypeError("%s: expected a w-stride of 1 and positive strides, got %s" % (name, (sf, sc, sr, sw)))
    return dtypes[t.dtype], sf, sc, sr


def call(library, dev, name, *args):
    """name(current stream of `dev`, *args) of a Library"""
    with torch.cuda.device(dev):
        return int(getattr(library.lib(), name)(torch.cuda.current_stream(dev).cuda_stream, *args))
