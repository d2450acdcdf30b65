"""ctypes binding of libmemc_hip_still.so (include/memc_still.h): the still-image demo loop's frame I/O and scores on the GPU
-- interleaved 8-bit RGB pictures of any height and width into the network's padded planar input, quantisation of its
output back to such bytes, and the integer sums of the RGB scores with the difference picture.

The library is loaded on first use, not at import.  A call without it raises RuntimeError: there is no fallback to the
numpy path of networks/png_io.py for a missing library (that path is chosen by its caller, never silently).

One door for all three storages: the functions take torch CUDA tensors, check what the C side cannot see (dtype, device,
contiguity, shape, w-stride 1) and hand over data_ptr() and the numbers; the C dtype (0 float32, 1 float16, 2 bfloat16) is
taken from `planes`.  Return value: the C function's int -- 0 enqueued, -1 a failed check.  Work is enqueued on the current
HIP stream of the tensors' device; nothing synchronises.
"""
import ctypes
import os
import threading

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libmemc_hip_still.so")
_lib = None
_lock = threading.Lock()
_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
_DTYPES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}          # memc_dtype's values


def lib():
    """The loaded library (loaded once, on first use)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        "libmemc_hip_still.so not found at %s -- build it with `make -C %s` (or `python -c 'import "
                        "__graft_entry__ as g; g.build()'` at the repo root); the still-image GPU frame I/O has no fallback"
                        % (LIB_PATH, os.path.join(_PKG_ROOT, "csrc")))
                L = ctypes.CDLL(LIB_PATH)
                L.memc_still_version.restype = ctypes.c_char_p
                L.memc_still_version.argtypes = []
                for name, args in (("memc_rgb8_decode", [_P, _P, _I, _I, _I, _P, _I, _L, _L, _L, _I, _I, _I, _I]),
                                   ("memc_rgb8_quantise", [_P, _P, _I, _L, _L, _L, _I, _I, _I, _P]),
                                   ("memc_rgb8_score", [_P, _P, _P, _I, _I, _I, _P, _P, _P, ctypes.c_size_t])):
                    f = getattr(L, name)
                    f.restype, f.argtypes = ctypes.c_int, args
                L.memc_rgb8_score_workspace_bytes.restype = ctypes.c_size_t
                L.memc_rgb8_score_workspace_bytes.argtypes = [_I, _I, _I]
                _lib = L
    return _lib


def version():
    return lib().memc_still_version().decode()


def _bytes(t, name, shape=None, dev=None):
    """a contiguous uint8 CUDA tensor [frames, h, w, 3] (of `shape`, on `dev`) -> its shape"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch.Tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise TypeError("%s: expected a CUDA (HIP) tensor; the frame I/O kernels have no CPU path" % name)
    if t.dtype != torch.uint8:
        raise TypeError("%s: expected torch.uint8, got %s" % (name, t.dtype))
    if not t.is_contiguous():
        raise TypeError("%s: expected a contiguous tensor" % name)
    if dev is not None and t.device != dev:
        raise TypeError("%s: all tensors must live on the same device" % name)
    if t.dim() != 4 or t.shape[3] != 3 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError("%s: expected shape %s, got %s" % (name, shape or "[frames, h, w, 3]", tuple(t.shape)))
    return tuple(t.shape)


def _planes(t, name, frames, rows, cols, dev):
    """a float32 / float16 / bfloat16 [frames, 3, rows, cols] view with w-stride 1 -> (C dtype, its (frame, channel, row)
    element strides)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in _DTYPES:
        raise TypeError("%s: expected a float32, float16 or bfloat16 CUDA (HIP) tensor" % name)
    if tuple(t.shape) != (frames, 3, rows, cols):
        raise ValueError("%s: expected shape %s, got %s" % (name, (frames, 3, rows, cols), tuple(t.shape)))
    if dev is not None and t.device != dev:
        raise TypeError("%s: all tensors must live on the same device" % name)
    sf, sc, sr, sw = t.stride()
    if sw != 1 or min(sf, sc, sr) <= 0:
        raise TypeError("%s: expected a w-stride of 1 and positive strides, got %s" % (name, (sf, sc, sr, sw)))
    return _DTYPES[t.dtype], sf, sc, sr


def _call(dev, name, *args):
    with torch.cuda.device(dev):
        return int(getattr(lib(), name)(torch.cuda.current_stream(dev).cuda_stream, *args))


def rgb8_decode(rgb, planes, pads=(0, 0, 0, 0)):
    """rgb: uint8 [frames, h, w, 3] -> planes: a float32, float16 or bfloat16 [frames, 3, h + top + bottom, w + left + right]
    view (w-stride 1, e.g. a slice of the network's input) that receives (float32(byte) / 255).to(planes.dtype),
    replicate-padded by pads = (left, right, top, bottom)."""
    frames, h, w, _c = _bytes(rgb, "rgb")
    left, right, top, bottom = (int(p) for p in pads)
    dtype, sf, sc, sr = _planes(planes, "planes", frames, h + top + bottom, w + left + right, rgb.device)
    return _call(rgb.device, "memc_rgb8_decode", rgb.data_ptr(), frames, h, w, planes.data_ptr(), dtype, sf, sc, sr, left,
                 right, top, bottom)


def rgb8_quantise(planes, rgb):
    """a float32, float16 or bfloat16 [frames, 3, h, w] view (w-stride 1, e.g. the crop of the network's output) -> rgb: uint8
    [frames, h, w, 3], round-half-even of 255 * clamp(float32(x), 0, 1)."""
    if not isinstance(planes, torch.Tensor) or planes.dim() != 4:
        raise TypeError("planes: expected a 4-D torch.Tensor")
    frames, _c, h, w = planes.shape
    dtype, sf, sc, sr = _planes(planes, "planes", frames, h, w, None)
    _bytes(rgb, "rgb", (frames, h, w, 3), planes.device)
    return _call(planes.device, "memc_rgb8_quantise", planes.data_ptr(), dtype, sf, sc, sr, frames, h, w, rgb.data_ptr())


def rgb8_score_workspace_bytes(frames, h, w):
    return int(lib().memc_rgb8_score_workspace_bytes(frames, h, w))


def rgb8_score(a, b, sums, work, diff=None):
    """sums: int64 [frames, 2] receives, per frame, the uint64 sums of |a - b| and (a - b)^2 over all samples of two uint8
    [frames, h, w, 3]; diff (optional): uint8 [frames, h, w, 3] receives (128 + a - b) mod 256; work: uint8, at least
    rgb8_score_workspace_bytes(frames, h, w) bytes, 8-byte aligned."""
    shape = _bytes(a, "a")
    dev = a.device
    _bytes(b, "b", shape, dev)
    if diff is not None:
        _bytes(diff, "diff", shape, dev)
    frames, h, w, _c = shape
    for t, name, dtype in ((sums, "sums", torch.int64), (work, "work", torch.uint8)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise TypeError("%s: expected a contiguous %s CUDA (HIP) tensor" % (name, dtype))
        if t.device != dev:
            raise TypeError("%s: all tensors must live on the same device" % name)
    if sums.numel() != 2 * frames:
        raise ValueError("sums: expected %d elements, got %d" % (2 * frames, sums.numel()))
    return _call(dev, "memc_rgb8_score", a.data_ptr(), b.data_ptr(), frames, h, w, sums.data_ptr(),
                 None if diff is None else diff.data_ptr(), work.data_ptr(), work.numel())


__all__ = ["LIB_PATH", "lib", "version", "rgb8_decode", "rgb8_quantise", "rgb8_score_workspace_bytes", "rgb8_score"]
