"""ctypes binding of libmemc_hip_video_lp.so (include/memc_video_lp.h): the HD demo loop's frame I/O on the GPU for a network
in float16 / bfloat16 -- I420 decode into a padded input of that storage and quantisation of an output of that storage.
Encode and the scores work on bytes: they stay with my_lib_video.

The library is loaded on first use, not at import.  A call without it raises RuntimeError: there is no fallback to a
float32 decode followed by a cast, nor to the numpy path of networks/yuv_io.py.

This door is half only: a float32 tensor is a TypeError here, as a half tensor is in my_lib_video.  The functions take torch
CUDA tensors, check what the C side cannot see (dtype, device, contiguity, sizes) and hand over data_ptr() and the numbers;
the C dtype (1 float16, 2 bfloat16) is taken from `planes`.  Return value: the C function's int -- 0 enqueued, -1 a failed
check.  Work is enqueued on the current HIP stream of the tensors' device; nothing synchronises.
"""
import ctypes
import os
import threading

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libmemc_hip_video_lp.so")
_lib = None
_lock = threading.Lock()
_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
_DTYPES = {torch.float16: 1, torch.bfloat16: 2}          # memc_dtype's values


def lib():
    """The loaded library (loaded once, on first use)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        "libmemc_hip_video_lp.so not found at %s -- build it with `make -C %s` (or `python -c 'import "
                        "__graft_entry__ as g; g.build()'` at the repo root); the fp16 / bf16 frame I/O has no fallback"
                        % (LIB_PATH, os.path.join(_PKG_ROOT, "csrc")))
                L = ctypes.CDLL(LIB_PATH)
                L.memc_video_lp_version.restype = ctypes.c_char_p
                L.memc_video_lp_version.argtypes = []
                for name, args in (("memc_i420_decode_lp", [_P, _P, _I, _I, _I, _P, _P, _I, _L, _L, _L, _I, _I, _I, _I]),
                                   ("memc_rgb_quantise_lp", [_P, _P, _I, _L, _L, _L, _I, _I, _I, _P])):
                    f = getattr(L, name)
                    f.restype, f.argtypes = ctypes.c_int, args
                _lib = L
    return _lib


def version():
    return lib().memc_video_lp_version().decode()


def frame_bytes(h, w):
    return h * w * 3 // 2


def _check(t, name, dtype, numel=None, dev=None):
    """a contiguous CUDA tensor of `dtype` (of `numel` elements, on `dev`)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch.Tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise TypeError("%s: expected a CUDA (HIP) tensor; the frame I/O kernels have no CPU path" % name)
    if t.dtype != dtype:
        raise TypeError("%s: expected %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise TypeError("%s: expected a contiguous tensor" % name)
    if numel is not None and t.numel() != numel:
        raise ValueError("%s: expected %d elements, got %d" % (name, numel, t.numel()))
    if dev is not None and t.device != dev:
        raise TypeError("%s: all tensors must live on the same device" % name)


def _planes(t, name, frames, rows, cols, dev):
    """a float16 / bfloat16 [frames, 3, rows, cols] view with w-stride 1 -> (C dtype, its (frame, channel, row) element
    strides)"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in _DTYPES:
        raise TypeError("%s: expected a float16 or bfloat16 CUDA (HIP) tensor (float32 planes go through my_lib_video)" % name)
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


def i420_decode(i420, frames, h, w, rgb=None, planes=None, pads=(0, 0, 0, 0)):
    """`frames` I420 frames (uint8, frames * h*w*3/2 bytes) -> rgb: uint8 [frames, h, w, 3] and / or planes: a float16 or
    bfloat16 [frames, 3, h + top + bottom, w + left + right] view (w-stride 1, e.g. a slice of the network's input) that
    receives (float32(byte) / 255).to(planes.dtype), replicate-padded by pads = (left, right, top, bottom).  Without planes
    the bytes do not depend on a dtype (float16 is handed over)."""
    _check(i420, "i420", torch.uint8, frames * frame_bytes(h, w))
    dev = i420.device
    left, right, top, bottom = (int(p) for p in pads)
    if rgb is not None:
        _check(rgb, "rgb", torch.uint8, frames * h * w * 3, dev)
    dtype, sf, sc, sr = 1, 0, 0, 0
    if planes is not None:
        dtype, sf, sc, sr = _planes(planes, "planes", frames, h + top + bottom, w + left + right, dev)
    return _call(dev, "memc_i420_decode_lp", i420.data_ptr(), frames, h, w, None if rgb is None else rgb.data_ptr(),
                 None if planes is None else planes.data_ptr(), dtype, sf, sc, sr, left, right, top, bottom)


def rgb_quantise(planes, rgb):
    """a float16 or bfloat16 [frames, 3, h, w] view (w-stride 1, e.g. the crop of the network's output) -> rgb: uint8
    [frames, h, w, 3], round-half-even of 255 * clamp(float32(x), 0, 1)."""
    if not isinstance(planes, torch.Tensor) or planes.dim() != 4:
        raise TypeError("planes: expected a 4-D torch.Tensor")
    frames, _c, h, w = planes.shape
    dtype, sf, sc, sr = _planes(planes, "planes", frames, h, w, None)
    _check(rgb, "rgb", torch.uint8, frames * h * w * 3, planes.device)
    return _call(planes.device, "memc_rgb_quantise_lp", planes.data_ptr(), dtype, sf, sc, sr, frames, h, w, rgb.data_ptr())


__all__ = ["LIB_PATH", "lib", "version", "frame_bytes", "i420_decode", "rgb_quantise"]
