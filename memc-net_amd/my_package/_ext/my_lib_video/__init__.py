"""ctypes binding of libmemc_hip_video.so (include/memc_video.h): the HD demo loop's frame I/O on the GPU -- I420 decode
into the network's padded input, quantisation of its output, I420 encode and the luma scores.

The library is loaded on first use, not at import.  A call without it raises RuntimeError: there is no fallback to the
numpy path of networks/yuv_io.py for a missing library (that path is chosen by its caller, never silently).

The C functions take plain pointers and ints; the functions here take torch CUDA tensors, check what the C side cannot see
(dtype, device, contiguity, sizes) and hand over data_ptr() and the numbers.  Return value: the C function's int -- 0
enqueued, -1 a failed check.  Work is enqueued on the current HIP stream of the tensors' device; nothing synchronises.
"""
import ctypes
import os
import threading

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libmemc_hip_video.so")
_lib = None
_lock = threading.Lock()
_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64


def lib():
    """The loaded library (loaded once, on first use)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        "libmemc_hip_video.so not found at %s -- build it with `make -C %s` (or `python -c 'import "
                        "__graft_entry__ as g; g.build()'` at the repo root); the GPU frame I/O has no fallback"
                        % (LIB_PATH, os.path.join(_PKG_ROOT, "csrc")))
                L = ctypes.CDLL(LIB_PATH)
                L.memc_video_version.restype = ctypes.c_char_p
                L.memc_video_version.argtypes = []
                for name, args in (("memc_i420_decode", [_P, _P, _I, _I, _I, _P, _P, _L, _L, _L, _I, _I, _I, _I]),
                                   ("memc_rgb_quantise", [_P, _P, _L, _L, _L, _I, _I, _I, _P]),
                                   ("memc_i420_encode", [_P, _P, _I, _I, _I, _P]),
                                   ("memc_luma_score", [_P, _P, _P, _I, _I, _I, _P, _P, ctypes.c_size_t])):
                    f = getattr(L, name)
                    f.restype, f.argtypes = ctypes.c_int, args
                L.memc_luma_score_workspace_bytes.restype = ctypes.c_size_t
                L.memc_luma_score_workspace_bytes.argtypes = [_I, _I, _I]
                _lib = L
    return _lib


def version():
    return lib().memc_video_version().decode()


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
    """a float32 [frames, 3, rows, cols] view with w-stride 1 -> its (frame, channel, row) element strides"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise TypeError("%s: expected a float32 CUDA (HIP) tensor" % name)
    if tuple(t.shape) != (frames, 3, rows, cols):
        raise ValueError("%s: expected shape %s, got %s" % (name, (frames, 3, rows, cols), tuple(t.shape)))
    if t.device != dev:
        raise TypeError("%s: all tensors must live on the same device" % name)
    sf, sc, sr, sw = t.stride()
    if sw != 1 or min(sf, sc, sr) <= 0:
        raise TypeError("%s: expected a w-stride of 1 and positive strides, got %s" % (name, (sf, sc, sr, sw)))
    return sf, sc, sr


def _call(dev, name, *args):
    with torch.cuda.device(dev):
        return int(getattr(lib(), name)(torch.cuda.current_stream(dev).cuda_stream, *args))


def i420_decode(i420, frames, h, w, rgb=None, planes=None, pads=(0, 0, 0, 0)):
    """`frames` I420 frames (uint8, frames * h*w*3/2 bytes) -> rgb: uint8 [frames, h, w, 3] and / or planes: a float32
    [frames, 3, h + top + bottom, w + left + right] view (w-stride 1, e.g. a slice of the network's input) that receives
    float32(byte) / 255, replicate-padded by pads = (left, right, top, bottom)."""
    _check(i420, "i420", torch.uint8, frames * frame_bytes(h, w))
    dev = i420.device
    left, right, top, bottom = (int(p) for p in pads)
    if rgb is not None:
        _check(rgb, "rgb", torch.uint8, frames * h * w * 3, dev)
    sf = sc = sr = 0
    if planes is not None:
        sf, sc, sr = _planes(planes, "planes", frames, h + top + bottom, w + left + right, dev)
    return _call(dev, "memc_i420_decode", i420.data_ptr(), frames, h, w, None if rgb is None else rgb.data_ptr(),
                 None if planes is None else planes.data_ptr(), sf, sc, sr, left, right, top, bottom)


def rgb_quantise(planes, rgb):
    """a float32 [frames, 3, h, w] view (w-stride 1, e.g. the crop of the network's output) -> rgb: uint8
    [frames, h, w, 3], round-half-even of 255 * clamp(x, 0, 1)."""
    if not isinstance(planes, torch.Tensor) or planes.dim() != 4:
        raise TypeError("planes: expected a 4-D torch.Tensor")
    frames, _c, h, w = planes.shape
    sf, sc, sr = _planes(planes, "planes", frames, h, w, planes.device)
    _check(rgb, "rgb", torch.uint8, frames * h * w * 3, planes.device)
    return _call(planes.device, "memc_rgb_quantise", planes.data_ptr(), sf, sc, sr, frames, h, w, rgb.data_ptr())


def i420_encode(rgb, frames, h, w, i420):
    """rgb: uint8 [frames, h, w, 3] -> i420: uint8, frames * h*w*3/2 bytes."""
    _check(rgb, "rgb", torch.uint8, frames * h * w * 3)
    _check(i420, "i420", torch.uint8, frames * frame_bytes(h, w), rgb.device)
    return _call(rgb.device, "memc_i420_encode", rgb.data_ptr(), frames, h, w, i420.data_ptr())


def luma_score_workspace_bytes(frames, h, w):
    return int(lib().memc_luma_score_workspace_bytes(frames, h, w))


def luma_score(rgb_a, rgb_b, frames, h, w, sums, workspace):
    """sums: int64 [frames, 2] receives, per frame, the uint64 sums of |dY| and dY^2 over the truncated 8-bit luma planes
    of two uint8 [frames, h, w, 3]; workspace: uint8, at least luma_score_workspace_bytes(frames, h, w) bytes."""
    _check(rgb_a, "rgb_a", torch.uint8, frames * h * w * 3)
    dev = rgb_a.device
    _check(rgb_b, "rgb_b", torch.uint8, frames * h * w * 3, dev)
    _check(sums, "sums", torch.int64, frames * 2, dev)
    _check(workspace, "workspace", torch.uint8, None, dev)
    return _call(dev, "memc_luma_score", rgb_a.data_ptr(), rgb_b.data_ptr(), frames, h, w, sums.data_ptr(),
                 workspace.data_ptr(), workspace.numel())


__all__ = ["LIB_PATH", "lib", "version", "frame_bytes", "i420_decode", "rgb_quantise", "i420_encode",
           "luma_score_workspace_bytes", "luma_score"]
