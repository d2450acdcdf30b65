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

import torch

from .._satellite import DTYPES as _DTYPES, Library, bytes4 as _bytes, call as _call, planes as _planes_of

_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
_LIB = Library("libmemc_hip_still.so", "memc_still_version", "the still-image GPU frame I/O has no fallback",
               [("memc_rgb8_decode", _I, [_P, _P, _I, _I, _I, _P, _I, _L, _L, _L, _I, _I, _I, _I]),
                ("memc_rgb8_quantise", _I, [_P, _P, _I, _L, _L, _L, _I, _I, _I, _P]),
                ("memc_rgb8_score", _I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, ctypes.c_size_t]),
                ("memc_rgb8_score_workspace_bytes", ctypes.c_size_t, [_I, _I, _I])])
LIB_PATH, lib, version = _LIB.path, _LIB.lib, _LIB.version


def _planes(t, name, frames, rows, cols, dev):
    """a float32 / float16 / bfloat16 [frames, 3, rows, cols] view with w-stride 1 -> (C dtype, its (frame, channel, row)
    element strides)"""
    return _planes_of(t, name, (frames, 3, rows, cols), dev, _DTYPES, "float32, float16 or bfloat16 CUDA (HIP) tensor")


def rgb8_decode(rgb, planes, pads=(0, 0, 0, 0)):
    """rgb: uint8 [frames, h, w, 3] -> planes: a float32, float16 or bfloat16 [frames, 3, h + top + bottom, w + left + right]
    view (w-stride 1, e.g. a slice of the network's input) that receives (float32(byte) / 255).to(planes.dtype),
    replicate-padded by pads = (left, right, top, bottom)."""
    frames, h, w, _c = _bytes(rgb, "rgb")
    left, right, top, bottom = (int(p) for p in pads)
    dtype, sf, sc, sr = _planes(planes, "planes", frames, h + top + bottom, w + left + right, rgb.device)
    return _call(_LIB, rgb.device, "memc_rgb8_decode", rgb.data_ptr(), frames, h, w, planes.data_ptr(), dtype, sf, sc, sr, left,
                 right, top, bottom)


def rgb8_quantise(planes, rgb):
    """a float32, float16 or bfloat16 [frames, 3, h, w] view (w-stride 1, e.g. the crop of the network's output) -> rgb: uint8
    [frames, h, w, 3], round-half-even of 255 * clamp(float32(x), 0, 1)."""
    if not isinstance(planes, torch.Tensor) or planes.dim() != 4:
        raise TypeError("planes: expected a 4-D torch.Tensor")
    frames, _c, h, w = planes.shape
    dtype, sf, sc, sr = _planes(planes, "planes", frames, h, w, None)
    _bytes(rgb, "rgb", (frames, h, w, 3), planes.device)
    return _call(_LIB, planes.device, "memc_rgb8_quantise", planes.data_ptr(), dtype, sf, sc, sr, frames, h, w, rgb.data_ptr())


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
    return _call(_LIB, dev, "memc_rgb8_score", a.data_ptr(), b.data_ptr(), frames, h, w, sums.data_ptr(),
                 None if diff is None else diff.data_ptr(), work.data_ptr(), work.numel())


__all__ = ["LIB_PATH", "lib", "version", "rgb8_decode", "rgb8_quantise", "rgb8_score_workspace_bytes", "rgb8_score"]
