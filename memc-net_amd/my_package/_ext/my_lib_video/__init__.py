"""ctypes binding of libmemc_hip_video.so (include/memc_video.h): the HD demo loop's frame I/O on the GPU -- I420 decode
into the network's padded input, quantisation of its output, I420 encode and the luma scores.

The library is loaded on first use, not at import.  A call without it raises RuntimeError: there is no fallback to the
numpy path of networks/yuv_io.py for a missing library (that path is chosen by its caller, never silently).

The C functions take plain pointers and ints; the functions here take torch CUDA tensors, check what the C side cannot see
(dtype, device, contiguity, sizes) and hand over data_ptr() and the numbers.  Return value: the C function's int -- 0
enqueued, -1 a failed check.  Work is enqueued on the current HIP stream of the tensors' device; nothing synchronises.
"""
import ctypes

import torch

from .._satellite import Library, call as _call, check as _check, planes as _planes_of

_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
_LIB = Library("libmemc_hip_video.so", "memc_video_version", "the GPU frame I/O has no fallback",
               [("memc_i420_decode", _I, [_P, _P, _I, _I, _I, _P, _P, _L, _L, _L, _I, _I, _I, _I]),
                ("memc_rgb_quantise", _I, [_P, _P, _L, _L, _L, _I, _I, _I, _P]),
                ("memc_i420_encode", _I, [_P, _P, _I, _I, _I, _P]),
                ("memc_luma_score", _I, [_P, _P, _P, _I, _I, _I, _P, _P, ctypes.c_size_t]),
                ("memc_luma_score_workspace_bytes", ctypes.c_size_t, [_I, _I, _I])])
LIB_PATH, lib, version = _LIB.path, _LIB.lib, _LIB.version


def frame_bytes(h, w):
    return h * w * 3 // 2


def _planes(t, name, frames, rows, cols, dev):
    """a float32 [frames, 3, rows, cols] view with w-stride 1 -> its (frame, channel, row) element strides"""
    return _planes_of(t, name, (frames, 3, rows, cols), dev, {torch.float32: 0}, "float32 CUDA (HIP) tensor")[1:]


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
    return _call(_LIB, dev, "memc_i420_decode", i420.data_ptr(), frames, h, w, None if rgb is None else rgb.data_ptr(),
                 None if planes is None else planes.data_ptr(), sf, sc, sr, left, right, top, bottom)


def rgb_quantise(planes, rgb):
    """a float32 [frames, 3, h, w] view (w-stride 1, e.g. the crop of the network's output) -> rgb: uint8
    [frames, h, w, 3], round-half-even of 255 * clamp(x, 0, 1)."""
    if not isinstance(planes, torch.Tensor) or planes.dim() != 4:
        raise TypeError("planes: expected a 4-D torch.Tensor")
    frames, _c, h, w = planes.shape
    sf, sc, sr = _planes(planes, "planes", frames, h, w, planes.device)
    _check(rgb, "rgb", torch.uint8, frames * h * w * 3, planes.device)
    return _call(_LIB, planes.device, "memc_rgb_quantise", planes.data_ptr(), sf, sc, sr, frames, h, w, rgb.data_ptr())


def i420_encode(rgb, frames, h, w, i420):
    """rgb: uint8 [frames, h, w, 3] -> i420: uint8, frames * h*w*3/2 bytes."""
    _check(rgb, "rgb", torch.uint8, frames * h * w * 3)
    _check(i420, "i420", torch.uint8, frames * frame_bytes(h, w), rgb.device)
    return _call(_LIB, rgb.device, "memc_i420_encode", rgb.data_ptr(), frames, h, w, i420.data_ptr())


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
    return _call(_LIB, dev, "memc_luma_score", rgb_a.data_ptr(), rgb_b.data_ptr(), frames, h, w, sums.data_ptr(),
                 workspace.data_ptr(), workspace.numel())


__all__ = ["LIB_PATH", "lib", "version", "frame_bytes", "i420_decode", "rgb_quantise", "i420_encode",
           "luma_score_workspace_bytes", "luma_score"]
