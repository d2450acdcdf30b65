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

import torch

from .._satellite import Library, call as _call, check as _check, planes as _planes_of

_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
_DTYPES = {torch.float16: 1, torch.bfloat16: 2}          # memc_dtype's values
_LIB = Library("libmemc_hip_video_lp.so", "memc_video_lp_version", "the fp16 / bf16 frame I/O has no fallback",
               [("memc_i420_decode_lp", _I, [_P, _P, _I, _I, _I, _P, _P, _I, _L, _L, _L, _I, _I, _I, _I]),
                ("memc_rgb_quantise_lp", _I, [_P, _P, _I, _L, _L, _L, _I, _I, _I, _P])])
LIB_PATH, lib, version = _LIB.path, _LIB.lib, _LIB.version


def frame_bytes(h, w):
    return h * w * 3 // 2


def _planes(t, name, frames, rows, cols, dev):
    """a float16 / bfloat16 [frames, 3, rows, cols] view with w-stride 1 -> (C dtype, its (frame, channel, row) element
    strides)"""
    return _planes_of(t, name, (frames, 3, rows, cols), dev, _DTYPES,
                      "float16 or bfloat16 CUDA (HIP) tensor (float32 planes go through my_lib_video)")


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
    return _call(_LIB, dev, "memc_i420_decode_lp", i420.data_ptr(), frames, h, w, None if rgb is None else rgb.data_ptr(),
                 None if planes is None else planes.data_ptr(), dtype, sf, sc, sr, left, right, top, bottom)


def rgb_quantise(planes, rgb):
    """a float16 or bfloat16 [frames, 3, h, w] view (w-stride 1, e.g. the crop of the network's output) -> rgb: uint8
    [frames, h, w, 3], round-half-even of 255 * clamp(float32(x), 0, 1)."""
    if not isinstance(planes, torch.Tensor) or planes.dim() != 4:
        raise TypeError("planes: expected a 4-D torch.Tensor")
    frames, _c, h, w = planes.shape
    dtype, sf, sc, sr = _planes(planes, "planes", frames, h, w, None)
    _check(rgb, "rgb", torch.uint8, frames * h * w * 3, planes.device)
    return _call(_LIB, planes.device, "memc_rgb_quantise_lp", planes.data_ptr(), dtype, sf, sc, sr, frames, h, w, rgb.data_ptr())


__all__ = ["LIB_PATH", "lib", "version", "frame_bytes", "i420_decode", "rgb_quantise"]
