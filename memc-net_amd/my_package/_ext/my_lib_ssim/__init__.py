"""ctypes binding of libmemc_hip_ssim.so (include/memc_ssim.h): the HD demo loop's third score on the GPU -- the SSIM of two
8-bit planes (skimage's compare_ssim at its defaults), of byte planes as they are or of the luma planes of two RGB frames.

The library is loaded on first use, not at import.  A call without it raises RuntimeError: there is no fallback to the
numpy rule of networks/yuv_io.py for a missing library (that path is chosen by its caller, never silently).

The C functions take plain pointers and ints; the functions here take torch CUDA tensors, check what the C side cannot see
(dtype, device, strides, sizes) and hand over data_ptr() and the numbers.  Return value: the C function's int -- 0
enqueued, -1 a failed check.  Work is enqueued on the current HIP stream of the tensors' device; nothing synchronises.
"""
import ctypes

import torch

from .._satellite import Library, call as _call, check

_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
_LIB = Library("libmemc_hip_ssim.so", "memc_ssim_version", "the GPU SSIM has no fallback",
               [("memc_ssim_workspace_bytes", ctypes.c_size_t, [_I, _I, _I]),
                ("memc_ssim_u8", _I, [_P, _P, _P, _L, _L, _I, _I, _I, _P, _P, ctypes.c_size_t]),
                ("memc_ssim_luma_rgb", _I, [_P, _P, _P, _I, _I, _I, _P, _P, ctypes.c_size_t])])
LIB_PATH, lib, version = _LIB.path, _LIB.lib, _LIB.version


def _check(t, name, dtype, numel=None, dev=None, contiguous=True):
    """a (contiguous) CUDA tensor of `dtype` (of `numel` elements, on `dev`)"""
    check(t, name, dtype, numel, dev, contiguous, "the SSIM kernels")


def ssim_workspace_bytes(frames, h, w):
    return int(lib().memc_ssim_workspace_bytes(frames, h, w))


def ssim_u8(a, b, ssim, workspace):
    """ssim: float64 [frames] receives, per frame, the SSIM of two uint8 [frames, h, w] views with a w-stride of 1 and the
    same frame and row strides (any padding between rows and frames, any base address); workspace: uint8, at least
    ssim_workspace_bytes(frames, h, w) bytes, 8-byte aligned."""
    _check(a, "a", torch.uint8, contiguous=False)
    dev = a.device
    _check(b, "b", torch.uint8, dev=dev, contiguous=False)
    if a.dim() != 3 or a.shape != b.shape:
        raise ValueError("a, b: expected two [frames, h, w] tensors of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    frames, h, w = a.shape
    strides = [tuple(t.stride()[0 if frames > 1 else 1:]) for t in (a, b)]
    if strides[0] != strides[1] or a.stride(2) != 1:
        raise TypeError("a, b: expected a w-stride of 1 and the same strides, got %s and %s" % (a.stride(), b.stride()))
    _check(ssim, "ssim", torch.float64, frames, dev)
    _check(workspace, "workspace", torch.uint8, None, dev)
    return _call(_LIB, dev, "memc_ssim_u8", a.data_ptr(), b.data_ptr(), a.stride(0), a.stride(1), frames, h, w, ssim.data_ptr(),
                 workspace.data_ptr(), workspace.numel())


def ssim_luma_rgb(rgb_a, rgb_b, frames, h, w, ssim, workspace):
    """ssim: float64 [frames] receives, per frame, the SSIM of the truncated 8-bit luma planes of two uint8
    [frames, h, w, 3]; workspace: uint8, at least ssim_workspace_bytes(frames, h, w) bytes, 8-byte aligned."""
    _check(rgb_a, "rgb_a", torch.uint8, frames * h * w * 3)
    dev = rgb_a.device
    _check(rgb_b, "rgb_b", torch.uint8, frames * h * w * 3, dev)
    _check(ssim, "ssim", torch.float64, frames, dev)
    _check(workspace, "workspace", torch.uint8, None, dev)
    return _call(_LIB, dev, "memc_ssim_luma_rgb", rgb_a.data_ptr(), rgb_b.data_ptr(), frames, h, w, ssim.data_ptr(),
                 workspace.data_ptr(), workspace.numel())


__all__ = ["LIB_PATH", "lib", "version", "ssim_workspace_bytes", "ssim_u8", "ssim_luma_rgb"]
