"""ctypes binding of libmemc_hip_ssim.so (include/memc_ssim.h): the HD demo loop's third score on the GPU -- the SSIM of two
8-bit planes (skimage's compare_ssim at its defaults), of byte planes as they are or of the luma planes of two RGB frames.

The library is loaded on first use, not at import.  A call without it raises RuntimeError: there is no fallback to the
numpy rule of networks/yuv_io.py for a missing library (that path is chosen by its caller, never silently).

The C functions take plain pointers and ints; the functions here take torch CUDA tensors, check what the C side cannot see
(dtype, device, strides, sizes) and hand over data_ptr() and the numbers.  Return value: the C function's int -- 0
enqueued, -1 a failed check.  Work is enqueued on the current HIP stream of the tensors' device; nothing synchronises.
"""
import ctypes
import os
import threading

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libmemc_hip_ssim.so")
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
                        "libmemc_hip_ssim.so not found at %s -- build it with `make -C %s` (or `python -c 'import "
                        "__graft_entry__ as g; g.build()'` at the repo root); the GPU SSIM has no fallback"
                        % (LIB_PATH, os.path.join(_PKG_ROOT, "csrc")))
                L = ctypes.CDLL(LIB_PATH)
                L.memc_ssim_version.restype = ctypes.c_char_p
                L.memc_ssim_version.argtypes = []
                L.memc_ssim_workspace_bytes.restype = ctypes.c_size_t
                L.memc_ssim_workspace_bytes.argtypes = [_I, _I, _I]
                L.memc_ssim_u8.restype = ctypes.c_int
                L.memc_ssim_u8.argtypes = [_P, _P, _P, _L, _L, _I, _I, _I, _P, _P, ctypes.c_size_t]
                L.memc_ssim_luma_rgb.restype = ctypes.c_int
                L.memc_ssim_luma_rgb.argtypes = [_P, _P, _P, _I, _I, _I, _P, _P, ctypes.c_size_t]
                _lib = L
    return _lib


def version():
    return lib().memc_ssim_version().decode()


def _check(t, name, dtype, numel=None, dev=None, contiguous=True):
    """a (contiguous) CUDA tensor of `dtype` (of `numel` elements, on `dev`)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: expected a torch.Tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise TypeError("%s: expected a CUDA (HIP) tensor; the SSIM kernels have no CPU path" % name)
    if t.dtype != dtype:
        raise TypeError("%s: expected %s, got %s" % (name, dtype, t.dtype))
    if contiguous and not t.is_contiguous():
        raise TypeError("%s: expected a contiguous tensor" % name)
    if numel is not None and t.numel() != numel:
        raise ValueError("%s: expected %d elements, got %d" % (name, numel, t.numel()))
    if dev is not None and t.device != dev:
        raise TypeError("%s: all tensors must live on the same device" % name)


def _call(dev, name, *args):
    with torch.cuda.device(dev):
        return int(getattr(lib(), name)(torch.cuda.current_stream(dev).cuda_stream, *args))


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
    return _call(dev, "memc_ssim_u8", a.data_ptr(), b.data_ptr(), a.stride(0), a.stride(1), frames, h, w, ssim.data_ptr(),
                 workspace.data_ptr(), workspace.numel())


def ssim_luma_rgb(rgb_a, rgb_b, frames, h, w, ssim, workspace):
    """ssim: float64 [frames] receives, per frame, the SSIM of the truncated 8-bit luma planes of two uint8
    [frames, h, w, 3]; workspace: uint8, at least ssim_workspace_bytes(frames, h, w) bytes, 8-byte aligned."""
    _check(rgb_a, "rgb_a", torch.uint8, frames * h * w * 3)
    dev = rgb_a.device
    _check(rgb_b, "rgb_b", torch.uint8, frames * h * w * 3, dev)
    _check(ssim, "ssim", torch.float64, frames, dev)
    _check(workspace, "workspace", torch.uint8, None, dev)
    return _call(dev, "memc_ssim_luma_rgb", rgb_a.data_ptr(), rgb_b.data_ptr(), frames, h, w, ssim.data_ptr(),
                 workspace.data_ptr(), workspace.numel())


__all__ = ["LIB_PATH", "lib", "version", "ssim_workspace_bytes", "ssim_u8", "ssim_luma_rgb"]
