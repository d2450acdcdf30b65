"""Frame-pair inference the way the reference demos run it (the part with a bearing on the
hot path): replicate-pad both frames so that H and W are multiples of 128 -- or by 32 on each side when they
already are -- run the network, crop the padding off (demo_HD720p.py:88-113,138-146; demo_MiddleBury.py:74-110).
The HD demo's YUV 4:2:0 reader / writer and its per-pair loop are in yuv_io.py (numpy only); the still-image demo's
files are read and written by png_io.py (zlib + numpy): 8-bit grey, grey + alpha, RGB, RGBA and palette PNGs, all five
scanline filters, CRC-checked -- no tRNS chunk (palette transparency is ignored), no 16-bit samples, no interlacing
(both rejected with an error).
"""
import torch
import torch.nn.functional as F


def pad_amounts(height, width):
    """(left, right, top, bottom) of the reference rule, demo_HD720p.py:88-106."""
    def one(n):
        if n != ((n >> 7) << 7):
            total = (((n >> 7) + 1) << 7) - n
            first = int(total / 2)
            return first, total - first
        return 32, 32
    left, right = one(width)
    top, bottom = one(height)
    return left, right, top, bottom


HALF_DTYPES = (torch.float16, torch.bfloat16)


def check_precision(dtype, autocast):
    """The demo loops' two precision arguments: dtype is None, torch.float32 (both: float32 planes, as without it) or a half
    dtype (the planes handed to the model have it; the caller has cast the model); autocast is None or a half dtype (the
    model call runs inside torch.autocast on float32 planes).  Any other dtype for either: TypeError; a half dtype together
    with autocast: ValueError.  Returns the half dtype of the planes, or None for float32 planes."""
    if dtype is not None and dtype != torch.float32 and dtype not in HALF_DTYPES:
        raise TypeError("dtype: expected None, torch.float32, torch.float16 or torch.bfloat16, got %r" % (dtype,))
    if autocast is not None and autocast not in HALF_DTYPES:
        raise TypeError("autocast: expected None, torch.float16 or torch.bfloat16, got %r" % (autocast,))
    if dtype in HALF_DTYPES and autocast is not None:
        raise ValueError("dtype=%s (a cast model) and autocast=%s (a float32 model) exclude each other" % (dtype, autocast))
    return dtype if dtype in HALF_DTYPES else None


def run_model(model, x, autocast=None):
    """model(x) without gradients, inside torch.autocast(dtype=autocast) where that is asked for; x: a tensor, or a list of
    tensors on one device (MEMC_Net_VE's seven frames)"""
    with torch.no_grad():
        if autocast is None:
            return model(x)
        first = x[0] if isinstance(x, (list, tuple)) else x
        with torch.autocast(first.device.type, dtype=autocast):
            return model(x)


def interpolate_pairs(model, frame0, frame2, which=1, dtype=None, autocast=None):
    """frame0, frame2: [B, 3, H, W] in [0, 1].  Returns the interpolated middle frames [B, 3, H, W]
    (which = 1: the rectified output, 0: the blended one -- the demos' `save_which`), padding removed.
    dtype=torch.float16 / torch.bfloat16: the frames are cast to it and padded in it (for a model cast with model.to(dtype));
    autocast=torch.float16 / torch.bfloat16: the model runs inside torch.autocast on the frames as they are (check_precision
    has the rules).  Either way the result is what the model returns, cropped: its dtype is the model's, not widened here."""
    half = check_precision(dtype, autocast)
    assert frame0.shape == frame2.shape and frame0.dim() == 4
    h, w = frame0.shape[2], frame0.shape[3]
    left, right, top, bottom = pad_amounts(h, w)
    if half is not None:
        frame0, frame2 = frame0.to(half), frame2.to(half)
    x = torch.stack([F.pad(f, (left, right, top, bottom), mode="replicate") for f in (frame0, frame2)])
    frames, _flows, _filters, _occlusions = run_model(model, x, autocast)
    return frames[which][:, :, top:top + h, left:left + w]
