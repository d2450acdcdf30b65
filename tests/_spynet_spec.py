"""tests/_spynet_spec.py -- what the tests of the SPyNet pyramid-level kernel (include/memc_spynet.h) share: the cases, and
the kernel's arithmetic restated in numpy.

`level(first, second, coarse, align_upsample, align_sample, dtype)` is ONE statement of the rule in the kernel's order,
evaluated in `dtype`:

    np.float32   the restatement of the kernel's arithmetic (every operation rounded on its own: numpy does not contract
                 a product and a sum, the compiler may -- which is invisible wherever every product is exact)
    np.float64   the direct formula with the same index rules: the reference value of the GPU tests

    up:      ATen's area_pixel_compute_source_index per axis (scale 0.5, or (h - 1) / (2h - 1) under align_upsample, of the
             unpadded size; destination index min(y, 2h - 1): a padded row or column repeats the last one);
             up = 2 * (ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d))
    sample:  px = x + up_x (align_sample) or (x + up_x) * W / (W - 1) - 0.5, clamped into [-2, W + 1] by comparisons that
             send a NaN to -2; corners floor(px), floor(px) + 1 with the weights (floor(px) + 1) - px and px - floor(px);
             out = nw + ne + sw + se, a corner outside the image contributing nothing.

That the direct position is the same function as torch's normalise / grid_sample route is shown in
tests/test_spynet_level_spec.py, not assumed.
"""
import zlib

import numpy as np

# (B, H, W) of the GPU tests: the quad kernel; the quad kernel with a padded row; the direct kernel; a padded row and
# column; the smallest quad width; a width below 8
SHAPES = ((2, 24, 40), (2, 25, 40), (2, 26, 42), (1, 33, 49), (1, 8, 8), (1, 6, 5))
FLAGS = ((0, 0), (1, 1), (0, 1))               # (align_upsample, align_sample)
EXACT_FLAGS = (0, 1)


def family(W):
    """the kernel family that serves a contiguous call of width W"""
    return "spynet_level:quad" if W % 4 == 0 and W >= 8 else "spynet_level:direct"


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def ordinary_case(shape, flow="normal"):
    """(first, second, coarse) in float32: images (U[0, 1) - 0.45) / 0.225, as preprocessed frames are; the coarse flow
    N(0, 4^2), zero, or a pan of 1e9 in x"""
    B, H, W = shape
    rng = _rng("ordinary", shape)
    first = ((rng.random((B, 3, H, W)) - 0.45) / 0.225).astype(np.float32)
    second = ((rng.random((B, 3, H, W)) - 0.45) / 0.225).astype(np.float32)
    coarse = (4.0 * rng.standard_normal((B, 2, H // 2, W // 2))).astype(np.float32)
    if flow == "zero":
        coarse[:] = 0.0
    elif flow == "pan":
        coarse[:, 0] = 1e9
        coarse[:, 1] = 0.0
    else:
        assert flow == "normal"
    return first, second, coarse


def exact_case(shape):
    """inputs on which every product and partial sum of the rule is an fp32 number under EXACT_FLAGS: pixels k / 16 with
    |k| <= 48, integer coarse flows with |f| <= 6 -- so `up` is a multiple of 1/8, every weight a multiple of 1/8"""
    B, H, W = shape
    rng = _rng("exact", shape)
    first = (rng.integers(-48, 49, (B, 3, H, W)) / 16.0).astype(np.float32)
    second = (rng.integers(-48, 49, (B, 3, H, W)) / 16.0).astype(np.float32)
    coarse = rng.integers(-6, 7, (B, 2, H // 2, W // 2)).astype(np.float32)
    return first, second, coarse


def up_index(dst, n_in, align, dtype):
    """area_pixel_compute_source_index for the destination indices `dst` (already clamped to the unpadded size 2 * n_in)"""
    d = dst.astype(dtype)
    if align:
        scale = dtype(n_in - 1) / dtype(2 * n_in - 1) if n_in > 1 else dtype(0)
        src = scale * d
    else:
        src = np.maximum(dtype(0.5) * (d + dtype(0.5)) - dtype(0.5), dtype(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(dtype)
    return i0, i1, dtype(1) - l1, l1


def upsampled(coarse, H, W, align_upsample, dtype):
    """up [B, 2, H, W] = 2 * bilinear_x2(coarse), a padded row / column repeating the last"""
    h, w = coarse.shape[2:]
    assert H in (2 * h, 2 * h + 1) and W in (2 * w, 2 * w + 1)
    c = coarse.astype(dtype)
    y0, y1, ly0, ly1 = up_index(np.minimum(np.arange(H), 2 * h - 1), h, align_upsample, dtype)
    x0, x1, lx0, lx1 = up_index(np.minimum(np.arange(W), 2 * w - 1), w, align_upsample, dtype)
    a, b = c[:, :, y0][:, :, :, x0], c[:, :, y0][:, :, :, x1]
    cc, d = c[:, :, y1][:, :, :, x0], c[:, :, y1][:, :, :, x1]
    ly0, ly1 = ly0[:, None], ly1[:, None]
    return dtype(2) * (ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * cc + lx1 * d))


def _position(idx, f, n, align_sample, dtype):
    p = idx.astype(dtype) + f
    if not align_sample:
        p = p * (dtype(n) / dtype(n - 1)) - dtype(0.5)
    with np.errstate(invalid="ignore"):
        p = np.where(p > dtype(-2), p, dtype(-2))
        p = np.where(p < dtype(n + 1), p, dtype(n + 1))
    return p.astype(dtype)


def corners(up, align_sample, dtype):
    """per site: the corner indices and their in-range tests along both axes, and the four weights"""
    _B, _two, H, W = up.shape
    px = _position(np.arange(W)[None, None, :], up[:, 0], W, align_sample, dtype)
    py = _position(np.arange(H)[None, :, None], up[:, 1], H, align_sample, dtype)
    fx0, fy0 = np.floor(px), np.floor(py)
    ix, iy = fx0.astype(np.int64), fy0.astype(np.int64)
    ax, ay, bx, by = px - fx0, py - fy0, (fx0 + dtype(1)) - px, (fy0 + dtype(1)) - py
    inx = (ix >= 0) & (ix < W), (ix + 1 >= 0) & (ix + 1 < W)
    iny = (iy >= 0) & (iy < H), (iy + 1 >= 0) & (iy + 1 < H)
    return ix, iy, inx, iny, (bx * by, ax * by, bx * ay, ax * ay)


def warp(second, up, align_sample, dtype):
    """second [B, 3, H, W] sampled at (x, y) + up, zero padding, in the order nw, ne, sw, se"""
    B, C, H, W = second.shape
    s = second.astype(dtype)
    ix, iy, inx, iny, weights = corners(up.astype(dtype), align_sample, dtype)
    bidx = np.arange(B)[:, None, None]
    out = np.zeros((B, C, H, W), dtype)
    for (dy, dx), wgt in zip(((0, 0), (0, 1), (1, 0), (1, 1)), weights):
        inside = inx[dx] & iny[dy]
        cx, cy = np.clip(ix + dx, 0, W - 1), np.clip(iy + dy, 0, H - 1)
        for ch in range(C):
            out[:, ch] = out[:, ch] + np.where(inside, s[bidx, ch, cy, cx] * wgt, dtype(0))
    return out


def level(first, second, coarse, align_upsample, align_sample, dtype, up=None):
    """[B, 8, H, W]: first | second warped by `up` | up.  `up`: another upsampled flow than this rule's own (the GPU tests
    hold the kernel's warp to the direct formula evaluated on the kernel's own `up`)."""
    H, W = first.shape[2:]
    if up is None:
        up = upsampled(coarse, H, W, align_upsample, dtype)
    up = up.astype(dtype)
    return np.concatenate([first.astype(dtype), warp(second, up, align_sample, dtype), up], axis=1)


def census(coarse, H, W, align_upsample, align_sample):
    """how many sites have 0, 1, 2 or 4 corners inside the image (float64 positions), how many sit in the padded row or
    column, and the kernel family that serves the case"""
    h, w = coarse.shape[2:]
    up = upsampled(coarse, H, W, align_upsample, np.float64)
    _ix, _iy, inx, iny, _w = corners(up, align_sample, np.float64)
    n = sum((inx[dx] & iny[dy]).astype(np.int64) for dy in (0, 1) for dx in (0, 1))
    out = {"corners_%d" % k: int((n == k).sum()) for k in (0, 1, 2, 3, 4)}
    B = coarse.shape[0]
    out["sites"] = int(n.size)
    out["padded"] = B * ((H - 2 * h) * W + (W - 2 * w) * H - (H - 2 * h) * (W - 2 * w))
    out["family"] = family(W)
    return out


def check_level(got, case, flags, what, exact=False):
    """The operator rule of the GPU tests for one [B, 8, H, W] result `got` (numpy float32) on `case`:
    got[:, 0:3] equals `first`; got[:, 6:8] is held to torch's float64 expression; got[:, 3:6] is held to the float64
    direct formula evaluated on got's OWN `up` -- by tests/_parity.close, or bit for bit on an exact case.  Returns the two
    worst errors."""
    import torch
    import _parity
    from my_package.functions.SpyNetLevelLayer import _composed
    first, second, coarse = case
    assert got.dtype == np.float32 and got.shape == (first.shape[0], 8) + first.shape[2:], (got.dtype, got.shape)
    assert np.array_equal(got[:, 0:3], first), what + ": first"
    want_up = _composed(*(torch.from_numpy(a).double() for a in case), bool(flags[0]), bool(flags[1]))[:, 6:8].numpy()
    want_warp = level(first, second, coarse, flags[0], flags[1], np.float64, up=got[:, 6:8])[:, 3:6]
    if exact:
        assert np.array_equal(got[:, 6:8].astype(np.float64), want_up), what + ": up, bit for bit"
        assert np.array_equal(got[:, 3:6].astype(np.float64), want_warp), what + ": warp, bit for bit"
        return 0.0, 0.0
    return (_parity.close(got[:, 6:8].astype(np.float64), want_up, what + ": up vs torch float64"),
            _parity.close(got[:, 3:6].astype(np.float64), want_warp, what + ": warp vs float64 direct formula on its own up"))
