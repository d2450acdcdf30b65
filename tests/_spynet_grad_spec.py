"""tests/_spynet_grad_spec.py -- what the tests of the SPyNet level backward kernel (include/memc_spynet_grad.h) share: the
cases, the rule restated in numpy and the kernel's footprint arithmetic.  Builds on tests/_spynet_spec.py, which it imports
and does not change.

`level_grad(second, coarse, G, flags, dtype, up=None)` is the header's rule: per fine site the gradient (gux, guy) reaching
the upsampled flow -- G[6:8] plus kx' * sum_c G[3 + c] dWc/dpx, the corners, in-range tests and weights from `floor` as in
the forward -- and per coarse cell twice the adjoint of the x2 upsampling.  np.float64 is the reference of the GPU tests;
`up` may be another upsampled flow than the rule's own (the GPU tests evaluate it on the kernel's own `up`).

`footprint(i, n_in, H, align, i1=None)` restates the source's candidate range of fine indices for the coarse cells
[i, i1) (one cell by default), `box_bound(n_in, H, align)` its bound of a tile's staged box; TILE and BOX are the source's
kTile and kBox (tests/test_spynet_grad_spec.py holds them to its text).

Admissibility.  The derivative jumps where a position crosses an integer.  An fp32 position below 64 differs from its
float64 value by less than 2^-14 (x + f, * k, - 0.5 and k's own rounding: four roundings of half an ulp of 64 each,
1.5e-5, against 6.1e-5), so an ordinary case is admissible only if no site with a corner inside the image has px or py
within DELTA = 2^-14 of an integer.  `ordinary_case` draws the coarse flow from an rng keyed by (shape, flags, attempt) and
takes the first admissible attempt, at most 64.  The zero flow under align_sample = 1, the pan and the exact cases sit on
exact positions and need no such test.
"""
import numpy as np

import _spynet_spec as S

TILE = 16                                      # kTile of spynet_level_bwd.hip
BOX = 2 * TILE + 7                             # kBox
DELTA = 2.0 ** -14
ATTEMPTS = 64

# _spynet_spec.SHAPES, then what this kernel needs beyond them: h or w equal to 1 with a padded column or row, and a coarse
# grid of 18 x 35 cells -- two tiles of 16 down, three across -- with a padded row and a width that is no multiple of four
SHAPES = S.SHAPES + ((1, 2, 3), (1, 3, 2), (1, 37, 70))
FLAGS = S.FLAGS
EXACT_FLAGS = S.EXACT_FLAGS


def flows(flags):
    """the flows of the ordinary cases under `flags`"""
    return ("normal", "zero", "pan") if flags[1] else ("normal", "pan")


def site_grad(second, up, G, align_sample, dtype):
    """[B, 2, H, W]: (gux, guy) per fine site"""
    B, _C, H, W = second.shape
    s, g = second.astype(dtype), G.astype(dtype)
    ix, iy, inx, iny, _wgt = S.corners(up.astype(dtype), align_sample, dtype)
    px = S._position(np.arange(W)[None, None, :], up.astype(dtype)[:, 0], W, align_sample, dtype)
    py = S._position(np.arange(H)[None, :, None], up.astype(dtype)[:, 1], H, align_sample, dtype)
    fx0, fy0 = np.floor(px), np.floor(py)
    ax, ay, bx, by = px - fx0, py - fy0, (fx0 + dtype(1)) - px, (fy0 + dtype(1)) - py
    bidx = np.arange(B)[:, None, None]
    dx, dy = np.zeros((B, H, W), dtype), np.zeros((B, H, W), dtype)
    for c in range(3):
        v = {}
        for name, (cy, cx) in (("nw", (0, 0)), ("ne", (0, 1)), ("sw", (1, 0)), ("se", (1, 1))):
            inside = inx[cx] & iny[cy]
            v[name] = np.where(inside, s[bidx, c, np.clip(iy + cy, 0, H - 1), np.clip(ix + cx, 0, W - 1)], dtype(0))
        dx = dx + g[:, 3 + c] * (by * (v["ne"] - v["nw"]) + ay * (v["se"] - v["sw"]))
        dy = dy + g[:, 3 + c] * (bx * (v["sw"] - v["nw"]) + ax * (v["se"] - v["ne"]))
    kx = dtype(1) if align_sample else dtype(W) / dtype(W - 1)
    ky = dtype(1) if align_sample else dtype(H) / dtype(H - 1)
    return np.stack([g[:, 6] + kx * dx, g[:, 7] + ky * dy], axis=1)


def adjoint_matrix(n_in, N, align, dtype):
    """[N, n_in]: the weight of coarse index i at fine index y, a padded one repeating 2 n_in - 1"""
    i0, i1, l0, l1 = S.up_index(np.minimum(np.arange(N), 2 * n_in - 1), n_in, align, dtype)
    m = np.zeros((N, n_in), dtype)
    np.add.at(m, (np.arange(N), i0), l0)
    np.add.at(m, (np.arange(N), i1), l1)
    return m


def upsample_adjoint(gu, h, w, align_upsample, dtype):
    """[B, 2, h, w] = 2 * sum_y sum_x wy(y, i) wx(x, j) gu(y, x)"""
    H, W = gu.shape[2:]
    my, mx = adjoint_matrix(h, H, align_upsample, dtype), adjoint_matrix(w, W, align_upsample, dtype)
    return dtype(2) * np.einsum("yi,bcyx,xj->bcij", my, gu.astype(dtype), mx)


def level_grad(second, coarse, G, flags, dtype, up=None):
    """gradcoarse [B, 2, h, w] of the header's rule, evaluated in `dtype`"""
    H, W = second.shape[2:]
    h, w = coarse.shape[2:]
    if up is None:
        up = S.upsampled(coarse, H, W, flags[0], dtype)
    return upsample_adjoint(site_grad(second, up, G, flags[1], dtype), h, w, flags[0], dtype)


# ---- the footprint arithmetic of spynet_level_bwd.hip (level_footprint, level_box_bound) ----

def footprint(i, n_in, H, align, i1=None):
    """(lo, hi): the candidate range of fine indices (of H, H in {2 n_in, 2 n_in + 1}) for the coarse cells [i, i1); `i`
    and `i1` may be integer arrays"""
    i = np.asarray(i, np.int64)
    i1 = i + 1 if i1 is None else np.asarray(i1, np.int64)
    last = 2 * n_in - 1
    if not align:
        a, b = 2 * i - 1, 2 * i1
    elif n_in == 1:
        a, b = np.zeros_like(i), np.full_like(i1, last)
    else:
        num, den = 2 * n_in - 1, n_in - 1
        a = np.where(i >= 1, ((i - 1) * num) // den, 0)
        b = np.minimum((i1 * num + den - 1) // den, last)
    lo, hi = np.maximum(a, 0), np.where(b >= last, H - 1, b)
    return (int(lo), int(hi)) if lo.ndim == 0 else (lo, hi)


def box_bound(n_in, H, align):
    """an upper bound of hi - lo + 1 over every tile of TILE cells"""
    if n_in <= TILE:
        return H
    if not align:
        return 2 * TILE + 2
    return 2 * TILE + 4 + (TILE + 1 + n_in - 2) // (n_in - 1) + (H - 2 * n_in)


# ---- cases ----

def gradoutput(shape, key="ordinary"):
    """G [B, 8, H, W] = N(0, 1) / 4, seeded"""
    B, H, W = shape
    return (S._rng("gradoutput", key, shape).standard_normal((B, 8, H, W)) / 4.0).astype(np.float32)


def admissible(up, align_sample, delta=DELTA):
    """no site with a corner inside the image has px or py within `delta` of an integer (float64 positions of `up`)"""
    _B, _two, H, W = up.shape
    up = up.astype(np.float64)
    _ix, _iy, inx, iny, _w = S.corners(up, align_sample, np.float64)
    inside = (inx[0] | inx[1]) & (iny[0] | iny[1])
    px = S._position(np.arange(W)[None, None, :], up[:, 0], W, align_sample, np.float64)
    py = S._position(np.arange(H)[None, :, None], up[:, 1], H, align_sample, np.float64)
    near = (np.abs(px - np.rint(px)) < delta) | (np.abs(py - np.rint(py)) < delta)
    return not bool((inside & near).any())


_CASES = {}


def ordinary_case(shape, flags, flow="normal"):
    """(second, coarse, G) in float32 and the attempt taken: `second` of _spynet_spec.ordinary_case; the coarse flow
    N(0, 4^2) by the first admissible attempt, zero (align_sample = 1 only) or the 1e9 pan; G = N(0, 1) / 4"""
    key = (shape, tuple(flags), flow)
    if key not in _CASES:
        B, H, W = shape
        second = S.ordinary_case(shape)[1]
        G = gradoutput(shape)
        if flow == "normal":
            for attempt in range(ATTEMPTS):
                coarse = (4.0 * S._rng("coarse", shape, tuple(flags), attempt).standard_normal((B, 2, H // 2, W // 2))).astype(
                    np.float32)
                if admissible(S.upsampled(coarse, H, W, flags[0], np.float32), flags[1]):
                    break
            else:
                raise AssertionError("no admissible draw in %d attempts: %s %s" % (ATTEMPTS, shape, flags))
        else:
            assert flow == "pan" or (flow == "zero" and flags[1]), (flow, flags)
            coarse, attempt = S.ordinary_case(shape, flow)[2], None
        for a in (second, coarse, G):
            a.setflags(write=False)
        _CASES[key] = (second, coarse, G, attempt)
    return _CASES[key]


def exact_case(shape):
    """(second, coarse, G): _spynet_spec.exact_case's frames and integer flows, integer G in [-4, 4]"""
    key = ("exact", shape)
    if key not in _CASES:
        B, H, W = shape
        _first, second, coarse = S.exact_case(shape)
        G = S._rng("gradoutput", "exact", shape).integers(-4, 5, (B, 8, H, W)).astype(np.float32)
        for a in (second, coarse, G):
            a.setflags(write=False)
        _CASES[key] = (second, coarse, G)
    return _CASES[key]
