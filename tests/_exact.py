"""tests/_exact.py -- inputs on which the warps, the projection sums, the projection backward and the x4 upsampling are exact in
fp32, whatever the order of the sums.

The grid
    image        k / 16,  k = 0 .. 15            (2^-4)
    taps         k / 8,   k = 0 .. 7             (2^-3)
    occlusion    k / 8,   k = -8 .. 8            (2^-3; a block of zeros and a block of negative values, as np_occlusion)
    depth        k / 8,   k = 1 .. 9             (2^-3); signed_depth: k = -9 .. 9 (the projection forward with hole filling)
    gradoutput   integers in [-G, G], G = 8
    context      k / 16,  k = 0 .. 15            (the features warped beside the frame: the image's grid)
    flow         round(4 f) / 4 of an existing generator's flow f (2^-2): a quarter of the sites per axis sit on integer
                 coordinates, so alpha and beta are 0, 1/4, 1/2 or 3/4 and a bilinear weight (1 - alpha)(1 - beta) is a
                 multiple of 2^-4.  Stored in bf16 the flow is clipped to +-63.75, in fp16 to +-511.75 (the largest
                 magnitudes those formats hold on the quarter grid); stored in fp32 it is not clipped.
Every value is a number of fp16 and of bf16.  Image, taps and gradoutput come from a generator seeded apart from the
flow's (seed + 1000), so that the flow is the very field tests/_lowp_paths.py counts.

The quantum of each result (the power of two every term and every partial sum is a multiple of)
    adaptive warp (FilterInterpolation), out = sum_taps tap * (bilinear mix of four pixels)
        forward          pixel 2^-4 * tap 2^-3 * weight 2^-4                        = 2^-11
        blend forward    the above times an occlusion 2^-3                          = 2^-14
        image gradient   gradoutput 1 * tap 2^-3 * weight 2^-4                      = 2^-7
        tap gradient     gradoutput 1 * pixel 2^-4 * weight 2^-4                    = 2^-8
        flow gradient    gradoutput 1 * tap 2^-3 * pixel 2^-4 * (1 - alpha) 2^-2    = 2^-9
      the blend's backward works on gradoutput * occlusion (2^-3):
        tap gradient 2^-11, flow gradient 2^-12; occlusion gradient = sum_c gradoutput * forward = 2^-11
    bilinear warp (Interpolation, InterpolationCh)
        forward 2^-4 * 2^-4 = 2^-8, image gradient 1 * 2^-4 = 2^-4, flow gradient 1 * 2^-4 * 2^-2 = 2^-6
    projection sums
        flow 2^-2; with a depth 2^-3 * 2^-2 = 2^-5; counts: integers, or multiples of 2^-3 with a depth.  Exact sums make
        the SIGN of every count certain (signed depths: negative, or exactly zero over a non-zero flow sum), so which
        cell is a hole, where its walks stop and which stops contribute is the same for every correct implementation:
        fill_expectation restates the reference's fill in float64, fill_sensitivity says what a walk one cell off would move
    projection backward, gradinput1 = -sum_corners gradoutput / count (* depth),
                         gradinput2 = -sum_corners gradoutput / count * (flow - forward output)
        The operators' ABI takes count (and the forward's output) as INPUTS.  The premise of these cases: both are
        SYNTHETIC -- count is +-2^e exactly where the true scatter puts anything (e = 0 .. 4; with a depth -2 .. 4 and a
        random sign, as real depth counts can be negative) and exactly 0 elsewhere; the forward output is k / 4 in
        [-64, 64].  Every quotient is then exact: gradoutput / count 2^-4; gradinput1 2^-4, with a depth 2^-7; gradinput2
        2^-4 * 2^-2 = 2^-6.  A count of 0 is staged as 1 / 0 = inf by the tiled kernel: a read of it by any site
        comes out as inf or NaN.  Real counts (sums of depths, any value) stay under the 1e-4 tests of
        tests/test_gpu_parity.py, which remain as they are.
    x4 upsampling of (mul * flow) / div, flow k / 4 in [-64, 64], (mul, div) = (20, 2) or (6, 3)
        the scaled flow 2^-1 (exact whether divided or multiplied by the reciprocal); without align_corners the weights
        are k / 8 per axis: 2^-1 * 2^-6 = 2^-7

Why order cannot matter.  A sum of multiples of 2^-q whose absolute values add up to M has every partial sum, in any
order and under any grouping, a multiple of 2^-q below M in magnitude: where M * 2^q < 2^24 each of them is a number
of fp32 and no addition rounds.  A fused multiply-add rounds once where a multiply and an add round twice: where neither
rounds the two agree.  The packed fixed-point planes, the LDS atomics, the global atomics and the oracle's sequential
loop therefore all return the same bits.  budget() gives M per output; tests/test_exact_inputs.py asserts
M * 2^q < 2^24 for every case the GPU module runs and shows with a float64 build of the oracle that nothing rounded.

What such inputs cannot see: a difference in rounding ORDER (a contraction, another association).  The bit-equality
tests between the libraries stay for that.
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd"), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _lowp_paths as LP      # noqa: E402
from tools import synth       # noqa: E402

G = 8                         # |gradoutput| <= G

# log2 of one over the quantum, per output
Q = dict(fi_fwd=11, blend_fwd=14, fi_image=7, fi_taps=8, fi_flow=9, blend_taps=11, blend_flow=12, blend_occ=11,
         bl_fwd=8, bl_image=4, bl_flow=6, proj=2, dproj=5,
         pb_quot=4, pb_g1=4, dpb_g1=7, dpb_g2=6)
LIMIT = 2.0 ** 24

CLIP = {"fp32": None, "fp16": 511.75, "bf16": 63.75}

# the two cases test_gpu_blend_grad.py adds to the census table (the minimum width; a wide row of mostly invalid sites)
EXTRA = [(2, 37, 8, "smooth", 4.0, 31), (1, 20, 1280, "iid", 0.6 * 1280, 32)]
# one case of this module's own: Gaussian flows all but never sit exactly on an edge of the validity test, and no case above
# has five sites on every one of them at once (|fx| == W / 2 needs a narrow image, the valid border sites a gentler flow
# than 1x40x40-iid30's).  Four 40 x 40 images under an i.i.d. flow of sigma 14: 11 or more sites on each of the six edges.
EDGES = (4, 40, 40, "iid", 14.0, 61)
TABLE = LP.CASES + EXTRA + [EDGES]
TABLE_IDS = LP.CASE_IDS + ["2x37x8-min-width", "1x20x1280-far", "4x40x40-edges"]
FAR = EXTRA[1]                # keeps its slow and capped sites only unclipped: flow stored in fp32 only


def quantise_flow(f, storage="fp32"):
    """round(4 f) / 4, clipped to what `storage` holds on the quarter grid"""
    q = np.round(np.asarray(f, dtype=np.float64) * 4.0) / 4.0
    if CLIP[storage] is not None:
        q = np.clip(q, -CLIP[storage], CLIP[storage])
    return np.ascontiguousarray(q, dtype=np.float32)


def payload(seed, B, C, H, W, taps=16, g=G):
    """(image, taps, gradoutput) on the grid, from a generator of its own"""
    rng = np.random.default_rng(seed + 1000)
    x = (rng.integers(0, 16, (B, C, H, W)) / 16.0).astype(np.float32)
    filt = (rng.integers(0, 8, (B, taps, H, W)) / 8.0).astype(np.float32)
    gout = rng.integers(-g, g + 1, (B, C, H, W)).astype(np.float32)
    return x, filt, gout


def occlusion(seed, B, H, W):
    """k / 8 in [0, 1] with np_occlusion's block of zeros and block of negative values"""
    rng = np.random.default_rng(seed + 2000)
    o = (rng.integers(0, 9, (B, 1, H, W)) / 8.0).astype(np.float32)
    o[:, :, H // 4:H // 2, W // 4:W // 2] = 0.0
    o[:, :, H // 2:3 * H // 4, W // 2:3 * W // 4] *= -1.0
    return o


def depth(seed, B, H, W):
    rng = np.random.default_rng(seed + 3000)
    return (rng.integers(1, 10, (B, 1, H, W)) / 8.0).astype(np.float32)


_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def table_flow(case, storage="fp32", second=False):
    return quantise_flow(LP.case_flow(case, second), storage)


def table_inputs(case, C=3, storage="fp32"):
    """(image, flow, taps, gradoutput) of a table case; never written"""
    def make():
        B, H, W, _kind, _sigma, seed = case
        x, filt, gout = payload(seed, B, C, H, W)
        return x, table_flow(case, storage), filt, gout
    return _once(("table", case, C, storage), make)


def blend_inputs(case, storage="fp32"):
    """dict x0, x2, f0, f1, k0, k1, o0, o1, gout of a table case: the second direction's flow is _lowp_paths' (seed + 100)"""
    def make():
        B, H, W, _kind, _sigma, seed = case
        x0, k0, gout = payload(seed, B, 3, H, W)
        x2, k1, _ = payload(seed + 100, B, 3, H, W)
        return dict(x0=x0, x2=x2, f0=table_flow(case, storage), f1=table_flow(case, storage, True), k0=k0, k1=k1,
                    o0=occlusion(seed, B, H, W), o1=occlusion(seed + 100, B, H, W), gout=gout)
    return _once(("blend", case, storage), make)


def shaped_inputs(B, C, H, W, kind, sigma, seed, taps=16):
    """a case given by its shape (test_gpu_parity.py's tables): the flow is the first draw from default_rng(seed)"""
    def make():
        f = synth.np_flow(np.random.default_rng(seed), B, H, W, kind, sigma)
        x, filt, gout = payload(seed, B, C, H, W, taps)
        return x, quantise_flow(f), filt, gout
    return _once(("shape", B, C, H, W, kind, sigma, seed, taps), make)


def many_inputs(row):
    """a row (B, C, H, W, kind) of test_gpu_parity.MANY, quantised; the flow as test_filter_interpolation_backward_many_channels draws it"""
    def make():
        import test_gpu_parity as FP32
        B, C, H, W, kind = row
        rng = np.random.default_rng(sum(row[:4]))
        synth.np_image(rng, B, C, H, W), synth.np_filter(rng, B, H, W), synth.np_image(rng, B, C, H, W)    # (its draws before the flow)
        f = FP32._many_channel_flows(kind, rng, B, H, W)
        x, filt, gout = payload(sum(row[:4]), B, C, H, W)
        return x, quantise_flow(f), filt, gout
    return _once(("many", row), make)


# ------------------------------------------------------------------------------------------------------------------
# projection
# ------------------------------------------------------------------------------------------------------------------
def project_sums(flow, dep=None):
    """the scatter of oracle/memc_oracle.c project_scatter in float64, before the division: (s [B, 2, H, W], c [B, 1, H, W])"""
    B, _, H, W = flow.shape
    s, c = np.zeros((B, 2, H, W), np.float64), np.zeros((B, 1, H, W), np.float64)
    fx, fy = flow[:, 0].astype(np.float32), flow[:, 1].astype(np.float32)
    x2 = np.arange(W, dtype=np.float32)[None, None, :] + fx
    y2 = np.arange(H, dtype=np.float32)[None, :, None] + fy
    ok = (x2 >= 0) & (y2 >= 0) & (x2 <= np.float32(W - 1)) & (y2 <= np.float32(H - 1))
    b, y, x = np.nonzero(ok)
    L, T = x2[ok].astype(np.int64), y2[ok].astype(np.int64)
    R, Bm = np.minimum(L + 1, W - 1), np.minimum(T + 1, H - 1)
    d = np.ones(len(b)) if dep is None else dep[:, 0][ok].astype(np.float64)
    vx, vy = -d * fx[ok].astype(np.float64), -d * fy[ok].astype(np.float64)
    for yy, xx in ((T, L), (T, R), (Bm, L), (Bm, R)):           # (R == L or Bm == T: the same cell twice, as the reference)
        np.add.at(s[:, 0], (b, yy, xx), vx)
        np.add.at(s[:, 1], (b, yy, xx), vy)
        np.add.at(c[:, 0], (b, yy, xx), d)
    return s, c


def projection_inputs(name):
    """(flow, depth) by name: rows 0, 5, 8 of test_gpu_parity.CASES, two pans and a few far sources, all on the grid and
    no larger than 200 x 320"""
    def make():
        if name.startswith("row"):
            import test_gpu_parity as FP32
            B, _C, H, W, kind, sigma, seed = FP32.CASES[int(name[3:])]
            f = synth.np_flow(np.random.default_rng(seed), B, H, W, kind, sigma)
        elif name.startswith("pan"):
            px, py, sigma = {"pan216": (216.0, 0.0, 1.0), "pan-300": (-300.0, 0.0, 1.5)}[name]
            B, H, W = 1, 200, 320
            f = synth.np_flow(np.random.default_rng(int(abs(px) * 7 + abs(py) * 13 + sigma)), B, H, W, "smooth", sigma)
            f[0, 0] += px
            f[0, 1] += py
            f[0, :, 50:70, 100:140] = 0.0                            # a static patch: far from the pan
            f[0, 0, 120:130, 280:300] -= 60.0                        # a fast object
        elif name == "far":                                          # test_projection_with_a_few_far_sources' image 0, smaller
            B, H, W = 1, 170, 320
            f = synth.np_flow(np.random.default_rng(4711), B, H, W, "smooth", 4.0)
            f[0, :, 60:70, 200:230] = 300.0                          # a hole (its sources leave the image) ...
            for (y, x, fx, fy) in ((5, 7, 150.0, 0.0), (100, 300, -200.5, 40.25), (160, 20, 30.0, -100.0), (64, 210, 0.0, 25.0),
                                   (40, 180, 35.5, 24.75), (90, 100, -24.0, 3.0), (12, 250, 23.75, -23.75)):
                f[0, 0, y, x], f[0, 1, y, x] = fx, fy                # ... that (40, 180) -> (215.5, 64.75) lands in
        elif name in PROJECTION_FILL:
            f = _fill_case(name)[0]
        else:
            raise ValueError(name)
        B, _, H, W = f.shape
        return quantise_flow(f), depth(len(name), B, H, W)          # (any seed: the depths are k / 8 whatever it is)
    return _once(("proj", name), make)


PROJECTION = ["row0", "row5", "row8", "pan216", "pan-300", "far"]
# hole filling: a hole over several 64 x 32 tiles beside an image nothing lands in; walks over 12 tile columns and over 9
# tile rows (the pending filler's rounds of eight neighbours make a second trip); a ragged width with holes in every tile;
# a width below 8 (the one-lane-per-site kernels and proj_fillhole); the shape of test_projection_forward_unusual_depths_and_flows
PROJECTION_FILL = ["2x70x134-patch-empty", "1x12x1280-long-rows", "1x600x8-long-columns", "1x40x70-iid6", "2x9x7-iid2",
                   "2x45x132-signed"]
PROJECTION_ALL = PROJECTION + PROJECTION_FILL
PROJECTION_SIGNED = ["2x70x134-patch-empty", "2x45x132-signed", "1x40x70-iid6", "2x9x7-iid2"]     # run with signed_depth too
PROJECTION_SENSITIVE = ["far", "2x70x134-patch-empty", "1x12x1280-long-rows"]                        # sensitivity >= 0.9
PROJECTION_OPS = [(n, op) for n in PROJECTION_ALL for op in ("flow", "depth") + (("signed",) if n in PROJECTION_SIGNED else ())]
PROJECTION_OP_IDS = ["%s-%s" % k for k in PROJECTION_OPS]
AWAY = 4000.0                 # a flow that takes every source out of any image here


def signed_depth(seed, B, H, W):
    """k / 8, k = -9 .. 9: depth sums that are negative, or exactly zero over a non-zero flow sum"""
    rng = np.random.default_rng(seed + 7000)
    return (rng.integers(-9, 10, (B, 1, H, W)) / 8.0).astype(np.float32)


def _fill_case(name):
    B, H, W = (int(v) for v in name.split("-")[0].split("x"))
    # (the seeds of the two thin cases: chosen to meet test_exact_inputs.py's sensitivity floors -- every hole of a row or
    # column of theirs ends at the same stop, so a flow that is flat there hides a walk one cell off from all of them)
    kind, sigma, seed = {"2x70x134-patch-empty": ("smooth", 4.0, None), "1x12x1280-long-rows": ("smooth", 3.0, 19),
                         "1x600x8-long-columns": ("iid", 1.5, 12), "1x40x70-iid6": ("iid", 6.0, None),
                         "2x9x7-iid2": ("iid", 2.0, None), "2x45x132-signed": ("smooth", 5.0, None)}[name]
    if seed is None:
        seed = 8000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    f = synth.np_flow(np.random.default_rng(seed), B, H, W, kind, sigma)
    if name == "2x70x134-patch-empty":
        f[0, :, 20:60, 30:110] = AWAY                                # a 40 x 80 hole over several tiles
        f[1] = AWAY                                                  # nothing lands in image 1: every cell an unfilled hole
    elif name == "1x12x1280-long-rows":
        f[0, :, :, :800] = AWAY
    elif name == "1x600x8-long-columns":
        f[0, :, 300:, :] = AWAY
    elif name == "2x45x132-signed":
        f[0, :, 3:9, 10:30] = AWAY
    return f, seed


def projection_signed_depth(name):
    """the signed depth plane of a case of PROJECTION_SIGNED"""
    B, _, H, W = projection_inputs(name)[0].shape
    # (seed + 2: the first draw with which 2x70x134-patch-empty meets its sensitivity floor of 0.9 under signed depths too)
    return _once(("projsigned", name), lambda: signed_depth(_fill_case(name)[1] + 2, B, H, W))


def projection_operator(name, op):
    """(flow, depth or None) of a case under one of the three operators: flow, depth (k / 8 > 0), signed (k / 8, any sign)"""
    flow, dep = projection_inputs(name)
    return flow, {"flow": None, "depth": dep, "signed": projection_signed_depth(name) if op == "signed" else None}[op]


def fill_expectation(out, count):
    """oracle/memc_oracle.c project_fillhole on out [B, 2, H, W] (fp32: the averaged output, holes not yet filled) and
    count [B, 1, H, W], in float64 and without a loop per hole.  A hole is a cell with count <= 0.  Its three walks (left,
    right, up; there is no downward walk) stop at the nearest cell with count != 0, or at the image border with nothing
    found; a stop contributes iff its count is > 0 (flags fl, fr, fu; n = fl + fr + fu).  The hole is KEPT when the sum of
    the three stops' counts (0 where nothing was found) is <= 0 and FILLED otherwise with
        v = (fl vl + fr vr + fu vu) / n,     and    S = (fl |vl| + fr |vr| + fu |vu|) / n
    is what an error bound is relative to (|v| can cancel to nothing).  Returns (v, S [B, 2, H, W]; n, filled, kept
    [B, 1, H, W]); v and S are 0 outside `filled`.  Counts must be exact in float64 (they are on this module's grid)."""
    o, c = np.asarray(out, dtype=np.float64), np.asarray(count, dtype=np.float64)
    B, _, H, W = o.shape
    lo, ro, uo = LP.proj_fill_walks(c)
    b = np.arange(B)[:, None, None]
    xs, ys = np.broadcast_to(np.arange(W)[None, None, :], lo.shape), np.broadcast_to(np.arange(H)[None, :, None], lo.shape)
    stops = ((lo >= 0, ys, np.maximum(lo, 0)), (ro >= 0, ys, np.maximum(ro, 0)), (uo >= 0, np.maximum(uo, 0), xs))
    cs = [np.where(found, c[:, 0][b, yy, xx], 0.0) for found, yy, xx in stops]
    flags = [(ck > 0).astype(np.float64) for ck in cs]
    n = flags[0] + flags[1] + flags[2]
    hole = c[:, 0] <= 0
    filled = hole & (cs[0] + cs[1] + cs[2] > 0)
    v, S = np.zeros_like(o), np.zeros_like(o)
    for k in (0, 1):
        vals = [np.where(fl > 0, o[:, k][b, yy, xx], 0.0) for fl, (_found, yy, xx) in zip(flags, stops)]
        v[:, k] = np.where(filled, sum(vals) / np.maximum(n, 1.0), 0.0)
        S[:, k] = np.where(filled, sum(np.abs(a) for a in vals) / np.maximum(n, 1.0), 0.0)
    return v, S, n[:, None], filled[:, None], (hole & ~filled)[:, None]


FILL_BOUND = 2.0 ** -21       # the kernels' fill: |got - v| <= FILL_BOUND * S (derived in tests/test_gpu_exact.py)


def fill_sensitivity(out, count):
    """The share of filled holes at which taking, for ONE used neighbour, the next cell outward instead (left of the left
    stop, right of the right stop, above the upper stop; only where that cell is inside the image and has count > 0) moves a
    component of the fill by more than 4 * FILL_BOUND * S: what a walk that is one cell off cannot hide behind the bound.
    (share, filled holes)"""
    o, c = np.asarray(out, dtype=np.float64), np.asarray(count, dtype=np.float64)[:, 0]
    B, _, H, W = o.shape
    _v, S, n, filled, _kept = fill_expectation(out, count)
    lo, ro, uo = LP.proj_fill_walks(count)
    b = np.arange(B)[:, None, None]
    xs, ys = np.broadcast_to(np.arange(W)[None, None, :], lo.shape), np.broadcast_to(np.arange(H)[None, :, None], lo.shape)
    moved = np.zeros(lo.shape, bool)
    for pos, dy, dx in ((lo, 0, -1), (ro, 0, 1), (uo, -1, 0)):
        y0, x0 = (np.maximum(pos, 0), xs) if dy else (ys, np.maximum(pos, 0))
        y1, x1 = y0 + dy, x0 + dx
        inside = (pos >= 0) & (y1 >= 0) & (x1 >= 0) & (x1 < W)
        y1, x1 = np.clip(y1, 0, H - 1), np.clip(x1, 0, W - 1)
        ok = inside & (c[b, y0, x0] > 0) & (c[b, y1, x1] > 0)
        for k in (0, 1):
            delta = np.abs(o[:, k][b, y1, x1] - o[:, k][b, y0, x0]) / np.maximum(n[:, 0], 1.0)
            moved |= ok & (delta > 4.0 * FILL_BOUND * S[:, k])
    f = filled[:, 0]
    return (float((moved & f).sum()) / max(int(f.sum()), 1)), int(f.sum())


# ------------------------------------------------------------------------------------------------------------------
# projection backward: the ABI takes count (and the forward's output) as INPUTS, so they are synthetic here
# ------------------------------------------------------------------------------------------------------------------
# (B, H, W, flow kind, sigma, seed): the flow is the first draw from default_rng(seed), quantised
PB_SMALL = [
    (1, 17, 9, "iid", 2.0, 70),            # the tiled kernel on two quads, one column behind them
    (2, 9, 7, "iid", 1.5, 71),             # one lane per site: ws = 4 < 8
    (2, 6, 3, "iid", 1.0, 72),             # one lane per site: below one quad
    (1, 40, 134, "smooth", 6.0, 73),       # two columns behind the quads
    (2, 33, 131, "iid", 12.0, 74),         # ragged staging of a clipped box, three columns behind the quads
]
PB_SHAPES = ["W50-C3", "W133-C3", "W4-C3"]  # of SHAPES below: the flow only


def _pb_id(c):
    return "%dx%dx%d-%s%g" % c[:5]


PB_IDS = TABLE_IDS + PB_SHAPES + [_pb_id(c) for c in PB_SMALL]
PB_SCALAR = [_pb_id(c) for c in PB_SMALL[1:3]]


def pb_flow(name):
    if name in TABLE_IDS:
        return table_flow(TABLE[TABLE_IDS.index(name)])
    if name in PB_SHAPES:
        return shaped_inputs(*SHAPES[name])[1]
    B, H, W, kind, sigma, seed = PB_SMALL[[_pb_id(c) for c in PB_SMALL].index(name)]
    return quantise_flow(synth.np_flow(np.random.default_rng(seed), B, H, W, kind, sigma))


def _pb_seed(name):
    return 4000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


def proj_bwd_inputs(name, with_depth):
    """dict flow, depth, count, fwd_out, gout of a projection-backward case (depth, fwd_out: the depth operator only).
    count: +-2^e where the true scatter puts anything (e in 0..4; with a depth -2..4 and a random sign: real depth counts
    can be negative), exactly 0 elsewhere -- the tiled kernel stages 1 / 0 = inf there, which no valid site may read.
    gradoutput: integers in [-G, G]; on the cells of count 0 its first plane alternates between 0 and a non-zero value
    (inf * 0 = NaN, inf * g = inf: a wrong read shows either way).  fwd_out: multiples of 1/4 in [-64, 64]."""
    def make():
        flow = pb_flow(name)
        B, _, H, W = flow.shape
        rng = np.random.default_rng(_pb_seed(name) + (1 if with_depth else 0))
        hit = project_sums(flow)[1] > 0
        e = rng.integers(-2 if with_depth else 0, 5, hit.shape)
        sign = np.where(rng.integers(0, 2, hit.shape) == 1, -1.0, 1.0) if with_depth else 1.0
        count = np.where(hit, sign * 2.0 ** e, 0.0).astype(np.float32)
        gout = rng.integers(-G, G + 1, (B, 2, H, W)).astype(np.float32)
        z = np.flatnonzero(~hit[:, 0])
        g0 = gout[:, 0].copy().reshape(-1)
        g0[z[0::2]] = 0.0
        g0[z[1::2]] = np.where(g0[z[1::2]] == 0, 5.0, g0[z[1::2]])
        gout[:, 0] = g0.reshape(B, H, W)
        h = dict(flow=flow, count=count, gout=gout, depth=None, fwd_out=None)
        if with_depth:
            h["depth"] = depth(_pb_seed(name), B, H, W)
            h["fwd_out"] = (rng.integers(-256, 257, (B, 2, H, W)) / 4.0).astype(np.float32)
        return h
    return _once(("pb", name, bool(with_depth)), make)


def proj_bwd_budget(h):
    """M per output of the projection backward, from the data: the sums of absolute terms over the four corners of every
    valid site.  pb_quot: the largest |gradoutput / count| a site reads."""
    flow, cnt, gout = h["flow"], np.abs(h["count"][:, 0]).astype(np.float64), np.abs(h["gout"]).astype(np.float64)
    valid, L, T, R, Bm, _x2, _y2 = LP.bl_locate(flow)
    b = np.arange(flow.shape[0])[:, None, None]
    corners = [(T, L), (T, R), (Bm, L), (Bm, R)]
    assert all((cnt[b, yy, xx][valid] > 0).all() for yy, xx in corners), "a valid site reads a count of zero"
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = [[np.where(valid, gout[:, k][b, yy, xx] / cnt[b, yy, xx], 0.0) for yy, xx in corners] for k in (0, 1)]
    if h["depth"] is None:
        return dict(pb_quot=float(max(q.max() for qs in quot for q in qs)), pb_g1=float(max(sum(qs).max() for qs in quot)))
    d, fo = h["depth"][:, 0].astype(np.float64), np.abs(h["fwd_out"]).astype(np.float64)
    g2 = sum(quot[k][i] * (np.abs(flow[:, k]).astype(np.float64) + fo[:, k][b, yy, xx])
             for k in (0, 1) for i, (yy, xx) in enumerate(corners))
    return dict(pb_quot=float(max(q.max() for qs in quot for q in qs)), dpb_g1=float(max((sum(qs) * d).max() for qs in quot)),
                dpb_g2=float(g2.max()))


def context(seed, B, C, H, W):
    """context features on the image's grid, k / 16; from a generator of their own"""
    return (np.random.default_rng(seed + 5000).integers(0, 16, (B, C, H, W)) / 16.0).astype(np.float32)


# context channels per table case: 8 everywhere, 64 on the first case and 4 on the minimum width as well
CTX_CHANNELS = [[8, 64], [8], [8], [8], [8], [8], [8, 4], [8], [8]]


def ctx_inputs(case, C):
    """(c0, c2): the context features of the two directions of blend_inputs(case)"""
    def make():
        B, H, W, _kind, _sigma, seed = case
        return context(seed, B, C, H, W), context(seed + 100, B, C, H, W)
    return _once(("ctx", case, C), make)


# the layer: the fused route on LAYER_CASE and the two shapes it composes from the separate operators
CTX_LAYER = ["fused-C8", "composed-C6", "composed-W50"]


def ctx_layer_inputs(name):
    """the ten inputs of FilterInterpolationCtxBlendModule by name, as a dict (blend_inputs' names plus c0, c2)"""
    def make():
        if name == "composed-W50":
            B, _C, H, W, kind, sigma, seed, _taps = SHAPES["W50-C3"]
            h = dict(parity_blend_inputs((B, 3, H, W, kind, sigma, seed)))
            C = 8
        else:
            B, H, W, _kind, _sigma, seed = LAYER_CASE
            h = dict(blend_inputs(LAYER_CASE))
            C = 8 if name == "fused-C8" else 6
        h["c0"], h["c2"] = context(seed, B, C, H, W), context(seed + 100, B, C, H, W)
        return h
    return _once(("ctxlayer", name), make)


# x4 upsampling of a scaled flow (flow_prologue.hip): (B, C, h, w) and (mul, div)
UPSAMPLE_SHAPES = [
    (1, 2, 3, 323),        # the column loop's second trip, three columns
    (1, 2, 2, 700),        # three trips, the last one partial
    (1, 2, 2, 65),         # 128 lanes
    (2, 2, 5, 13),
    (1, 1, 1, 1),
]
UPSAMPLE_SCALES = [(20.0, 2.0), (6.0, 3.0)]        # a power-of-two divisor (multiplied by its reciprocal) and one that divides


def upsample_input(shape):
    """seeded multiples of 1/4 in [-64, 64]: (mul * f) / div is exact for both scales (5 k / 2 and k / 2), the weights of
    align_corners = False are multiples of 1/8 per axis: quantum 2^-7, values below 2^10"""
    return _once(("up", shape), lambda: (np.random.default_rng(6000 + sum(shape)).integers(-256, 257, shape) / 4.0).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------
# the proof obligations
# ------------------------------------------------------------------------------------------------------------------
def flow_bound(C, g=G, occ=1.0):
    """sum of absolute terms of a flow gradient: per channel and tap |gradoutput| * tap * (four pixels, two weights that add
    up to one) <= 2 g even when the kernel expands the pixel differences: 16 taps * 2 = 32 (the mix itself stays below 16)"""
    return 32.0 * C * g * occ


def budget(O, x, flow, filt, gout, occ=None):
    """M per output of the adaptive warp: the oracle O (fp32 or float64 front-end) on |gradoutput| and the non-negative
    image and taps, where no term cancels; the flow gradient's analytic bound.  occ: the blend's backward (gradoutput * occ)."""
    assert x.min() >= 0 and filt.min() >= 0
    C = x.shape[1]
    ga = np.abs(gout if occ is None else gout * occ).astype(np.float32)
    g1, _g2, g3 = O.filter_interpolation_backward(x, flow, filt, ga)
    fwd = O.filter_interpolation_forward(x, flow, filt)
    m = dict(fi_fwd=float(fwd.max()), fi_image=float(g1.max()), fi_taps=float(g3.max()), fi_flow=flow_bound(C))
    if occ is not None:
        m = dict(blend_fwd=2.0 * float(fwd.max()), blend_taps=m["fi_taps"], blend_flow=m["fi_flow"],
                 blend_occ=float(C * G * fwd.max()))
    return m


def bilinear_budget(O, x, flow, gout):
    assert x.min() >= 0
    g1, _ = O.interpolation_ch_backward(x, flow, np.abs(gout))
    return dict(bl_fwd=float(O.interpolation_ch_forward(x, flow).max()), bl_image=float(g1.max()),
                bl_flow=4.0 * x.shape[1] * G)              # per channel |gradoutput| * four pixels below one


def holds(m):
    """M * 2^q < 2^24 for every output of m"""
    return all(v * 2.0 ** Q[k] < LIMIT for k, v in m.items())


def border_sites(flow):
    """sites exactly on the edges of the validity test: valid ones on x2 == 0, x2 == W - 1, y2 == 0, y2 == H - 1 (the `<=` /
    `>=` sides) and sites with |fx| == W / 2, |fy| == H / 2 (invalid by the strict `<`)"""
    B, _, H, W = flow.shape
    valid, _, _ = LP.locate(flow)
    fx, fy = flow[:, 0], flow[:, 1]
    x2 = np.arange(W, dtype=np.float32)[None, None, :] + fx
    y2 = np.arange(H, dtype=np.float32)[None, :, None] + fy
    return dict(x2_0=int((valid & (x2 == 0)).sum()), x2_last=int((valid & (x2 == W - 1)).sum()),
                y2_0=int((valid & (y2 == 0)).sum()), y2_last=int((valid & (y2 == H - 1)).sum()),
                fx_half=int((np.abs(fx) == W / 2.0).sum()), fy_half=int((np.abs(fy) == H / 2.0).sum()))


# ------------------------------------------------------------------------------------------------------------------
# the cases tests/test_gpu_exact.py runs and tests/test_exact_inputs.py proves, by name
# ------------------------------------------------------------------------------------------------------------------
STORAGES = ["fp32", "fp16", "bf16"]
# channel counts of the forward per table case, as test_gpu_lowp_paths.FWD_CHANNELS; the three added cases: RGB
FWD_CHANNELS = [[3, 8, 5, 64], [3, 8, 5, 1], [3, 8, 5, 64], [3, 8, 5], [3, 8, 5], [3, 8, 5], [3], [3], [3]]
# (B, C, H, W, flow kind, sigma, seed, taps): ragged widths (W % 4 = 2, 1), the minimum width, other filter sizes
SHAPES = {
    "W50-C3": (1, 3, 20, 50, "smooth", 3.0, 50, 16), "W50-C8": (1, 8, 20, 50, "smooth", 3.0, 51, 16),
    "W133-C3": (2, 3, 24, 133, "smooth", 5.0, 52, 16), "W133-C8": (2, 8, 24, 133, "smooth", 5.0, 53, 16),
    "W4-C3": (2, 3, 24, 4, "smooth", 1.0, 54, 16), "W4-C8": (2, 8, 24, 4, "smooth", 1.0, 55, 16),
    "fs2": (2, 3, 21, 34, "iid", 3.0, 22, 4), "fs3": (2, 3, 21, 34, "iid", 3.0, 23, 9), "fs6": (2, 3, 21, 34, "iid", 3.0, 26, 36),
}
LAYER_CASE = (2, 40, 64, "smooth", 4.0, 41)          # the layers' 2x3x40x64


def storages_of(case):
    return ["fp32"] if case == FAR else STORAGES


def parity_blend_cases():
    """test_gpu_parity.BLEND_CASES as (B, C, H, W, kind, sigma, seed)"""
    import test_gpu_parity as FP32
    return FP32.BLEND_CASES


def parity_blend_inputs(case):
    def make():
        B, C, H, W, kind, sigma, seed = case
        h = {}
        for d, (x, f, k, o) in enumerate((("x0", "f0", "k0", "o0"), ("x2", "f1", "k1", "o1"))):
            h[x], h[f], h[k], _ = shaped_inputs(B, C, H, W, kind, sigma, seed + 100 * d)
            h[o] = occlusion(seed + 100 * d, B, H, W)
        h["gout"] = shaped_inputs(B, C, H, W, kind, sigma, seed)[3]
        return h
    return _once(("pblend", case), make)


def bilinear_rgb_cases():
    """table cases 0, 2, 5: (id, image, flow, gradoutput)"""
    for ci in (0, 2, 5):
        x, flow, _filt, gout = table_inputs(TABLE[ci], 3)
        yield TABLE_IDS[ci], x, flow, gout


def many_rows():
    import test_gpu_parity as FP32
    return FP32.MANY
