"""tests/_lp_bl_cases.py -- the inputs of the fp16 / bf16 bilinear warp's tests (libmemc_hip_lp_bl.so), shared by
tests/test_lp_bl_cases.py (the premises, on the CPU) and tests/test_gpu_lp_bilinear.py (the kernels).

Random cases (B, H, W, flow kind, sigma, seed): the flow is the first draw of np.random.default_rng(seed), rounded to T;
image and gradoutput follow from the same generator, rounded to T.

Exact cases: tests/_exact.bilinear_rgb_cases()'s table cases 0, 2, 5 with the flow stored in T (clipped by _exact.CLIP), plus
one 8-channel instance of table case 0 for the chunk kernel.

The census restates the tiled kernels' staged box (csrc/lp_interpolation.hip: bl_locate<true>, tile_region<16, true, CAP, NT>)
in numpy: per tile the box of its valid sites' corners, fitted to CAP pixel quads, and the valid sites whose corners lie
outside it -- those gather their corners from global memory (forward) or scatter with per-site atomics (backward).
"""
import os
import re
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import _exact as E            # noqa: E402
import _lowp_paths as LP      # noqa: E402
from tools import synth       # noqa: E402

TNAMES = ("fp16", "bf16")
CSRC = os.path.join(LP.ROOT, "memc-net_amd", "csrc")

#   1x8x8      the minimum tiled width, one partial tile
#   2x20x72    2 x 2 forward tiles of 64 x 16, partial in both directions, a batch stride
#   1x40x136   an i.i.d. flow of sigma 12: staged boxes clipped in x and y, corners gathered from global memory
#   1x72x136   the same for the backward's 64 x 32 tiles
RANDOM = [(1, 8, 8, "smooth", 2.0, 301), (2, 20, 72, "smooth", 4.0, 302), (1, 40, 136, "iid", 12.0, 303),
          (1, 72, 136, "iid", 20.0, 305)]
RANDOM_IDS = ["%dx%dx%d-%s%g" % c[:5] for c in RANDOM]
SMOOTH, IID_FWD, IID_BWD = RANDOM[:2], RANDOM[2], RANDOM[3]
ORDINARY = RANDOM[1]          # the case held to the oracle under tests/_netcalls.rule_rounded
FWD_CHANNELS = (3, 1, 2, 5, 8)
BWD_CHANNELS = (3,)
DECLINED_CHANNELS = 8         # the backward's declined channel count


def is_number_of(a, tname):
    return bool((LP.rounded(a, tname) == np.asarray(a, dtype=np.float32)).all())


def random_flow(case, tname):
    B, H, W, kind, sigma, seed = case
    return LP.rounded(synth.np_flow(np.random.default_rng(seed), B, H, W, kind, sigma), tname)


def random_inputs(case, C, tname):
    """(image, flow, gradoutput): float32 numpy, numbers of T; never written"""
    def make():
        B, H, W, kind, sigma, seed = case
        rng = np.random.default_rng(seed)
        flow = LP.rounded(synth.np_flow(rng, B, H, W, kind, sigma), tname)
        x = LP.rounded(synth.np_image(rng, B, C, H, W), tname)
        gout = LP.rounded(rng.standard_normal((B, C, H, W)).astype(np.float32), tname)
        return x, flow, gout
    return E._once(("lp-bl", case, C, tname), make)


EXACT_TABLE = (0, 2, 5)       # _exact.bilinear_rgb_cases()'s table cases
EXACT_IDS = [E.TABLE_IDS[ci] for ci in EXACT_TABLE]
EXACT_C8 = E.TABLE_IDS[0] + "-C8"


def exact_inputs(name, tname):
    """(image, flow, gradoutput) of an exact case with its flow stored in T: EXACT_IDS in RGB, EXACT_C8 in 8 channels"""
    C = 8 if name == EXACT_C8 else 3
    ci = E.TABLE_IDS.index(name[:-3] if name == EXACT_C8 else name)
    x, flow, _filt, gout = E.table_inputs(E.TABLE[ci], C, tname)
    return x, flow, gout


# ------------------------------------------------------------------------------------------------------------------
# the census
# ------------------------------------------------------------------------------------------------------------------
def source_constants():
    """what the census needs of the sources' text: the staging budgets of the three tiled kernels, the lanes of their
    workgroups, the tile geometry of memc_tile.hpp"""
    with open(os.path.join(CSRC, "lp_interpolation.hip")) as f:
        text = f.read()

    def one(pattern, what, t=text):
        m = re.findall(pattern, t)
        assert len(m) == 1, "expected exactly one `%s` (%s), found %d" % (pattern, what, len(m))
        return m[0]
    k = dict(cap_c3=int(one(r"launch_bl_fwd_lp_tiled<3, (\d+)>\(k\)", "the RGB forward's budget")),
             cap_chunks=int(one(r"launch_bl_fwd_lp_tiled<0, (\d+)>\(k\)", "the chunk forward's budget")))
    cap, nt = one(r"constexpr int kBlBwdCap = (\d+), kBlBwdNT = (\d+);", "the backward's budget and lanes")
    k.update(cap_bwd=int(cap), nt_bwd=int(nt))
    fwd_nt = one(r"bl_fwd_lp_tiled<T, FT, CT, CAP>\), dim3\(walk_grid\(g\.ntx, g\.nty, k\.batch, sw\)\), dim3\((\d+)\)",
                 "the forward's lanes")
    k["nt_fwd"] = int(fwd_nt)
    one(r"tile_region<LX, true, CAP>\(cmin, cmax, rmin, rmax, tile_x0, tile_y0, bb\)", "the forward's box")
    one(r"tile_region<LX, true, CAP, NT>\(cmin, cmax, rmin, rmax, tile_x0, tile_y0, bb\)", "the backward's box")
    with open(os.path.join(CSRC, "memc_tile.hpp")) as f:
        tile = f.read()
    one(r"static constexpr int kTW = 4 \* LX;", "tile width", tile)
    one(r"static constexpr int kTH = kThreads / LX;", "tile height", tile)
    one(r"static constexpr int kPitch = kTW \+ (32);", "pitch", tile)
    one(r"y0 = min\(max\(tile_y0 \+ G::kTH / 2 - rows / 2, lo\), hi\);", "the clip in y", tile)
    one(r"x0 = min\(max\(\(tile_x0 \+ G::kTW / 2 - G::kPitch / 2\) & ~3, lo\), hi\);", "the clip in x", tile)
    k["th_fwd"], k["th_bwd"] = k["nt_fwd"] // LP.LX, k["nt_bwd"] // LP.LX
    return k


def bl_locate(flow):
    """bl_locate<true> of memc_common.hpp (the bilinear warp's strict test, x2 < W) for every site, in float32:
    (valid, L, T, R, Bm); invalid sites: L = T = 0"""
    B, _, H, W = flow.shape
    fx, fy = flow[:, 0].astype(np.float32), flow[:, 1].astype(np.float32)
    x2 = np.arange(W, dtype=np.float32)[None, None, :] + fx
    y2 = np.arange(H, dtype=np.float32)[None, :, None] + fy
    valid = (x2 >= 0) & (y2 >= 0) & (x2 < np.float32(W)) & (y2 < np.float32(H))
    L = np.where(valid, x2, 0).astype(np.int32)
    T = np.where(valid, y2, 0).astype(np.int32)
    return valid, L, T, np.minimum(L + 1, W - 1), np.minimum(T + 1, H - 1)


def tile_region(cmin, cmax, rmin, rmax, tile_x0, tile_y0, cap, th):
    """tile_region<16, true, cap, 16 * th> of memc_tile.hpp for the box of a tile's valid sites (TileGeom<16, cap, 16 * th>:
    tiles of 64 x th sites, pitch 96): (x0, y0, w, h, clipped in x, in y)"""
    TW, PITCH = LP.TW, LP.PITCH
    x0, y0 = cmin & ~3, rmin
    w, h = (cmax | 3) + 1 - x0, rmax + 1 - y0
    clip_x = w > PITCH
    if clip_x:
        lo, hi = x0, x0 + w - PITCH
        x0 = min(max((tile_x0 + TW // 2 - PITCH // 2) & ~3, lo), hi)
        w = PITCH
    pitch = (w + 15) & ~15
    rows = cap // pitch
    clip_y = h > rows
    if clip_y:
        lo, hi = y0, y0 + h - rows
        y0 = min(max(tile_y0 + th // 2 - rows // 2, lo), hi)
        h = rows
    return x0, y0, w, h, clip_x, clip_y


def census(flow, cap, th):
    """Counts over the 64 x th tiles of flow [B, 2, H, W] under a staging budget of `cap` pixel quads"""
    B, _, H, W = flow.shape
    assert W % 4 == 0 and W >= 8
    TW = LP.TW
    valid, L, T, R, Bm = bl_locate(flow)
    out = dict(sites=int(valid.size), valid=int(valid.sum()), tiles=0, empty=0, clip_x=0, clip_y=0, uncovered=0)
    for b in range(B):
        for ty in range((H + th - 1) // th):
            for tx in range((W + TW - 1) // TW):
                ys, xs = slice(ty * th, min(ty * th + th, H)), slice(tx * TW, min(tx * TW + TW, W))
                v = valid[b, ys, xs]
                out["tiles"] += 1
                if not v.any():
                    out["empty"] += 1
                    continue
                l, t, r, bm = L[b, ys, xs], T[b, ys, xs], R[b, ys, xs], Bm[b, ys, xs]
                x0, y0, w, h, cx, cy = tile_region(int(l[v].min()), int(r[v].max()), int(t[v].min()), int(bm[v].max()),
                                                   tx * TW, ty * th, cap, th)
                out["clip_x"] += cx
                out["clip_y"] += cy
                out["uncovered"] += int((v & ~((l >= x0) & (r < x0 + w) & (t >= y0) & (bm < y0 + h))).sum())
    return {k: int(x) for k, x in out.items()}
