"""tests/_lowp_paths.py -- which in-kernel path of the tiled fp16 / bf16 warps an input runs, counted on the CPU.

libmemc_hip_lp.so and libmemc_hip_lp_grad.so report only the kernel family of a call (last_kernel_path()); whether a tile
swept several LDS bands, hit the kMaxBands cap, sent sites to the per-site loop from global memory or stored a lane's four
sites in pieces is decided inside the kernel.  This module restates that decision in numpy (memc-net_amd/csrc: fi_locate
of memc_common.hpp; TileGeom<16>, tile_bbox, make_bands<16, true, 3072>, band_region of memc_tile.hpp; fi_covered of
memc_fi.hpp; the `done` bookkeeping of fi_fwd_lp_tiled, fi_blend_lp_tiled and fi_bwd_c3_body.inc, which all three share)
so that a test can state which paths its inputs reach.  tests/test_lowp_path_census.py holds the constants below to the
header's text and the case table to its conditions; tests/test_gpu_lowp_paths.py runs the table on the GPU.

The last section does the same for the projection backward (flow_projection.hip: launch_proj_bwd's routing, bl_locate<false>,
tile_region<16, true, 2496>, Region::covers): which sites the tiled kernel gathers from global memory, which tiles clip
their staged box, which columns go to the one-lane-per-site kernel.  tests/test_exact_inputs.py holds it to the sources'
text and the cases of tests/_exact.py to their conditions.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tools import synth      # noqa: E402

# geometry the census assumes (test_lowp_path_census.py reads the same values out of memc_tile.hpp)
LX = 16                      # lanes per tile row
TW, TH = 4 * LX, 256 // LX   # 64 x 16 sites per tile, four consecutive sites of a row per lane
PITCH = TW + 32              # kPitch
CAP = 3072                   # LDS budget in pixel quads
MAX_BANDS = 6                # kMaxBands
STEP_X = (PITCH - 4) & ~3    # 92: bands overlap by four columns

# (B, H, W, flow kind, sigma, seed): the flow is the FIRST draw from np.random.default_rng(seed)
CASES = [
    (1, 96, 256, "smooth", 25.0, 16),      # bands in both directions, one capped tile, a handful of slow sites
    (2, 64, 256, "iid", 20.0, 8),          # every tile sweeps the full six bands, nothing slow, thousands of split lanes
    (1, 112, 320, "iid", 30.0, 22),        # most tiles capped: thousands of slow sites
    (1, 200, 320, "smooth", 40.0, 23),     # capped tiles under smooth motion; a ragged last tile row (200 = 12 * 16 + 8)
    (2, 100, 132, "smooth", 8.0, 12),      # tiles without a valid site; 4-column edge tiles (132 = 2 * 64 + 4)
    (1, 40, 40, "iid", 30.0, 6),           # three partial tiles, mostly invalid sites, lanes of mixed validity
]
CASE_IDS = ["%dx%dx%d-%s%g" % c[:5] for c in CASES]
BLEND_CASES = CASES[:4]                    # the second direction's flow: the first draw from seed + 100


def case_flow(case, second=False):
    B, H, W, kind, sigma, seed = case
    return synth.np_flow(np.random.default_rng(seed + (100 if second else 0)), B, H, W, kind, sigma)


def case_inputs(case, C, signed_gradient=True):
    """(image, flow, taps, gradoutput) of a table case: the flow first, then the rest from the same generator"""
    B, H, W, kind, sigma, seed = case
    rng = np.random.default_rng(seed)
    flow = synth.np_flow(rng, B, H, W, kind, sigma)
    x, filt = synth.np_image(rng, B, C, H, W), synth.np_filter(rng, B, H, W)
    gout = rng.standard_normal((B, C, H, W)).astype(np.float32) if signed_gradient else synth.np_image(rng, B, C, H, W)
    return x, flow, filt, gout


def rounded(a, tname):
    """a (fp32 numpy) rounded to fp16 / bf16 and widened again; "fp32": unchanged"""
    if tname == "fp32":
        return np.ascontiguousarray(a, dtype=np.float32)
    import torch
    T = {"fp16": torch.float16, "bf16": torch.bfloat16}[tname]
    return torch.from_numpy(np.ascontiguousarray(a)).to(T).float().numpy()


def locate(flow):
    """fi_locate for every site, in float32 as the kernels compute it: (valid, ix, iy)"""
    B, _, H, W = flow.shape
    fx, fy = flow[:, 0].astype(np.float32), flow[:, 1].astype(np.float32)
    x2 = np.arange(W, dtype=np.float32)[None, None, :] + fx
    y2 = np.arange(H, dtype=np.float32)[None, :, None] + fy
    valid = ((x2 >= 0) & (y2 >= 0) & (x2 <= np.float32(W - 1)) & (y2 <= np.float32(H - 1)) &
             (np.abs(fx) < np.float32(W) / np.float32(2)) & (np.abs(fy) < np.float32(H) / np.float32(2)))
    ix = np.where(valid, x2, 0).astype(np.int32)
    iy = np.where(valid, y2, 0).astype(np.int32)
    return valid, ix, iy


def make_bands(bw_, bh_):
    """make_bands<16, true, 3072> for an unclipped box of bw_ x bh_ pixels: (nbx, nby, bw, bh, sy)"""
    bw = min(bw_, PITCH)
    pitch = max((bw + 15) & ~15, 16)
    rows = CAP // pitch
    bh = min(bh_, rows)
    sy = rows - 3
    nbx = (bw_ - bw + STEP_X - 1) // STEP_X + 1 if bw_ > bw else 1
    nby = (bh_ - bh + sy - 1) // sy + 1 if bh_ > bh else 1
    return nbx, nby, bw, bh, sy


def census(flow):
    """Counts over every 64 x 16 tile of flow [B, 2, H, W] (W % 4 == 0: the tiled kernels' precondition)."""
    B, _, H, W = flow.shape
    assert W % 4 == 0 and W >= 8
    valid, ix, iy = locate(flow)
    c0, c1 = np.maximum(ix - 1, 0), np.minimum(ix + 2, W - 1)      # the clamped 4 x 4 window of a site
    r0, r1 = np.maximum(iy - 1, 0), np.minimum(iy + 2, H - 1)
    out = dict(tiles=0, empty=0, nbx_gt1=0, nby_gt1=0, capped=0, max_bands_run=0, slow=0, split_lanes=0, mixed_lanes=0,
               valid=int(valid.sum()), sites=int(valid.size), ragged_rows=H % TH, ragged_cols=W % TW)
    for b in range(B):
        for ty in range((H + TH - 1) // TH):
            for tx in range((W + TW - 1) // TW):
                ys, xs = slice(ty * TH, min(ty * TH + TH, H)), slice(tx * TW, min(tx * TW + TW, W))
                v = valid[b, ys, xs]
                out["tiles"] += 1
                nv = v.reshape(v.shape[0], -1, 4).sum(-1)
                out["mixed_lanes"] += int(((nv > 0) & (nv < 4)).sum())
                if not v.any():                                    # box.w == 0: one round that copies the input pixels
                    out["empty"] += 1
                    continue
                C0, C1, R0, R1 = c0[b, ys, xs], c1[b, ys, xs], r0[b, ys, xs], r1[b, ys, xs]
                # tile_bbox
                bx0 = int(C0[v].min()) & ~3
                bw_ = (int(C1[v].max()) | 3) + 1 - bx0
                by0 = int(R0[v].min())
                bh_ = int(R1[v].max()) + 1 - by0
                nbx, nby, bw, bh, sy = make_bands(bw_, bh_)
                n = min(nbx * nby, MAX_BANDS)
                out["nbx_gt1"] += nbx > 1
                out["nby_gt1"] += nby > 1
                out["capped"] += nbx * nby > MAX_BANDS
                done = np.zeros_like(v)
                run = 0
                for bi in range(n):
                    # band_region, fi_covered
                    rx0 = min(bx0 + (bi % nbx) * STEP_X, bx0 + bw_ - bw)
                    ry0 = min(by0 + (bi // nbx) * sy, by0 + bh_ - bh)
                    sel = v & (C0 >= rx0) & (C1 < rx0 + bw) & (R0 >= ry0) & (R1 < ry0 + bh) & ~done
                    if bi > 0 and not sel.any():                   # the vote: nobody needs this band
                        continue
                    run += 1
                    done |= sel
                    wr = sel | ~v if bi == 0 else sel              # band 0 also writes the out-of-range sites
                    w4 = wr.reshape(wr.shape[0], -1, 4).sum(-1)
                    out["split_lanes"] += int(((w4 > 0) & (w4 < 4)).sum())
                out["max_bands_run"] = max(out["max_bands_run"], run)
                out["slow"] += int((v & ~done).sum())
    return {k: int(x) for k, x in out.items()}


# ------------------------------------------------------------------------------------------------------------------
# the projection backward (flow_projection.hip: launch_proj_bwd, proj_bwd_tiled<DEPTH, 2496, RAG>, proj_bwd<DEPTH>)
# ------------------------------------------------------------------------------------------------------------------
PB_CAP = 2496                # the staging budget launch_proj_bwd instantiates (test_exact_inputs.py reads it out of the source)


def bl_locate(flow):
    """bl_locate<false> of memc_common.hpp for every site, in float32: (valid, L, T, R, Bm, x2, y2); invalid sites: L = T = 0"""
    B, _, H, W = flow.shape
    fx, fy = flow[:, 0].astype(np.float32), flow[:, 1].astype(np.float32)
    x2 = np.arange(W, dtype=np.float32)[None, None, :] + fx
    y2 = np.arange(H, dtype=np.float32)[None, :, None] + fy
    valid = (x2 >= 0) & (y2 >= 0) & (x2 <= np.float32(W - 1)) & (y2 <= np.float32(H - 1))
    L = np.where(valid, x2, 0).astype(np.int32)
    T = np.where(valid, y2, 0).astype(np.int32)
    return valid, L, T, np.minimum(L + 1, W - 1), np.minimum(T + 1, H - 1), x2, y2


def tile_region(cmin, cmax, rmin, rmax, tile_x0, tile_y0, cap=PB_CAP):
    """tile_region<16, true, cap> of memc_tile.hpp for the box of a tile's valid sites: (x0, y0, w, h, clipped in x, in y)"""
    x0, y0 = cmin & ~3, rmin
    w, h = (cmax | 3) + 1 - x0, rmax + 1 - y0
    clip_x = w > PITCH
    if clip_x:                                          # clip around the tile centre, keep 4-alignment
        lo, hi = x0, x0 + w - PITCH
        x0 = min(max((tile_x0 + TW // 2 - PITCH // 2) & ~3, lo), hi)
        w = PITCH
    pitch = (w + 15) & ~15                              # DYN: the narrowest pitch that holds the box buys rows
    rows = cap // pitch
    clip_y = h > rows
    if clip_y:
        lo, hi = y0, y0 + h - rows
        y0 = min(max(tile_y0 + TH // 2 - rows // 2, lo), hi)
        h = rows
    return x0, y0, w, h, clip_x, clip_y


def proj_bwd_route(W):
    """launch_proj_bwd: ("tiled" | "scalar", ws): whole quads (x < ws = W & ~3) on the tiled kernel and the W & 3 columns
    behind them on proj_bwd; a ragged width below two quads on proj_bwd alone"""
    ws = W & ~3
    return ("tiled" if W % 4 == 0 or ws >= 8 else "scalar"), ws


def proj_bwd_census(flow):
    """Counts over the projection backward of flow [B, 2, H, W].  `uncovered`: valid sites of the tiled kernel whose corners
    (L..R, T..Bm) lie outside their tile's staged box (Region::covers fails: the gather from global memory); `mask`: those sites."""
    B, _, H, W = flow.shape
    route, ws = proj_bwd_route(W)
    valid, L, T, R, Bm, x2, y2 = bl_locate(flow)
    out = dict(route=route, ws=ws, sites=int(valid.size), valid=int(valid.sum()), tiles=0, empty=0, clip_x=0, clip_y=0,
               uncovered=0, tiled_valid=0, tail_valid=0, L_eq_R=int((valid & (L == R)).sum()), T_eq_Bm=int((valid & (T == Bm)).sum()),
               x2_0=int((valid & (x2 == 0)).sum()), y2_0=int((valid & (y2 == 0)).sum()))
    mask = np.zeros_like(valid)
    if route == "scalar":
        out["tail_valid"] = out["valid"]                # every site on the one-lane-per-site kernel
        return out, mask
    out["tail_valid"] = int(valid[:, :, ws:].sum())
    for b in range(B):
        for ty in range((H + TH - 1) // TH):
            for tx in range((ws + TW - 1) // TW):
                ys, xs = slice(ty * TH, min(ty * TH + TH, H)), slice(tx * TW, min(tx * TW + TW, ws))
                v = valid[b, ys, xs]
                out["tiles"] += 1
                out["tiled_valid"] += int(v.sum())
                if not v.any():
                    out["empty"] += 1
                    continue
                l, t, r, bm = L[b, ys, xs], T[b, ys, xs], R[b, ys, xs], Bm[b, ys, xs]
                x0, y0, w, h, cx, cy = tile_region(int(l[v].min()), int(r[v].max()), int(t[v].min()), int(bm[v].max()),
                                                   tx * TW, ty * TH)
                out["clip_x"] += cx
                out["clip_y"] += cy
                un = v & ~((l >= x0) & (r < x0 + w) & (t >= y0) & (bm < y0 + h))
                mask[b, ys, xs] = un
                out["uncovered"] += int(un.sum())
    return out, mask


# ------------------------------------------------------------------------------------------------------------------
# the projection forward (flow_projection.hip: launch_proj_fwd's routing; proj_fill.hpp: the 64 x kOwnerTH tiles of the
# owner kernels and of proj_fill_pending, the walks of the hole filling).  tests/test_exact_inputs.py holds the constants
# to the sources' text and the projection cases of tests/_exact.py to their conditions.
# ------------------------------------------------------------------------------------------------------------------
PF_TW, PF_TH = 64, 32        # an owner tile: 64 x kOwnerTH cells


def proj_fwd_route(W):
    """launch_proj_fwd: ("owner" | "scalar", ragged).  vec4_ok is the width alone (memc_tile.hpp: strides and base pointers
    may be anything), so the owner kernels' ragged-row instantiations serve W >= 8 with W % 4 != 0 and nothing else; a
    ragged width below 8 takes the one-lane-per-site kernels and proj_fillhole.  Both owner instantiations record `owner`."""
    if W % 4 == 0:
        return "owner", False
    return ("owner", True) if W >= 8 else ("scalar", False)


def proj_fill_walks(count):
    """The three walks of oracle/memc_oracle.c project_fillhole from EVERY cell of count [B, 1, H, W]: the column of the
    nearest cell with count != 0 to the left and to the right, the row of the nearest one above; -1 where the walk reaches
    the image border with nothing found.  (lo, ro, uo), each [B, H, W]; cumulative maxima of indices, no loop per cell."""
    nz = count[:, 0] != 0
    B, H, W = nz.shape
    xs, ys = np.arange(W)[None, None, :], np.arange(H)[None, :, None]
    last = np.maximum.accumulate(np.where(nz, xs, -1), axis=2)            # the last non-zero column <= x
    lo = np.concatenate([np.full((B, H, 1), -1), last[:, :, :-1]], axis=2)
    first = np.minimum.accumulate(np.where(nz, xs, W)[:, :, ::-1], axis=2)[:, :, ::-1]   # the first non-zero column >= x
    ro = np.concatenate([first[:, :, 1:], np.full((B, H, 1), W)], axis=2)
    ro = np.where(ro == W, -1, ro)
    above = np.maximum.accumulate(np.where(nz, ys, -1), axis=1)
    uo = np.concatenate([np.full((B, 1, W), -1), above[:, :-1, :]], axis=1)
    return lo, ro, uo


def proj_fwd_census(s, count):
    """Counts over the hole filling of the sums s [B, 2, H, W] and count [B, 1, H, W] (float64, exact): per direction the
    walks of the holes (count <= 0) that end in another 64 x 32 tile, that find nothing, and the most tile borders one
    crosses; filled holes by the number n of positive neighbours; tiles without a non-zero cell; and what only signed
    depths reach (negative counts stop a walk, are holes themselves and contribute nothing)."""
    c = count[:, 0]
    B, H, W = c.shape
    lo, ro, uo = proj_fill_walks(count)
    hole = c <= 0
    b = np.arange(B)[:, None, None]
    xs, ys = np.broadcast_to(np.arange(W)[None, None, :], c.shape), np.broadcast_to(np.arange(H)[None, :, None], c.shape)
    cl = np.where(lo >= 0, c[b, ys, np.maximum(lo, 0)], 0.0)
    cr = np.where(ro >= 0, c[b, ys, np.maximum(ro, 0)], 0.0)
    cu = np.where(uo >= 0, c[b, np.maximum(uo, 0), xs], 0.0)
    n = (cl > 0).astype(int) + (cr > 0) + (cu > 0)
    filled = hole & (cl + cr + cu > 0)
    kept = hole & ~filled
    out = dict(route=proj_fwd_route(W)[0], ragged=proj_fwd_route(W)[1], cells=int(c.size), holes=int(hole.sum()),
               filled=int(filled.sum()), kept=int(kept.sum()))
    for k in (1, 2, 3):
        out["n%d" % k] = int((filled & (n == k)).sum())
    for name, pos, own, size in (("l", lo, xs, PF_TW), ("r", ro, xs, PF_TW), ("u", uo, ys, PF_TH)):
        crossed = np.where(hole & (pos >= 0), np.abs(pos // size - own // size), 0)
        out["other_tile_" + name] = int((crossed > 0).sum())
        out["nothing_" + name] = int((hole & (pos < 0)).sum())
        out["borders_" + name] = int(crossed.max())
    nty, ntx = (H + PF_TH - 1) // PF_TH, (W + PF_TW - 1) // PF_TW
    pad = np.zeros((B, nty * PF_TH, ntx * PF_TW), bool)
    pad[:, :H, :W] = c != 0
    out["tiles"] = B * nty * ntx
    out["empty_tiles"] = int((~pad.reshape(B, nty, PF_TH, ntx, PF_TW).any(axis=(2, 4))).sum())
    # what only signed depths reach
    out["negative"] = int((c < 0).sum())
    out["zero_count_nonzero_sum"] = int(((c == 0) & (s != 0).any(axis=1)).sum())
    out["kept_beside_positive"] = int((kept & (n > 0)).sum())
    out["filled_past_negative"] = int((filled & ((cl < 0) | (cr < 0) | (cu < 0))).sum())
    return out
