"""tests/_image_grad.py -- the image gradient of the adaptive warp (gradinput1 of FilterInterpolation) restated in float64,
and a per-cell bound on what a correct fp32 kernel may return for it, whatever order the hardware adds in.

The operation.  A site (x, y) of batch element b with flow (fx, fy) is valid under fi_locate's test (memc_common.hpp; the same
test as tests/_lowp_paths.locate, in float32).  With x2 = x + fx, ix = int(x2), a = x2 - ix (all float32; b from y2 likewise),
tap (k, m) of its fs x fs window lands on the cell
    (clamp(iy + 1 - fs / 2 + k, 0, H - 1), clamp(ix + 1 - fs / 2 + m, 0, W - 1))
and adds, for every channel c, the term
    gradoutput[b, c, y, x] * wa * wb * tap[b, k * fs + m, y, x],     wa = m < fs / 2 ? 1 - a : a,   wb = k < fs / 2 ? 1 - b : b.
The clamp folds window positions beyond the border onto the border cell (fi_bwd_adds_pk: clampi(g.iy[j] - 1 + k, H - 1)).
Only the float32 values of ix, iy, a, b are taken over; the weights 1 - a, their product, the term and the sums are float64.

Per cell, restate() returns `want` (the sum of the terms), `n` (how many terms land in the cell) and `mass` (the sum of
their absolute values).  Plain numpy (np.bincount, one pass per tap and channel); no kernel code and no oracle text is used.

The bound.  bound() adds up, for one cell, every rounding a kernel commits on the way to it.  u = 2^-24 is fp32's unit
roundoff.  Nothing in it is fitted to a result.

  packed planes    n * 2^(e - 23).  memc_pk.hpp: a packed site's contribution is rounded ONCE to a multiple of 2^(e_tile - 22),
                   i.e. by at most 2^(e_tile - 23); the sums of those integers are exact.  e_tile comes from
                   B = min(max s, 16 x mean s) <= max over the tile's sites of (largest |gradoutput|) x (largest |tap|), and
                   B < 2^e_tile <= 2 B (pk_tile_resolve: frexpf).  With 2^e_g / 2^e_t the powers of two strictly above the
                   largest finite |gradoutput| / |tap| of the batch element, the fp32 product of those two maxima stays below
                   2^(e_g + e_t) (the largest floats below the two powers multiply to 2^e (1 - 2^-23 + 2^-48), which rounds
                   down), so e_tile <= e = e_g + e_t for every tile.  Sites that leave the planes (outliers, Inf / NaN sites,
                   slow sites, tiles that take atomics for everything) commit no such rounding: the part covers them too.
                   plane_grid() states the same part with the exponent taken per 64 x 16 site tile (from max s, which B never
                   exceeds): the sum over the cell's terms of 2^(e_M(tile of the term's site) - 23) <= n * 2^(e - 23).  With
                   the per-batch exponent 2 * bound exceeds ulp_fp16(want) in up to 15.9 % of a table case's live cells,
                   with the per-tile one in at most 8.3 %; Reference uses the per-tile form.
  fp32             (n + F) * k * u * mass covers every relative rounding:
                   k = 5 roundings form one term.  MEMC_FI_BWD_SITE_IMAGE_ATOMICS_BODY and fi_bwd_site_scalar (memc_fi.hpp)
                     compute gv * wa * wb * tap: 1 - a, 1 - b and three products.  fi_bwd_adds_pk has four (1 - a, 1 - b,
                     their product, times the tap; the scales st and sg are powers of two, the fma's rounding is the planes'
                     part above); the many-channel owner and the direct kernels (fi_bwd_cn.hip: (wa * wb) * tap, then one
                     product or fma with gradoutput) have five or fewer.  The CPU oracle's g * (1 - a) * (1 - b) * tap has five.
                   n + F roundings of a running sum: every add into the cell carries at least one of its n terms, so there are
                     at most n adds, each rounding a partial sum that is at most mass (1 + small) in magnitude; a flush add
                     (pk_flush) rounds its value a second time, when the exact integer sum is converted to float.  F bounds
                     the flush adds of a cell: each carries at least one term, so F = n.  (The geometry gives nothing smaller
                     in general: under i.i.d. motion a cell's n terms come from n different tiles.)
                   To first order the error is (k + n + F) u mass; the product (n + F) k is larger for every n >= 1 and
                   leaves room for the second-order terms ((1 + u)^(n + F + k) - 1 <= 1.01 (n + F + k) u for n < 2^14).
                   Without planes (F = 0) the same count gives n * k * u * mass: at most n roundings of partial sums (the owner
                   kernels' fmas, their segment sums -- one per kSegLen entries -- and slab adds; the direct kernel's atomics).
  underflow        n * k * 2^-126: a product that leaves the normal range is off by at most the smallest normal float,
                   whether the hardware keeps or flushes denormals.
  storage          ulp_T(want) / 2 when the result was rounded once more to T (the layers' .grad); the ulp is that of T's
                   binade that holds |want| + the rest of the bound, so that a sum just below a power of two is covered.
"""
import numpy as np

U = 2.0 ** -24               # fp32 unit roundoff
K_TERM = 5                   # roundings that form one term (see above)
MANT = {"fp16": (10, -14), "bf16": (7, -126)}      # (stored mantissa bits, exponent of the smallest normal)


def locate32(flow):
    """fi_locate in float32 for flow [B, 2, H, W]: (valid, ix, iy, a, b) -- a, b float32, zero at invalid sites"""
    flow = np.asarray(flow, dtype=np.float32)
    B, _, H, W = flow.shape
    fx, fy = flow[:, 0], flow[:, 1]
    x2 = (np.arange(W, dtype=np.float32)[None, None, :] + fx).astype(np.float32)
    y2 = (np.arange(H, dtype=np.float32)[None, :, None] + fy).astype(np.float32)
    with np.errstate(invalid="ignore"):
        valid = ((x2 >= 0) & (y2 >= 0) & (x2 <= np.float32(W - 1)) & (y2 <= np.float32(H - 1)) &
                 (np.abs(fx) < np.float32(W) / np.float32(2)) & (np.abs(fy) < np.float32(H) / np.float32(2)))
    x2, y2 = np.where(valid, x2, np.float32(0)), np.where(valid, y2, np.float32(0))
    ix, iy = x2.astype(np.int32), y2.astype(np.int32)
    a, b = (x2 - ix.astype(np.float32)).astype(np.float32), (y2 - iy.astype(np.float32)).astype(np.float32)
    return valid, ix, iy, a, b


def restate(flow, taps, gradoutput, H, W, fs, drop=None, swap_wa=False):
    """(want, n, mass) per image-gradient cell, float64 [B, C, H, W] / int64 [B, 1, H, W] / float64 [B, C, H, W], for inputs
    already widened to what the kernel reads (float32 values).  `drop` = (k, m) leaves that tap's terms out, `drop` =
    "one per cell" leaves out one term of every live cell, and `swap_wa` exchanges wa between m < fs / 2 and m >= fs / 2: the
    wrong operators tests/test_image_grad_bound.py holds the bound against."""
    flow, taps, g = (np.asarray(t, dtype=np.float32) for t in (flow, taps, gradoutput))
    B, C = g.shape[0], g.shape[1]
    assert flow.shape == (B, 2, H, W) and taps.shape == (B, fs * fs, H, W) and g.shape == (B, C, H, W)
    valid, ix, iy, a, b = locate32(flow)
    sel = valid.reshape(-1)
    nz = np.flatnonzero(sel)
    bi = (nz // (H * W)).astype(np.int64)
    ixv, iyv = ix.reshape(-1)[nz].astype(np.int64), iy.reshape(-1)[nz].astype(np.int64)
    av, bv = a.reshape(-1)[nz].astype(np.float64), b.reshape(-1)[nz].astype(np.float64)
    gv = [g[:, c].reshape(-1)[nz].astype(np.float64) for c in range(C)]
    cells = B * H * W
    want, mass = np.zeros((C, cells)), np.zeros((C, cells))
    n = np.zeros(cells, dtype=np.int64)
    lost = np.zeros(cells, dtype=bool)
    half = fs // 2
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(fs):
            row = np.clip(iyv + 1 - half + k, 0, H - 1)
            wb = (1.0 - bv) if k < half else bv
            for m in range(fs):
                if drop == (k, m):
                    continue
                col = np.clip(ixv + 1 - half + m, 0, W - 1)
                left = (m < half) != bool(swap_wa)
                wa = (1.0 - av) if left else av
                coef = wa * wb * taps[:, k * fs + m].reshape(-1)[nz].astype(np.float64)
                idx = bi * (H * W) + row * W + col
                if drop == "one per cell":                              # the first term that reaches a cell is left out
                    cell, first = np.unique(idx, return_index=True)
                    first = first[~lost[cell]]
                    lost[idx[first]] = True
                    keep = np.ones(idx.size, dtype=bool)
                    keep[first] = False
                    idx, coef = idx[keep], coef[keep]
                    sub = [v[keep] for v in gv]
                else:
                    sub = gv
                n += np.bincount(idx, minlength=cells)
                for c in range(C):
                    t = sub[c] * coef
                    want[c] += np.bincount(idx, weights=t, minlength=cells)
                    mass[c] += np.bincount(idx, weights=np.abs(t), minlength=cells)
    shape = (C, B, H, W)
    return (np.ascontiguousarray(want.reshape(shape).transpose(1, 0, 2, 3)), n.reshape(B, 1, H, W),
            np.ascontiguousarray(mass.reshape(shape).transpose(1, 0, 2, 3)))


def exponent_above(v):
    """per batch element: e with (largest finite |v|) < 2^e, shaped [B, 1, 1, 1]; 0 where nothing is finite and non-zero (no
    finite term is then non-zero either)"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    v = np.where(np.isfinite(v), v, 0.0).reshape(v.shape[0], -1).max(axis=1)
    e = np.where(v > 0, np.frexp(v)[1], 0)
    return e.reshape(-1, 1, 1, 1).astype(np.int64)


def block_exponent(taps, gradoutput):
    """e = e_g + e_t of the packed planes' part, [B, 1, 1, 1]"""
    return exponent_above(gradoutput) + exponent_above(taps)


def plane_grid(flow, taps, gradoutput, H, W, tile=(64, 16)):
    """The packed planes' part with the exponent taken per tile instead of per batch element: [B, 1, H, W], the sum over a
    cell's terms of 2^(e_M - 23), where M is the largest site bound s = fl32(largest |gradoutput| x largest |tap|) among the
    valid sites with a finite, non-zero s of the term's 64 x 16 site tile (fi_bwd_c3_body.inc: sbits, pk_tile_publish's
    `use`) and M < 2^e_M.  pk_tile_resolve takes B = min(M, 16 x a robust mean) <= M, so e_tile <= e_M: still an upper
    bound of every tile's block exponent, and never above block_exponent().  Sites without a finite, non-zero s are never
    packed and add nothing here.  (fs == 4, C == 3: the only kernels with planes.)"""
    flow, taps, g = (np.asarray(t, dtype=np.float32) for t in (flow, taps, gradoutput))
    B = g.shape[0]
    tw, th = tile
    valid, ix, iy, _a, _b = locate32(flow)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (np.abs(g).max(axis=1) * np.abs(taps).max(axis=1)).astype(np.float32)
    use = valid & np.isfinite(s) & (s != 0)
    ny, nx = -(-H // th), -(-W // tw)
    pad = np.zeros((B, ny * th, nx * tw), dtype=np.float32)
    pad[:, :H, :W] = np.where(use, s, np.float32(0))
    M = pad.reshape(B, ny, th, nx, tw).max(axis=(2, 4))
    eM = np.frexp(M)[1]
    unit = np.ldexp(1.0, eM - 23)                                       # per tile
    per_site = np.repeat(np.repeat(unit, th, axis=1), tw, axis=2)[:, :H, :W]
    per_site = np.where(use, per_site, 0.0)
    nz = np.flatnonzero(use.reshape(-1))
    bi = (nz // (H * W)).astype(np.int64)
    ixv, iyv = ix.reshape(-1)[nz].astype(np.int64), iy.reshape(-1)[nz].astype(np.int64)
    wt = per_site.reshape(-1)[nz]
    cells = B * H * W
    out = np.zeros(cells)
    for k in range(4):
        row = np.clip(iyv - 1 + k, 0, H - 1)
        for m in range(4):
            col = np.clip(ixv - 1 + m, 0, W - 1)
            out += np.bincount(bi * (H * W) + row * W + col, weights=wt, minlength=cells)
    return out.reshape(B, 1, H, W)


def ulp_T(v, tname):
    """the spacing of T's values in the binade that holds |v| (float64 in, float64 out; subnormals: the smallest spacing)"""
    mant, emin = MANT[tname]
    v = np.abs(np.asarray(v, dtype=np.float64))
    e = np.where(v > 0, np.frexp(v)[1] - 1, emin)
    return np.ldexp(1.0, np.maximum(e, emin) - mant)


def bound(n, mass, e=None, stored=None, want=None, grid=None):
    """The largest |result - want| of a correct kernel, per cell (the module docstring derives every summand).
    e: block_exponent(...) for the kernels that pack the image gradient into LDS planes (the RGB fs == 4 tiled backward in
    its fp32, half and mixed builds); None for kernels without planes (generic filter sizes, the direct kernel, the
    many-channel owner kernels).  grid: plane_grid(...) -- the same part with the exponent taken per tile -- replaces
    n * 2^(e - 23) where given.  stored: "fp16" / "bf16" when the result was rounded once more to that type; needs `want`."""
    n = np.asarray(n, dtype=np.float64)
    planes = e is not None or grid is not None
    flushes = n if planes else 0.0                                      # F
    out = (n + flushes) * K_TERM * U * mass + n * K_TERM * 2.0 ** -126  # fp32 roundings; underflow
    if grid is not None:
        out = out + grid                                                # the planes' fixed-point grid, exponent per tile
    elif e is not None:
        out = out + n * np.ldexp(1.0, np.asarray(e) - 23)               # ... exponent per batch element
    if stored is not None:
        out = out + 0.5 * ulp_T(np.abs(want) + out, stored)
    return out


class Reference:
    """want / n / mass of one call's inputs, made once and shared by every check of that call (never written)."""

    def __init__(self, flow, taps, gradoutput, fs=4, planes=True):
        flow, taps, gradoutput = (_widened(t) for t in (flow, taps, gradoutput))
        B, C, H, W = gradoutput.shape
        self.want, self.n, self.mass = restate(flow, taps, gradoutput, H, W, fs)
        self.e = block_exponent(taps, gradoutput) if planes else None
        self.grid = plane_grid(flow, taps, gradoutput, H, W) if planes else None
        self.live = np.broadcast_to(self.n > 0, self.want.shape)
        self.finite = np.isfinite(self.mass)

    def bound(self, stored=None):
        with np.errstate(invalid="ignore"):
            return bound(self.n, self.mass, self.e, stored, self.want, self.grid)

    def boundary_inside(self, tname, stored=None):
        """cells where a rounding boundary of T (the midpoint of two neighbouring values of T) lies inside want +- bound:
        there two results within the bound may round to different values of T"""
        bd = self.bound(stored)
        with np.errstate(invalid="ignore"):
            lo, hi = _round_T(self.want - bd, tname), _round_T(self.want + bd, tname)
            return ~(lo == hi)

    def ratio(self, got, stored=None):
        """|got - want| / bound over the cells with a finite mass (0 / 0 counts as 0; a result that is not finite there counts
        as infinitely far off), and the mask of the cells that were compared"""
        got = np.asarray(got, dtype=np.float64)
        bd = self.bound(stored)
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.abs(got - self.want)
            r = np.where(err == 0, 0.0, err / bd)
        ok = self.finite & np.isfinite(got)
        return np.where(ok, r, np.where(self.finite, np.inf, 0.0)), ok


def _widened(t):
    if hasattr(t, "detach"):
        t = t.detach().float().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32)


def _round_T(v, tname):
    import torch
    T = {"fp16": torch.float16, "bf16": torch.bfloat16}[tname]
    return torch.from_numpy(np.ascontiguousarray(v)).to(T).double().numpy()
