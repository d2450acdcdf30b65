"""The premises of the SPyNet level backward tests (tests/_spynet_grad_spec.py), on the CPU:

  * `level_grad` in float64 is torch's float64 autograd through `SpyNetLevelLayer._composed` (to 1e-9 of the largest
    gradient) on every admissible ordinary case and the pan.  The zero flow under align_sample = 1 puts every site ON an
    integer position, where the derivative is one-sided: the rule's position is x exactly and takes the right-hand one,
    the composed route's normalise / un-normalise round trip lands a rounding error to either side of x and takes
    whichever -- no statement of the rule can agree with it there (measured: 7.3 against a largest gradient of 8.0 at
    2 x 24 x 40).  So that flow is held to torch at a uniform flow of 2^-10 px beside it (admissible: every position is
    2^-10 from its integer, the same corners as at zero), and at exactly zero to the right-hand differences written out;
  * the exact cases are exact: every `up` is a multiple of 1/8, every term of gu a multiple of 1/128, every term of the
    doubled adjoint a multiple of 1/1024, and every sum of absolute terms stays below 2^24 quanta -- so any order of
    summation, contracted or not, gives the same bits;
  * `footprint` covers every fine index of nonzero weight and a tile's staged box stays within `box_bound` <= BOX, for
    every coarse size from 1 to 1024, both upsampling modes and both parities; the constants are the source's.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd"), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _spynet_spec as S                   # noqa: E402
import _spynet_grad_spec as SG             # noqa: E402


def torch_grad(second, coarse, G, flags):
    from my_package.functions.SpyNetLevelLayer import _composed
    s, g = torch.from_numpy(second.copy()).double(), torch.from_numpy(G.copy()).double()
    c = torch.from_numpy(coarse.copy()).double().requires_grad_(True)
    out = _composed(torch.zeros_like(s), s, c, bool(flags[0]), bool(flags[1]))
    return torch.autograd.grad(out, c, g)[0].numpy()


@pytest.mark.parametrize("flags", SG.FLAGS)
@pytest.mark.parametrize("shape", SG.SHAPES)
def test_rule_is_torch_float64_autograd(shape, flags):
    for flow in SG.flows(flags):
        second, coarse, G, attempt = SG.ordinary_case(shape, flags, flow)
        if flow == "zero":
            check_zero_flow(second, coarse, G, flags)
            coarse = np.full_like(coarse, 2.0 ** -11)      # up = 2^-10 everywhere: beside zero, off the integers
            assert SG.admissible(S.upsampled(coarse, shape[1], shape[2], flags[0], np.float64), flags[1])
        got = SG.level_grad(second, coarse, G, flags, np.float64)
        want = torch_grad(second, coarse, G, flags)
        assert got.shape == want.shape == coarse.shape
        scale = float(np.abs(want).max())
        err = float(np.abs(got - want).max())
        print(shape, flags, flow, "attempt", attempt, "max |want| %.3g, max error %.3g" % (scale, err))
        assert scale > 0 and err <= 1e-9 * scale, (shape, flags, flow, err, scale)
        if flow == "pan":                      # every warp term is 0: the pure adjoint of the upsampling of G[6:8]
            h, w = coarse.shape[2:]
            assert np.array_equal(got, SG.upsample_adjoint(G[:, 6:8].astype(np.float64), h, w, flags[0], np.float64))


def check_zero_flow(second, coarse, G, flags):
    """at zero flow under align_sample = 1: floor(px) = x, ax = 0, bx = 1 -- the right-hand differences of `second`, the
    neighbour beyond the last column or row counting as 0"""
    assert flags[1] and not coarse.any()
    s, g = second.astype(np.float64), G.astype(np.float64)
    right = np.concatenate([s[..., 1:], np.zeros_like(s[..., :1])], axis=3) - s
    down = np.concatenate([s[:, :, 1:], np.zeros_like(s[:, :, :1])], axis=2) - s
    gu = np.stack([g[:, 6] + (g[:, 3:6] * right).sum(axis=1), g[:, 7] + (g[:, 3:6] * down).sum(axis=1)], axis=1)
    h, w = coarse.shape[2:]
    want = SG.upsample_adjoint(gu, h, w, flags[0], np.float64)
    got = SG.level_grad(second, coarse, G, flags, np.float64)
    assert float(np.abs(got - want).max()) <= 1e-12 * float(np.abs(want).max())


def test_admissible_draws_exist_and_the_test_bites():
    """the builder's attempts are recorded; a flow that puts a site on an integer position is refused"""
    taken = [SG.ordinary_case(shape, flags)[3] for shape in SG.SHAPES for flags in SG.FLAGS]
    print("attempts taken:", taken)
    assert all(t is not None and t < SG.ATTEMPTS for t in taken)
    up = np.zeros((1, 2, 6, 5), np.float32)
    assert not SG.admissible(up, 1)            # every position an integer
    up[:] = 0.5
    assert SG.admissible(up, 1)
    up[0, 0, 2, 2] = 1.0 - 2.0 ** -15
    assert not SG.admissible(up, 1)
    up[0, 0, 2, 2] = 1e9                       # clamped outside: no corner inside, its integer position does not count
    assert SG.admissible(up, 1)


@pytest.mark.parametrize("shape", SG.SHAPES)
def test_exact_cases_are_exact(shape):
    second, coarse, G = SG.exact_case(shape)
    B, H, W = shape
    h, w = coarse.shape[2:]
    au, asmp = SG.EXACT_FLAGS
    up = S.upsampled(coarse, H, W, au, np.float64)
    assert np.array_equal(up * 8, np.rint(up * 8))
    assert np.array_equal(up, S.upsampled(coarse, H, W, au, np.float32).astype(np.float64))
    # the terms of gu: |G[3 + c]| * (by |ne - nw| + ay |se - sw|), each product a multiple of 1/128
    s, g = second.astype(np.float64), G.astype(np.float64)
    ix, iy, inx, iny, _w = S.corners(up, asmp, np.float64)
    px = S._position(np.arange(W)[None, None, :], up[:, 0], W, asmp, np.float64)
    py = S._position(np.arange(H)[None, :, None], up[:, 1], H, asmp, np.float64)
    ax, ay = px - np.floor(px), py - np.floor(py)
    bidx = np.arange(B)[:, None, None]
    absx, absy = np.abs(g[:, 6]), np.abs(g[:, 7])
    for c in range(3):
        v = [[np.where(inx[dx] & iny[dy], s[bidx, c, np.clip(iy + dy, 0, H - 1), np.clip(ix + dx, 0, W - 1)], 0.0)
              for dx in (0, 1)] for dy in (0, 1)]
        for term in ((1 - ay) * (v[0][1] - v[0][0]), ay * (v[1][1] - v[1][0]), (1 - ax) * (v[1][0] - v[0][0]),
                     ax * (v[1][1] - v[0][1])):
            assert np.array_equal(term * 128, np.rint(term * 128))
        absx = absx + np.abs(g[:, 3 + c]) * ((1 - ay) * np.abs(v[0][1] - v[0][0]) + ay * np.abs(v[1][1] - v[1][0]))
        absy = absy + np.abs(g[:, 3 + c]) * ((1 - ax) * np.abs(v[1][0] - v[0][0]) + ax * np.abs(v[1][1] - v[0][1]))
    assert float(max(absx.max(), absy.max())) * 128 < 2 ** 24
    gu = SG.site_grad(second, up, G, asmp, np.float64)
    assert np.array_equal(gu * 128, np.rint(gu * 128))
    assert np.array_equal(gu, SG.site_grad(second, up, G, asmp, np.float32).astype(np.float64))
    # the adjoint: weights are multiples of 1/4, wy * wx * gu of 1/2048, doubled of 1/1024
    my, mx = SG.adjoint_matrix(h, H, au, np.float64), SG.adjoint_matrix(w, W, au, np.float64)
    assert np.array_equal(my * 4, np.rint(my * 4)) and np.array_equal(mx * 4, np.rint(mx * 4))
    want = SG.level_grad(second, coarse, G, SG.EXACT_FLAGS, np.float64)
    assert np.array_equal(want * 1024, np.rint(want * 1024))
    sum_abs = 2.0 * np.einsum("yi,bcyx,xj->bcij", my, np.stack([absx, absy], 1), mx)
    print(shape, "largest sum of absolute terms: %.0f quanta of 1/1024" % (float(sum_abs.max()) * 1024))
    assert float(sum_abs.max()) * 1024 < 2 ** 24
    assert np.array_equal(want, SG.level_grad(second, coarse, G, SG.EXACT_FLAGS, np.float32).astype(np.float64))
    assert float(np.abs(want).max()) > 0


def test_footprint_covers_every_weight_and_the_box_stays_within_its_bound():
    worst = {0: 0, 1: 0}
    for align in (0, 1):
        for n in range(1, 1025):
            for N in (2 * n, 2 * n + 1):
                if N < 2:
                    continue
                # the kernel's own fp32 indices and weights: the (fine index, cell) pairs of nonzero weight
                i0, i1, l0, l1 = S.up_index(np.minimum(np.arange(N), 2 * n - 1), n, align, np.float32)
                ys = np.concatenate([np.arange(N)[l0 != 0], np.arange(N)[l1 != 0]])
                cells = np.concatenate([i0[l0 != 0], i1[l1 != 0]])
                assert len(ys) >= N
                lo, hi = SG.footprint(np.arange(n), n, N, align)
                assert (lo[0], hi[0]) == SG.footprint(0, n, N, align) and (lo[-1], hi[-1]) == SG.footprint(n - 1, n, N, align)
                assert (lo >= 0).all() and (hi <= N - 1).all() and (lo <= hi).all(), (align, n, N)
                assert ((lo[cells] <= ys) & (ys <= hi[cells])).all(), (align, n, N)
                bound = SG.box_bound(n, N, align)
                assert bound <= SG.BOX, (align, n, N, bound)
                for t0 in range(0, n, SG.TILE):
                    t1 = min(t0 + SG.TILE, n)
                    a, b = SG.footprint(t0, n, N, align, t1)
                    assert b - a + 1 <= bound, (align, n, N, t0, a, b, bound)
                    assert a <= lo[t0:t1].min() and hi[t0:t1].max() <= b, (align, n, N, t0)   # a cell's range lies in its tile's
                    worst[align] = max(worst[align], b - a + 1)
    print("largest staged box side: %d without align_upsample, %d under it; bound %d" % (worst[0], worst[1], SG.BOX))
    assert worst[0] == 2 * SG.TILE + 2 and worst[1] <= SG.BOX


def test_constants_are_the_source_s():
    text = open(os.path.join(ROOT, "memc-net_amd", "csrc", "spynet_level_bwd.hip")).read()
    assert int(re.search(r"constexpr int kTile = (\d+);", text).group(1)) == SG.TILE
    assert re.search(r"constexpr int kBox = 2 \* kTile \+ 7;", text) and SG.BOX == 2 * SG.TILE + 7
    assert "if (n <= kTile) return N;" in text and "if (!align) return 2 * kTile + 2;" in text
    assert "return 2 * kTile + 4 + (kTile + 1 + n - 2) / (n - 1) + (N - 2 * n);" in text
    assert "a = i0 >= 1 ? (int)(((i0 - 1) * num) / den) : 0;" in text and "(i1 * num + den - 1) / den" in text
    assert "__shared__ float gu[2][kBox * kPitch];" in text
