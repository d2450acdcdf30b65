"""Which in-kernel paths of the tiled fp16 / bf16 warps the case table of tests/_lowp_paths.py reaches -- counted on the
CPU, no GPU needed.  tests/test_gpu_lowp_paths.py runs the same table against the oracle; this module is what says that
those runs sweep vertical and horizontal bands, hit the kMaxBands cap, leave sites to the per-site loop, store lanes in
pieces, meet tiles without a valid site and lanes of mixed validity -- and that the 24 x 160 inputs of
tests/test_gpu_lowp_parity.py cannot.

The conditions are thresholds well inside the counts observed when the table was chosen (fp32 / fp16 / bf16 flow):
    1x96x256 smooth 25    24 tiles, nbx > 1: 9, nby > 1: 19, capped: 1, slow 14 / 14 / 14, split lanes ~1650
    2x64x256 iid 20       32 tiles, all nbx > 1 and nby > 1, up to 6 bands run, slow 0, split lanes ~14 800
    1x112x320 iid 30      35 tiles, capped: 26, slow 5213 / 5214 / 5196
    1x200x320 smooth 40   65 tiles, capped: 31, slow 3421 / 3418 / 3419
    2x100x132 smooth 8    42 tiles, 5 without a valid site, one with nby > 1
    1x40x40 iid 30        3 partial tiles, 216 of 1600 sites valid, ~175 mixed lanes
`pytest -s` prints the counts of this run.
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lowp_paths as LP      # noqa: E402

FLOW_TYPES = ["fp32", "fp16", "bf16"]


def _show(label, c):
    print("%s: %s" % (label, " ".join("%s=%d" % kv for kv in c.items())))


def test_census_constants_are_the_headers():
    """The census restates memc_tile.hpp; a change of the budget, the pitch or the cap there must change it here too."""
    path = os.path.join(LP.ROOT, "memc-net_amd", "csrc", "memc_tile.hpp")
    with open(path) as f:
        text = f.read()

    def one(pattern, what):
        m = re.findall(pattern, text)
        assert len(m) == 1, "memc_tile.hpp: expected exactly one `%s` (%s), found %d" % (pattern, what, len(m))
        return m[0]

    max_bands = int(one(r"constexpr\s+int\s+kMaxBands\s*=\s*(\d+)\s*;", "kMaxBands"))
    assert max_bands == LP.MAX_BANDS, "kMaxBands is %d, the census assumes %d" % (max_bands, LP.MAX_BANDS)
    cap = int(one(r"template\s*<int LX,\s*int CAP\s*=\s*(\d+),\s*int NT\s*=\s*256>\s*struct TileGeom", "TileGeom's default CAP"))
    assert cap == LP.CAP, "TileGeom's default CAP is %d, the census assumes %d" % (cap, LP.CAP)
    band_cap = int(one(r"template\s*<int LX,\s*bool DYN\s*=\s*true,\s*int CAP\s*=\s*(\d+)>\s*__device__ __forceinline__ Bands make_bands",
                       "make_bands' default CAP"))
    assert band_cap == LP.CAP, "make_bands' default CAP is %d, the census assumes %d" % (band_cap, LP.CAP)
    pad = int(one(r"static constexpr int kPitch\s*=\s*kTW\s*\+\s*(\d+)\s*;", "kPitch = kTW + pad"))
    assert LP.TW + pad == LP.PITCH, "kPitch is kTW + %d, the census assumes a pitch of %d" % (pad, LP.PITCH)
    one(r"static constexpr int kTW\s*=\s*4\s*\*\s*LX\s*;", "four sites per lane")
    one(r"d\.sx\s*=\s*\(G::kPitch - 4\)\s*&\s*~3\s*;", "the horizontal band step")
    one(r"d\.sy\s*=\s*rows - 3\s*;", "the vertical band step")
    one(r"d\.n\s*=\s*b\.w == 0 \? 1 : min\(d\.nbx \* d\.nby, kMaxBands\)\s*;", "the band count")
    # the backward's budget (memc_fi_bwd_c3.hpp: PkGeomT<256>::kCap) is the forward's
    with open(os.path.join(LP.ROOT, "memc-net_amd", "csrc", "memc_fi_bwd_c3.hpp")) as f:
        m = re.findall(r"static constexpr int kCap\s*=\s*(\d+)\s*\*\s*NT\s*;", f.read())
    assert len(m) == 1 and int(m[0]) * 256 == LP.CAP, "memc_fi_bwd_c3.hpp: PkGeomT<256>::kCap is not %d: %s" % (LP.CAP, m)
    assert (LP.TW, LP.TH, LP.PITCH, LP.STEP_X, LP.CAP // LP.PITCH) == (64, 16, 96, 92, 32)


# per case: conditions on the census of the flow as generated and rounded to fp16 / bf16
def _cond_smooth25(c):
    assert 1 <= c["slow"] <= 100, c
    assert c["nbx_gt1"] >= 1 and c["nby_gt1"] >= 1, c


def _cond_iid20(c):
    assert c["slow"] == 0, c
    assert c["max_bands_run"] == 6, c
    assert c["split_lanes"] >= 5000, c
    assert c["nbx_gt1"] == c["tiles"] and c["nby_gt1"] == c["tiles"], c


def _cond_iid30(c):
    assert c["slow"] >= 1000, c


def _cond_smooth40(c):
    assert c["slow"] >= 1000, c
    assert c["ragged_rows"] != 0, c


def _cond_ragged_tiles(c):
    assert c["empty"] >= 1, c
    assert c["ragged_rows"] == 4 and c["ragged_cols"] == 4, c


def _cond_mostly_invalid(c):
    assert c["valid"] < 0.25 * c["sites"], c
    assert c["mixed_lanes"] >= 50, c
    assert c["tiles"] == 3, c


CONDITIONS = [_cond_smooth25, _cond_iid20, _cond_iid30, _cond_smooth40, _cond_ragged_tiles, _cond_mostly_invalid]


@pytest.mark.parametrize("ci", range(len(LP.CASES)), ids=LP.CASE_IDS)
def test_table_cases_reach_their_paths(ci):
    case = LP.CASES[ci]
    flow = LP.case_flow(case)
    assert np.array_equal(flow, LP.case_inputs(case, 3)[1])       # the GPU tests' flow is this one
    for ft in FLOW_TYPES:
        c = LP.census(LP.rounded(flow, ft))
        _show("%s flow %s" % (LP.CASE_IDS[ci], ft), c)
        B, H, W = case[:3]
        assert c["tiles"] == B * ((H + 15) // 16) * ((W + 63) // 64)
        CONDITIONS[ci](c)


def test_blend_second_direction_sweeps_bands_too():
    """The blend's second warp (flow drawn from seed + 100) runs its own band loop: more than one band on every blend
    case, and at least one case leaves slow sites to BOTH directions' per-site loops."""
    both = 0
    for ci, case in enumerate(LP.BLEND_CASES):
        slow_everywhere = True
        for ft in FLOW_TYPES:
            c0, c1 = LP.census(LP.rounded(LP.case_flow(case), ft)), LP.census(LP.rounded(LP.case_flow(case, True), ft))
            _show("%s second direction, flow %s" % (LP.CASE_IDS[ci], ft), c1)
            assert c1["max_bands_run"] > 1, (case, ft, c1)
            assert c1["nbx_gt1"] >= 1 and c1["nby_gt1"] >= 1, (case, ft, c1)
            slow_everywhere = slow_everywhere and c0["slow"] >= 1 and c1["slow"] >= 1
        both += slow_everywhere
    assert both >= 1


def test_24x160_inputs_cannot_reach_a_vertical_band_or_the_cap():
    """Why the table is needed: tests/test_gpu_lowp_parity.py runs at H = 24 (or 20), W <= 160.  Whatever the flow, a box
    there is at most 160 x 24 pixels: every pitch leaves >= 32 rows > H (one vertical band), and the width needs at most
    two bands -- below the cap, so no site is ever left to the per-site loop."""
    for bw_ in range(4, 161, 4):
        for bh_ in range(1, 25):
            nbx, nby, bw, bh, sy = LP.make_bands(bw_, bh_)
            assert nby == 1 and nbx <= 2 and nbx * nby < LP.MAX_BANDS
    # and the census of that module's most violent flow agrees
    import torch      # noqa: F401  (rounded())
    rng = np.random.default_rng(14)
    for kind, sigma in (("smooth", None), ("iid", None), ("iid", 0.6 * 160)):
        flow = LP.synth.np_flow(rng, 2, 24, 160, kind, sigma)
        for ft in FLOW_TYPES:
            c = LP.census(LP.rounded(flow, ft))
            assert c["nby_gt1"] == 0 and c["capped"] == 0 and c["slow"] == 0 and c["max_bands_run"] <= 2, c
