"""The premises of tests/test_gpu_lp_bilinear.py, proved without a GPU (the cases: tests/_lp_bl_cases.py).

  * every exact case handed to the half kernels holds numbers of T only (image, flow, gradoutput convert to T and back
    unchanged; the flow is the tabled one clipped by _exact.CLIP), stays exact in fp32 in any order
    (_exact.bilinear_budget / _exact.holds) and a float64 build of the oracle returns the same numbers;
  * the census of the tiled kernels' staged boxes (_lp_bl_cases.census, whose constants are read out of the sources' text:
    the budgets 2496 / 3072 / 4096 and the tile heights 16 / 32): the i.i.d. cases put hundreds of valid sites outside
    their tile's box -- the corners gathered from global memory, the per-site atomics of the backward -- and the smooth
    cases none.  These are conditions on the inputs: if a seed misses one, the seed changes, not the condition;
  * the random cases' expectations are not vacuous under the absolute rule.
"""
import os
import sys

import numpy as np
import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
for _p in (ROOT, _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _exact as E            # noqa: E402
import _lp_bl_cases as C      # noqa: E402
from _parity import ATOL      # noqa: E402


@pytest.fixture(scope="module")
def oracle64():
    from oracle import memc_oracle64
    memc_oracle64.build()
    memc_oracle64.lib()
    return memc_oracle64


def test_the_constants_of_the_sources():
    k = C.source_constants()
    assert (k["cap_c3"], k["cap_chunks"], k["cap_bwd"]) == (2496, 3072, 4096), k
    assert (k["nt_fwd"], k["nt_bwd"], k["th_fwd"], k["th_bwd"]) == (256, 512, 16, 32), k
    # what the restated box formula assumes of memc_tile.hpp beyond the expressions source_constants() matched
    assert (C.LP.LX, C.LP.TW, C.LP.PITCH) == (16, 64, 96)


def test_the_exact_cases_are_the_tabled_ones():
    """bilinear_rgb_cases() is table cases 0, 2, 5 in fp32 storage: the same images and gradoutputs here, the flow clipped"""
    want = list(E.bilinear_rgb_cases())
    assert [w[0] for w in want] == C.EXACT_IDS
    for tname in C.TNAMES:
        for (name, x, flow, gout) in want:
            hx, hflow, hgout = C.exact_inputs(name, tname)
            assert np.array_equal(hx, x) and np.array_equal(hgout, gout)
            assert np.array_equal(hflow, np.clip(flow, -E.CLIP[tname], E.CLIP[tname]))
        assert C.exact_inputs(C.EXACT_C8, tname)[0].shape[1] == 8
        assert np.array_equal(C.exact_inputs(C.EXACT_C8, tname)[1], C.exact_inputs(C.EXACT_IDS[0], tname)[1])


@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("name", C.EXACT_IDS + [C.EXACT_C8])
def test_exact_cases_hold_numbers_of_t_and_stay_exact(oracle, oracle64, name, tname):
    x, flow, gout = C.exact_inputs(name, tname)
    for k, a in (("image", x), ("flow", flow), ("gradoutput", gout)):
        assert a.dtype == np.float32 and C.is_number_of(a, tname), "%s %s: %s is not a number of %s" % (name, tname, k, tname)
    assert float(np.abs(flow).max()) <= E.CLIP[tname]
    m = E.bilinear_budget(oracle64, x, flow, gout)
    print(name, tname, m)
    assert E.holds(m), (name, tname, m)
    # nothing rounded anywhere in the fp32 oracle
    f32, f64 = oracle.interpolation_ch_forward(x, flow), oracle64.interpolation_ch_forward(x, flow)
    assert np.array_equal(f32.astype(np.float64), f64)
    for a, b in zip(oracle.interpolation_ch_backward(x, flow, gout), oracle64.interpolation_ch_backward(x, flow, gout)):
        assert np.array_equal(np.asarray(a).astype(np.float64), b)
    assert np.abs(oracle64.interpolation_ch_backward(x, flow, gout)[1]).max() <= m["bl_flow"]
    # every result is a number of fp32 that T rounds once: the image gradient is compared in fp32
    assert np.isfinite(f32).all() and float(np.abs(f32).max()) > 0


@pytest.mark.parametrize("tname", C.TNAMES)
def test_the_census_of_the_random_cases(tname):
    """computed here with the restatement, under the bilinear warp's own validity test (x2 < W; the projection's x2 <= W - 1
    gives 3796 valid sites and 589 / 591 uncovered ones): 1x40x136 has 3881 (fp16) / 3880 (bf16) valid sites of 5440 and,
    of those, 621 / 618 outside their tile's box at CAP 2496 and 263 at CAP 3072; 1x72x136 has 1347 / 1348 on the
    backward's 64 x 32 tiles at CAP 4096; the smooth cases none"""
    k = C.source_constants()
    for case, cid in zip(C.SMOOTH, C.RANDOM_IDS[:2]):
        flow = C.random_flow(case, tname)
        assert C.is_number_of(flow, tname)
        for cap, th in ((k["cap_c3"], k["th_fwd"]), (k["cap_chunks"], k["th_fwd"]), (k["cap_bwd"], k["th_bwd"])):
            c = C.census(flow, cap, th)
            print(tname, cid, cap, th, c)
            assert c["uncovered"] == 0 and c["valid"] > 0, (cid, cap, c)
    assert C.census(C.random_flow(C.SMOOTH[0], tname), k["cap_c3"], k["th_fwd"])["tiles"] == 1
    assert C.census(C.random_flow(C.SMOOTH[1], tname), k["cap_c3"], k["th_fwd"])["tiles"] == 8     # 2 x 2 per image
    flow = C.random_flow(C.IID_FWD, tname)
    c3, chunks = C.census(flow, k["cap_c3"], k["th_fwd"]), C.census(flow, k["cap_chunks"], k["th_fwd"])
    print(tname, "1x40x136", c3, chunks)
    assert c3["uncovered"] >= 200 and chunks["uncovered"] >= 100, (c3, chunks)
    assert c3["clip_x"] >= 1 and c3["clip_y"] >= 1, c3
    assert 0 < c3["valid"] < c3["sites"] == 5440
    bwd = C.census(C.random_flow(C.IID_BWD, tname), k["cap_bwd"], k["th_bwd"])
    print(tname, "1x72x136", bwd)
    assert bwd["uncovered"] >= 500 and bwd["clip_y"] >= 1, bwd
    assert bwd["tiles"] == 9                                                                   # 3 x 3 tiles of 64 x 32


@pytest.mark.parametrize("tname", C.TNAMES)
def test_random_cases_are_not_vacuous(oracle, tname):
    for case, cid in zip(C.RANDOM, C.RANDOM_IDS):
        x, flow, gout = C.random_inputs(case, 3, tname)
        assert all(C.is_number_of(a, tname) for a in (x, flow, gout))
        assert np.array_equal(flow, C.random_flow(case, tname))
        fwd = oracle.interpolation_forward(x, flow)
        g1, g2 = oracle.interpolation_backward(x, flow, gout)
        for what, a in (("forward", fwd), ("image gradient", g1), ("flow gradient", g2)):
            top = float(np.abs(a).max())
            assert np.isfinite(a).all() and top >= 100 * ATOL, (cid, what, top)
