"""The premises of tests/test_gpu_lp_dproj_grad.py, proved without a GPU (the cases: tests/_lp_dproj_cases.py).

  * every exact case handed to the half kernel holds numbers of T only -- flow, depth and gradoutput convert to T and back
    unchanged, the count and the forward output are float32 by contract -- and stays exact in fp32: the float32 oracle and
    the same source built in double (oracle/memc_oracle64) return the same three gradient planes, per case and per dtype,
    and the sums of absolute terms stay below 2^24 quanta (tests/_exact.proj_bwd_budget: whatever the order of the sum).
    Where _exact.proj_bwd_inputs' own flow is NOT a number of T the case is the restated one (the flow clipped to T's range
    on the quarter grid, _lp_dproj_cases.exact_inputs); which (case, T) pairs those are is pinned below;
  * the census of the kernel's branches (tests/_lowp_paths.proj_bwd_census, which tests/test_exact_inputs.py holds to the
    text of the fp32 kernel that the half kernel restates): the exact cases reach the gather from global memory, boxes
    clipped in x and in y, a case in which every site is served from LDS, invalid sites and tiles without a valid site;
    the random 1x2x40x136 case has hundreds of sites on the global gather;
  * the random cases' expected gradients are not vacuous under the absolute rule: max |want| >= 100 x ATOL, both planes;
  * the one ordinary case held to the oracle (2x2x20x72): the float32 oracle's gradinput2 -- a sum of eight signed terms
    that can cancel (tests/_parity.py) -- lies within _parity's bound of the float64 oracle's, so the reference alone passes
    tests/_netcalls.rule_rounded there.
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

import _exact as E             # noqa: E402
import _lowp_paths as LP       # noqa: E402
import _lp_dproj_cases as C    # noqa: E402
from _parity import ATOL, BIG, RTOL      # noqa: E402

# the (case, T) pairs whose tabled flow T cannot hold: restated on the clipped flow
RESTATED = {"fp16": ["1x20x1280-far"],
            "bf16": ["2x64x256-iid20", "1x112x320-iid30", "1x200x320-smooth40", "1x40x40-iid30", "1x20x1280-far"]}


@pytest.fixture(scope="module")
def oracle64():
    from oracle import memc_oracle64
    memc_oracle64.build()
    memc_oracle64.lib()
    return memc_oracle64


def test_the_case_lists_split_pb_ids_by_the_kernel_s_width_rule():
    assert sorted(C.COVERED + C.DECLINED) == sorted(E.PB_IDS) and not set(C.COVERED) & set(C.DECLINED)
    assert len(C.COVERED) == 9 and len(C.DECLINED) == 8
    widths = {n: E.pb_flow(n).shape[3] for n in E.PB_IDS}
    assert all(C.covered_width(widths[n]) for n in C.COVERED) and not any(C.covered_width(widths[n]) for n in C.DECLINED)
    assert 8 in [widths[n] for n in C.COVERED]                                                     # the minimum width


@pytest.mark.parametrize("tname", C.TNAMES)
def test_which_exact_cases_are_restated_on_a_clipped_flow(tname):
    got = [n for n in C.COVERED if C.exact_inputs(n, tname) is not E.proj_bwd_inputs(n, True)]
    assert got == RESTATED[tname], got
    for n in got:                                      # restated because the tabled flow is no number of T, and only then
        assert not C.is_number_of(E.proj_bwd_inputs(n, True)["flow"], tname)
        assert float(np.abs(C.exact_inputs(n, tname)["flow"]).max()) == E.CLIP[tname]


_PROVED = {}


@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("name", C.COVERED)
def test_exact_cases_hold_numbers_of_t_and_stay_exact(oracle, oracle64, name, tname):
    h = C.exact_inputs(name, tname)
    for k in ("flow", "depth", "gout"):
        assert h[k].dtype == np.float32 and C.is_number_of(h[k], tname), "%s %s: %s is not a number of %s" % (name, tname, k, tname)
    B, _, H, W = h["flow"].shape
    assert h["depth"].shape == (B, 1, H, W) and h["count"].shape == (B, 1, H, W) and h["fwd_out"].shape == (B, 2, H, W)
    assert h["count"].dtype == np.float32 and h["fwd_out"].dtype == np.float32
    # synthetic counts: +-2^e (e = -2 .. 4) exactly where the scatter of THIS flow puts anything, exactly 0 elsewhere
    hit = E.project_sums(h["flow"])[1] > 0
    assert np.array_equal(h["count"] != 0, hit)
    assert set(np.unique(np.abs(h["count"]))) <= {0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0}
    assert (h["count"][hit] > 0).any() and (h["count"][hit] < 0).any()
    assert (~hit).any(), "no cell of count 0: a wrong read could not show as inf or NaN"
    assert set(np.unique(h["depth"] * 8)) <= set(float(k) for k in range(1, 10))                   # k / 8
    assert np.array_equal(h["fwd_out"] * 4, np.round(h["fwd_out"] * 4)) and np.abs(h["fwd_out"]).max() <= 64
    if id(h) in _PROVED:                               # the same arrays for both dtypes: proved once
        return
    m = E.proj_bwd_budget(h)                           # asserts that no valid site reads a count of zero
    print("%s %s: budget %s" % (name, tname, m))
    assert E.holds(m), (name, tname, m)
    a = (h["flow"], h["depth"], h["count"], h["fwd_out"], h["gout"])
    got32, got64 = oracle.depth_flow_projection_backward(*a), oracle64.depth_flow_projection_backward(*a)
    for g32, g64, n, key in zip(got32, got64, ("gradinput1", "gradinput2"), ("dpb_g1", "dpb_g2")):
        assert g32.dtype == np.float32 and g64.dtype == np.float64 and np.isfinite(g64).all(), (name, n)
        assert np.array_equal(g32.astype(np.float64), g64), "%s %s %s: the fp32 oracle rounded somewhere" % (name, tname, n)
        assert np.abs(g64).max() <= m[key], (name, n, m)
    _PROVED[id(h)] = True


@pytest.mark.parametrize("tname", C.TNAMES)
def test_the_exact_cases_reach_every_branch_of_the_kernel(tname):
    census = {n: LP.proj_bwd_census(C.exact_inputs(n, tname)["flow"])[0] for n in C.COVERED}
    for n, c in census.items():
        assert c["route"] == "tiled" and c["ws"] == E.pb_flow(n).shape[3] and c["tail_valid"] == 0, (n, c)
        print(tname, n, {k: c[k] for k in ("sites", "valid", "tiles", "empty", "clip_x", "clip_y", "uncovered")})
    assert any(c["uncovered"] > 0 for c in census.values())                    # the gather from global memory
    assert any(c["clip_x"] > 0 for c in census.values())
    assert any(c["clip_y"] > 0 for c in census.values())
    assert any(c["uncovered"] == 0 and c["valid"] > 0 for c in census.values())     # every site from LDS
    assert any(c["empty"] > 0 for c in census.values())                        # tiles without a valid site: zeros stored
    assert all(c["valid"] < c["sites"] for c in census.values())               # invalid sites in every case
    assert sum(c["uncovered"] for c in census.values()) > 50000


@pytest.mark.parametrize("tname", C.TNAMES)
def test_declined_cases_are_well_formed(tname):
    for n in C.DECLINED:
        h = E.proj_bwd_inputs(n, True)
        assert all(C.is_number_of(h[k], tname) for k in ("flow", "depth", "gout")), n
        assert not C.covered_width(h["flow"].shape[3])


def _ordinary(oracle, case, tname):
    flow, depth, gout = C.random_inputs(case, tname)
    out, count = oracle.depth_flow_projection_forward(flow, depth, 0)
    return flow, depth, count, out, gout


@pytest.mark.parametrize("tname", C.TNAMES)
def test_random_cases_reach_what_they_are_for_and_are_not_vacuous(oracle, tname):
    """1x2x8x8: one partial tile; 2x2x20x72: four tiles per image, partial in both directions; 1x2x40x136: hundreds of valid
    sites whose corners lie outside their tile's staged box, boxes clipped in y"""
    seen = {}
    for case, cid in zip(C.RANDOM, C.RANDOM_IDS):
        a = _ordinary(oracle, case, tname)
        flow, depth = a[0], a[1]
        assert all(C.is_number_of(t, tname) for t in (flow, depth, a[4]))
        assert 0.09 < float(depth.min()) and float(depth.max()) < 1.11
        c = LP.proj_bwd_census(flow)[0]
        seen[cid] = c
        assert c["route"] == "tiled" and c["valid"] > 0 and c["tail_valid"] == 0, c
        for want, n in zip(oracle.depth_flow_projection_backward(*a), ("gradinput1", "gradinput2")):
            top = float(np.abs(want[np.isfinite(want)]).max())
            print(tname, cid, n, {k: c[k] for k in ("valid", "tiles", "clip_x", "clip_y", "uncovered")}, "max |want| %.4g" % top)
            assert np.isfinite(want).all() and top >= 100 * ATOL, (cid, n, top)
    assert seen["1x2x8x8"]["tiles"] == 1 and seen["2x2x20x72"]["tiles"] == 8 and seen["1x2x40x136"]["tiles"] == 9
    assert seen["1x2x40x136"]["uncovered"] >= 500 and seen["1x2x40x136"]["clip_y"] >= 1
    assert seen["2x2x20x72"]["uncovered"] == 0


@pytest.mark.parametrize("tname", C.TNAMES)
def test_the_reference_alone_passes_the_rule_on_the_ordinary_case(oracle, oracle64, tname):
    """gradinput2 of the float32 oracle against the float64 oracle's on the 2x2x20x72 case, both gradients for good measure:
    within _parity's bound (ATOL up to |want| = 10, max(ATOL, RTOL * |want|) beyond), the bound tests/_netcalls.rule_rounded
    widens by half an ulp of T"""
    a = _ordinary(oracle, C.ORDINARY, tname)
    for g32, g64, n in zip(oracle.depth_flow_projection_backward(*a), oracle64.depth_flow_projection_backward(*a),
                           ("gradinput1", "gradinput2")):
        aw = np.abs(g64)
        bound = np.where(aw <= BIG, ATOL, np.maximum(ATOL, RTOL * aw))
        err = np.abs(g32.astype(np.float64) - g64)
        print(tname, n, "max err %.3g, max |want| %.4g, worst err / bound %.3g" % (err.max(), aw.max(), (err / bound).max()))
        assert (err <= bound).all(), (tname, n, float((err / bound).max()))
