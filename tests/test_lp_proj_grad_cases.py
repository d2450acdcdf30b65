"""The premises of tests/test_gpu_lp_proj_grad.py, proved without a GPU (the cases: tests/_lp_proj_cases.py).

  * every exact case handed to the half kernel holds numbers of T only -- flow and gradoutput convert to T and back
    unchanged, the count is float32 by contract -- and stays exact in fp32 (tests/_exact.proj_bwd_budget: no valid site
    reads a count of zero, every sum below 2^24 quanta).  Where _exact.proj_bwd_inputs' own flow is NOT a number of T the
    case is the restated one (the flow clipped to T's range on the quarter grid, _lp_proj_cases.exact_inputs); which
    (case, T) pairs those are is pinned below, so that a change to the tables shows;
  * the census of the kernel's branches (tests/_lowp_paths.proj_bwd_census, which tests/test_exact_inputs.py holds to the
    text of the fp32 kernel that the half kernel restates): the exact cases reach the gather from global memory, boxes
    clipped in x and in y, and a case in which every site is served from LDS; the random 1x2x40x136 case has hundreds of
    sites on the global gather;
  * the random cases' expected gradients are not vacuous under the absolute rule: max |want| >= 100 x ATOL.
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
import _lowp_paths as LP      # noqa: E402
import _lp_proj_cases as C    # noqa: E402
from _parity import ATOL      # noqa: E402

# the (case, T) pairs whose tabled flow T cannot hold: restated on the clipped flow
RESTATED = {"fp16": ["1x20x1280-far"],
            "bf16": ["2x64x256-iid20", "1x112x320-iid30", "1x200x320-smooth40", "1x40x40-iid30", "1x20x1280-far"]}


def test_the_case_lists_split_pb_ids_by_the_kernel_s_width_rule():
    assert sorted(C.COVERED + C.DECLINED) == sorted(E.PB_IDS) and not set(C.COVERED) & set(C.DECLINED)
    assert len(C.COVERED) == 9 and len(C.DECLINED) == 8
    widths = {n: E.pb_flow(n).shape[3] for n in E.PB_IDS}
    assert all(widths[n] % 4 == 0 and widths[n] >= 8 for n in C.COVERED), widths
    assert any(widths[n] == 4 for n in C.DECLINED) and any(widths[n] < 4 for n in C.DECLINED)      # narrow
    assert any(widths[n] % 4 and widths[n] > 8 for n in C.DECLINED)                                # ragged
    assert 8 in [widths[n] for n in C.COVERED]                                                     # the minimum width


@pytest.mark.parametrize("tname", C.TNAMES)
def test_which_exact_cases_are_restated_on_a_clipped_flow(tname):
    got = [n for n in C.COVERED if C.exact_inputs(n, tname) is not E.proj_bwd_inputs(n, False)]
    assert got == RESTATED[tname], got
    for n in got:                                      # restated because the tabled flow is no number of T, and only then
        assert not C.is_number_of(E.proj_bwd_inputs(n, False)["flow"], tname)
        assert float(np.abs(C.exact_inputs(n, tname)["flow"]).max()) == E.CLIP[tname]


@pytest.mark.parametrize("tname", C.TNAMES)
@pytest.mark.parametrize("name", C.COVERED)
def test_exact_cases_hold_numbers_of_t_and_stay_exact(name, tname):
    h = C.exact_inputs(name, tname)
    for k in ("flow", "gout"):
        assert h[k].dtype == np.float32 and C.is_number_of(h[k], tname), "%s %s: %s is not a number of %s" % (name, tname, k, tname)
    assert h["count"].dtype == np.float32 and h["count"].shape == (h["flow"].shape[0], 1) + h["flow"].shape[2:]
    # synthetic counts: 2^e (e = 0 .. 4) exactly where the scatter of THIS flow puts anything, exactly 0 elsewhere
    hit = E.project_sums(h["flow"])[1] > 0
    assert np.array_equal(h["count"] > 0, hit) and set(np.unique(h["count"])) <= {0.0, 1.0, 2.0, 4.0, 8.0, 16.0}
    assert (~hit).any(), "no cell of count 0: a wrong read could not show as inf or NaN"
    m = E.proj_bwd_budget(h)                           # asserts that no valid site reads a count of zero
    assert m["pb_quot"] * 2.0 ** E.Q["pb_quot"] < E.LIMIT and m["pb_g1"] * 2.0 ** E.Q["pb_g1"] < E.LIMIT, m
    # the gradient is a multiple of 2^-4 below 64: an fp32 number whatever the order; T rounds it once
    assert m["pb_g1"] <= 4 * E.G


@pytest.mark.parametrize("tname", C.TNAMES)
def test_the_exact_cases_reach_every_branch_of_the_kernel(tname):
    census = {n: LP.proj_bwd_census(C.exact_inputs(n, tname)["flow"])[0] for n in C.COVERED}
    for n, c in census.items():
        assert c["route"] == "tiled" and c["ws"] == E.pb_flow(n).shape[3] and c["tail_valid"] == 0, (n, c)
        print(tname, n, {k: c[k] for k in ("valid", "tiles", "empty", "clip_x", "clip_y", "uncovered")})
    assert any(c["uncovered"] > 0 for c in census.values())                    # the gather from global memory
    assert any(c["clip_x"] > 0 for c in census.values())
    assert any(c["clip_y"] > 0 for c in census.values())
    assert any(c["uncovered"] == 0 and c["valid"] > 0 for c in census.values())     # every site from LDS
    assert any(c["empty"] > 0 for c in census.values())                        # tiles without a valid site: zeros stored
    assert sum(c["uncovered"] for c in census.values()) > 50000


@pytest.mark.parametrize("tname", C.TNAMES)
def test_declined_cases_are_well_formed(tname):
    for n in C.DECLINED:
        h = E.proj_bwd_inputs(n, False)
        assert C.is_number_of(h["flow"], tname) and C.is_number_of(h["gout"], tname), n


@pytest.mark.parametrize("tname", C.TNAMES)
def test_random_cases_reach_what_they_are_for_and_are_not_vacuous(oracle, tname):
    """1x2x8x8: one partial tile; 2x2x20x72: four tiles per image, partial in both directions; 1x2x40x136: 589 (fp16) / 591
    (bf16) valid sites whose corners lie outside their tile's staged box, boxes clipped in y in six tiles of nine"""
    seen = {}
    for case, cid in zip(C.RANDOM, C.RANDOM_IDS):
        flow, gout = C.random_inputs(case, tname)
        assert C.is_number_of(flow, tname) and C.is_number_of(gout, tname)
        c = LP.proj_bwd_census(flow)[0]
        seen[cid] = c
        assert c["route"] == "tiled" and c["valid"] > 0 and c["tail_valid"] == 0, c
        count = oracle.flow_projection_forward(flow, 0)[1]
        want = oracle.flow_projection_backward(flow, count, gout)
        top = float(np.abs(want[np.isfinite(want)]).max())
        print(tname, cid, {k: c[k] for k in ("valid", "tiles", "clip_x", "clip_y", "uncovered")}, "max |want| %.4g" % top)
        assert np.isfinite(want).all() and top >= 100 * ATOL, (cid, top)
    assert seen["1x2x8x8"]["tiles"] == 1 and seen["2x2x20x72"]["tiles"] == 8 and seen["1x2x40x136"]["tiles"] == 9
    assert seen["1x2x40x136"]["uncovered"] >= 500 and seen["1x2x40x136"]["clip_y"] >= 1
    assert seen["2x2x20x72"]["uncovered"] == 0
