"""The premises of tests/_proj_bound.py, on the CPU: the fp32 oracle stays inside the derived per-cell bounds on every output
of the four projection entry points, the float64 oracle build agrees with the restatement to float64 roundoff, wrong
operators and a 12-bit reciprocal leave the bounds, and the bounds are far below 1e-4 where the flow is a few pixels.
Run with -s for the figures (profiles/proj_bounds_observed.md records them)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _parity as P          # noqa: E402
import _proj_bound as PB     # noqa: E402

IDS = [c[0] for c in PB.CASES]
_CACHE = {}


def inputs(c):
    """the case's inputs, the fp32 oracle's planes and the restatements: made once, shared, never written"""
    if c[0] not in _CACHE:
        from oracle import memc_oracle as O
        d = PB.make(c)
        d["fwd"] = {dep: PB.Forward(d["flow"], d["depth"] if dep else None) for dep in (False, True)}
        d["o"] = {}
        for dep in (False, True):
            for fill in (0, 1):
                d["o"][dep, fill] = (O.depth_flow_projection_forward(d["flow"], d["depth"], fill) if dep
                                     else O.flow_projection_forward(d["flow"], fill))
        out0, cnt0 = d["o"][False, 0]
        dout0, dcnt0 = d["o"][True, 0]
        d["bwd"] = {False: PB.Backward(d["flow"], None, cnt0, None, d["gout"]),
                    True: PB.Backward(d["flow"], d["depth"], dcnt0, dout0, d["gout"])}
        for a in d.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[c[0]] = d
    return _CACHE[c[0]]


def worst(r_ok):
    r, ok = r_ok
    return float(r[ok].max()) if ok.any() else 0.0


@pytest.mark.parametrize("c", PB.CASES, ids=IDS)
def test_the_fp32_oracle_lies_within_the_bound(oracle, c):
    d = inputs(c)
    seen = {}
    for dep in (False, True):
        fw, name = d["fwd"][dep], "dproj" if dep else "proj"
        assert fw.excluded == 0, "%s: %d cells without a bounded quotient" % (name, fw.excluded)
        for fill in (0, 1):
            out, cnt = d["o"][dep, fill]
            seen["%s count fill %d" % (name, fill)] = worst(fw.ratio_count(cnt))
            seen["%s out fill %d" % (name, fill)] = worst(fw.ratio_out(out, fill))
    seen["proj gin1"] = worst(d["bwd"][False].ratio1(oracle.flow_projection_backward(d["flow"], d["o"][False, 0][1], d["gout"])))
    g1, g2 = oracle.depth_flow_projection_backward(d["flow"], d["depth"], d["o"][True, 0][1], d["o"][True, 0][0], d["gout"])
    seen["dproj gin1"] = worst(d["bwd"][True].ratio1(g1))
    seen["dproj gin2"] = worst(d["bwd"][True].ratio2(g2))
    for k, v in seen.items():
        print("%-12s %-22s oracle err / bound %.3f" % (c[0], k, v))
    assert max(seen.values()) <= 1.0, seen
    # invalid sites are exactly zero, and the special values made some
    inv = ~d["bwd"][True].valid
    assert not g2[inv].any() and not g1[np.broadcast_to(inv, g1.shape)].any()
    if c[0] == "special":
        assert int(inv.sum()) >= 5


def _stats(name, bd, live):
    b = bd[np.broadcast_to(live, bd.shape)]
    b = b[np.isfinite(b)]
    return "%-12s median bound %.2e, largest %.2e, share above 1e-4: %.4f" % (
        name, float(np.median(b)) if b.size else 0.0, float(b.max()) if b.size else 0.0, float((b > 1e-4).mean()) if b.size else 0.0)


@pytest.mark.parametrize("c", PB.CASES, ids=IDS)
def test_the_bounds_are_far_below_the_parity_rule_where_the_flow_is_small(oracle, c):
    d = inputs(c)
    shares = {}
    for dep in (False, True):
        fw, bw, name = d["fwd"][dep], d["bwd"][dep], "dproj" if dep else "proj"
        print("%-12s %s: n max %d, live share %.3f, holes %.3f" % (c[0], name, int(fw.n.max()), float(fw.live.mean()), fw.holes()))
        rows = [("out fill 0", fw.out(0)[1], fw.live), ("out fill 1", fw.out(1)[1], np.ones_like(fw.live)),
                ("gin1", bw.bound1, bw.valid)]
        if dep:
            rows += [("count", fw.bound_count, fw.live), ("gin2", bw.bound2, bw.valid)]
        for what, bd, live in rows:
            print("  " + _stats(what, bd, live))
            b = bd[np.broadcast_to(live, bd.shape)]
            shares[name + " " + what] = float((b[np.isfinite(b)] > 1e-4).mean()) if b.size else 0.0
    if c[0] in PB.SMALL_FLOW:
        assert max(shares.values()) == 0.0, shares


CASES64 = ["smooth4", "iid3", "iid10", "smooth30", "iid160", "scalar"]      # (their seeds: the locations agree in double)


@pytest.mark.parametrize("name", CASES64)
def test_the_float64_oracle_build_agrees_with_the_restatement(name):
    """oracle/memc_oracle64.py locates in double and the flow is itself a summand here, so it is used only where the double
    and the float32 locations agree at every site (asserted); d * f stays unrounded on both sides."""
    from oracle import memc_oracle64 as O64
    d = inputs(PB.case(name))
    assert PB.locations_agree_in_double(d["flow"]), "pick another seed for %s" % name
    tol = 4 * 2.0 ** -45
    f64, d64, g64 = (d[k].astype(np.float64) for k in ("flow", "depth", "gout"))
    for dep in (False, True):
        r = PB.restate_forward(d["flow"], d["depth"] if dep else None, product32=False)
        out, cnt = O64.depth_flow_projection_forward(f64, d64, 0) if dep else O64.flow_projection_forward(f64, 0)
        live = r["n"] > 0
        assert np.all(np.abs(cnt - r["D"]) <= tol * r["massD"])
        with np.errstate(invalid="ignore", divide="ignore"):
            scale = np.where(live, r["massN"] / np.abs(r["D"]) + np.abs(r["want"]), 0.0)
        assert np.all(np.abs(out - r["want"]) <= tol * scale)
        cnt32, out32 = d["o"][dep, 0][1], d["o"][dep, 0][0]
        bw = d["bwd"][dep].r
        if dep:
            g1, g2 = O64.depth_flow_projection_backward(f64, d64, cnt32, out32, g64)
            assert np.all(np.abs(g2 - bw["want2"]) <= tol * bw["mass2"])
        else:
            g1 = O64.flow_projection_backward(f64, cnt32, g64)
        assert np.all(np.abs(g1 - bw["want1"]) <= tol * bw["mass1"])


# (mutation, output): the outputs that hold a term the mutation changes
MUTANTS = [("drop corner", "count"), ("drop corner", "out"), ("drop corner", "gin1"), ("drop corner", "gin2"),
           ("no clamp", "count"), ("no clamp", "gin1"), ("no clamp", "gin2"),
           ("swap out", "gin2"),
           ("neighbour d", "count"), ("neighbour d", "out"), ("neighbour d", "gin1"),
           ("rcp12", "gin1"), ("rcp12", "gin2"), ("rcp17", "gin1"), ("rcp17", "gin2")]
MUTANT_CASES = ["smooth4", "iid3", "iid10", "smooth30", "iid160"]


def _parity_bound(want, cancel=0.0):
    aw = np.abs(want)
    floor = max(P.ATOL, cancel * float(aw.max()))
    return np.where(aw <= P.BIG, floor, np.maximum(floor, P.RTOL * aw))


BORDER_CASES = ["two rows", "two columns"]      # the only ones with sites on the clamp: "no clamp" runs on these


@pytest.mark.parametrize("mutant,name", [(m, n) for m in MUTANTS for n in (BORDER_CASES if m[0] == "no clamp" else MUTANT_CASES)],
                         ids=lambda v: "%s, %s" % v if isinstance(v, tuple) else v)
def test_a_wrong_operator_breaks_the_bound(oracle, mutant, name):
    """Each mutation of the DepthFlowProjection restatement leaves want +- bound in more than half of the cells that hold a
    term it changes.  Printed beside it: the share of the same cells today's tests/_parity rule would flag."""
    mutation, what = mutant
    d = inputs(PB.case(name))
    fw, bw = d["fwd"][True], d["bwd"][True]
    if what in ("count", "out"):
        m = PB.restate_forward(d["flow"], d["depth"], mutate=mutation)
        if mutation == "neighbour d":                                   # (a cell with ONE term returns -fl32(d f) / d: no d left)
            reach = fw.live if what == "count" else fw.n >= 2
        else:                                                           # the cells whose set of terms changed
            reach = m["n"] != fw.n
        if what == "count":
            got, want, bd, cancel = m["D"], fw.want_count, fw.bound_count, 0.0
        else:
            got, (want, bd), cancel = m["want"], fw.out(0), 0.0
            reach = reach & fw.live & (m["n"] > 0)
    else:
        dout0, dcnt0 = d["o"][True, 0]
        m = PB.restate_backward(d["flow"], d["depth"], dcnt0, dout0, d["gout"], mutate=mutation)
        reach = bw.r["touches"] if mutation == "no clamp" else bw.valid
        if what == "gin1":
            got, want, bd, cancel = m["want1"], bw.want1, bw.bound1, 0.0
        else:
            got, want, bd, cancel = m["want2"], bw.want2, bw.bound2, P.CANCEL
    reach = np.broadcast_to(reach, got.shape)
    assert reach.any()
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
        beyond = ~(err <= bd)[reach]
        parity = ~(err <= _parity_bound(want, cancel))[reach]
    print("%-12s %-12s %-6s cells reached %6d, beyond the derived bound %.4f, beyond the parity rule %.4f"
          % (name, mutation, what, int(reach.sum()), float(beyond.mean()), float(parity.mean())))
    assert float(beyond.mean()) > 0.5
