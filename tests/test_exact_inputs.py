"""The proof obligations of tests/_exact.py, on the CPU: for every case tests/test_gpu_exact.py runs,
  * every input is a number of fp16 and of bf16 (a flow: of the format it is stored in);
  * the fp32 oracle and the same source built in double (oracle/Makefile: libmemc_oracle64.so) return the same numbers
    for every output -- nothing rounded anywhere in the fp32 build;
  * the sum of absolute terms of every output stays below 2^24 quanta (budget()): no partial sum rounds in ANY order;
  * the quantised flow of a census-table case still reaches the in-kernel paths tests/test_lowp_path_census.py states
    for it, in each of its three storages;
  * sites sit exactly on the edges of the validity test.
These are conditions on the inputs.  If a seed misses one, the seed changes, not the condition.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact as E                        # noqa: E402
import _lowp_paths as LP                  # noqa: E402
import test_lowp_path_census as CENSUS    # noqa: E402

HALVES = {"fp16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def oracle64():
    from oracle import memc_oracle64
    memc_oracle64.build()
    memc_oracle64.lib()
    return memc_oracle64


def survives(a, tnames=("fp16", "bf16")):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return all(torch.equal(t.to(HALVES[n]).float(), t) for n in tnames)


def same(a32, a64, what):
    assert a32.dtype == np.float32 and a64.dtype == np.float64
    assert np.array_equal(a32.astype(np.float64), a64), "%s: the fp32 oracle rounded somewhere (max diff %g)" % (
        what, np.abs(a32 - a64).max())


def prove_fi(oracle, oracle64, x, flow, filt, gout, what, backward=True):
    same(oracle.filter_interpolation_forward(x, flow, filt), oracle64.filter_interpolation_forward(x, flow, filt), what + " forward")
    if backward:
        for a, b, n in zip(oracle.filter_interpolation_backward(x, flow, filt, gout),
                           oracle64.filter_interpolation_backward(x, flow, filt, gout), ("image", "flow", "tap")):
            same(a, b, "%s %s gradient" % (what, n))
    m = E.budget(oracle64, x, flow, filt, gout)
    print("%s: budget %s" % (what, m))
    assert E.holds(m), (what, m)
    # the flow gradient's analytic bound is a bound
    if backward:
        assert np.abs(oracle64.filter_interpolation_backward(x, flow, filt, gout)[1]).max() <= m["fi_flow"]


@pytest.mark.parametrize("ci", range(len(E.TABLE)), ids=E.TABLE_IDS)
def test_table_cases(oracle, oracle64, ci):
    case = E.TABLE[ci]
    for storage in E.storages_of(case):
        for C in E.FWD_CHANNELS[ci]:
            x, flow, filt, gout = E.table_inputs(case, C, storage)
            assert survives(x) and survives(filt) and survives(gout)
            assert survives(flow, ("fp16", "bf16") if storage == "bf16" else ("fp16",) if storage == "fp16" else ())
            assert np.array_equal(flow * 4, np.round(flow * 4))
            prove_fi(oracle, oracle64, x, flow, filt, gout, "%s C%d flow %s" % (E.TABLE_IDS[ci], C, storage), backward=C == 3)


@pytest.mark.parametrize("ci", range(len(E.TABLE)), ids=E.TABLE_IDS)
def test_blend_directions(oracle, oracle64, ci):
    """both directions of the blend: forward (two exact products, one exact sum), the backward on gradoutput * occlusion
    and the occlusion gradient sum_c gradoutput * forward"""
    case = E.TABLE[ci]
    for storage in E.storages_of(case):
        h = E.blend_inputs(case, storage)
        assert all(survives(h[n]) for n in ("x0", "x2", "k0", "k1", "o0", "o1", "gout"))
        assert set(np.unique(h["o0"] * 8)) <= set(range(-8, 9)) and (h["o0"] == 0).sum() > 0 and (h["o0"] < 0).sum() > 0
        w = []
        for x, f, k, o in (("x0", "f0", "k0", "o0"), ("x2", "f1", "k1", "o1")):
            go = h["gout"] * h[o]
            for a, b, n in zip(oracle.filter_interpolation_backward(h[x], h[f], h[k], go),
                               oracle64.filter_interpolation_backward(h[x], h[f], h[k], go.astype(np.float64)), ("image", "flow", "tap")):
                same(a, b, "%s %s blend %s gradient" % (E.TABLE_IDS[ci], x, n))
            w32, w64 = oracle.filter_interpolation_forward(h[x], h[f], h[k]), oracle64.filter_interpolation_forward(h[x], h[f], h[k])
            same(w32, w64, "warp " + x)
            same((h["gout"] * w32).sum(axis=1, keepdims=True, dtype=np.float32),
                 (h["gout"].astype(np.float64) * w64).sum(axis=1, keepdims=True), "occlusion gradient " + o)
            w.append((h[o] * w32, h[o].astype(np.float64) * w64))
            m = E.budget(oracle64, h[x], h[f], h[k], h["gout"], h[o])
            print("%s %s flow %s: budget %s" % (E.TABLE_IDS[ci], x, storage, m))
            assert E.holds(m), m
        same(w[0][0] + w[1][0], w[0][1] + w[1][1], "blend forward")


def test_census_of_the_quantised_flows():
    for ci, case in enumerate(LP.CASES):
        B, H, W = case[:3]
        for storage in E.STORAGES:
            c = LP.census(E.table_flow(case, storage))
            CENSUS._show("%s quantised, flow %s" % (LP.CASE_IDS[ci], storage), c)
            assert c["tiles"] == B * ((H + 15) // 16) * ((W + 63) // 64)
            CENSUS.CONDITIONS[ci](c)
    # the blend's second direction sweeps bands too (test_blend_second_direction_sweeps_bands_too)
    for ci, case in enumerate(LP.BLEND_CASES):
        for storage in E.STORAGES:
            c1 = LP.census(E.table_flow(case, storage, True))
            assert c1["max_bands_run"] > 1 and c1["nbx_gt1"] >= 1 and c1["nby_gt1"] >= 1, (case, storage, c1)
    # the two added cases (test_gpu_blend_grad.test_census_of_the_added_cases)
    far = LP.census(E.table_flow(E.FAR))
    CENSUS._show("1x20x1280-far quantised", far)
    assert far["valid"] < 0.5 * far["sites"] and far["mixed_lanes"] > 0 and far["slow"] > 0 and far["capped"] > 0, far
    narrow = LP.census(E.table_flow(E.EXTRA[0]))
    assert narrow["tiles"] == 2 * 3 and narrow["ragged_cols"] == 8 and narrow["ragged_rows"] == 5, narrow


def test_sites_exactly_on_the_edges_of_the_validity_test():
    best = {}
    for ci, case in enumerate(E.TABLE):
        for storage in E.storages_of(case):
            b = E.border_sites(E.table_flow(case, storage))
            print("%s flow %s: %s" % (E.TABLE_IDS[ci], storage, b))
            best[(ci, storage)] = b
    assert any(all(v >= 5 for v in b.values()) for b in best.values()), best


@pytest.mark.parametrize("row", E.many_rows(), ids=["%dx%dx%dx%d-%s" % r for r in E.many_rows()])
def test_many_channel_rows(oracle, oracle64, row):
    x, flow, filt, gout = E.many_inputs(row)
    assert survives(x) and survives(filt) and survives(gout)
    what = "%dx%dx%dx%d-%s" % row
    prove_fi(oracle, oracle64, x, flow, filt, gout, what)
    prove_bilinear(oracle, oracle64, x, flow, gout, what)


def prove_bilinear(oracle, oracle64, x, flow, gout, what):
    same(oracle.interpolation_ch_forward(x, flow), oracle64.interpolation_ch_forward(x, flow), what + " bilinear forward")
    for a, b, n in zip(oracle.interpolation_ch_backward(x, flow, gout), oracle64.interpolation_ch_backward(x, flow, gout), ("image", "flow")):
        same(a, b, "%s bilinear %s gradient" % (what, n))
        if n == "flow":
            assert np.abs(b).max() <= 4.0 * x.shape[1] * E.G
    m = E.bilinear_budget(oracle64, x, flow, gout)
    assert E.holds(m), (what, m)


def test_bilinear_rgb_cases(oracle, oracle64):
    for name, x, flow, gout in E.bilinear_rgb_cases():
        prove_bilinear(oracle, oracle64, x, flow, gout, name)
        same(oracle.interpolation_forward(x, flow), oracle64.interpolation_forward(x, flow), name + " Interpolation forward")
        for a, b in zip(oracle.interpolation_backward(x, flow, gout), oracle64.interpolation_backward(x, flow, gout)):
            same(a, b, name + " Interpolation gradient")


@pytest.mark.parametrize("name", sorted(E.SHAPES))
def test_other_shapes(oracle, oracle64, name):
    x, flow, filt, gout = E.shaped_inputs(*E.SHAPES[name])
    assert survives(x) and survives(filt) and survives(gout) and survives(flow)
    prove_fi(oracle, oracle64, x, flow, filt, gout, name)


def test_parity_blend_cases_and_the_layers_case(oracle, oracle64):
    hs = [E.parity_blend_inputs(c) for c in E.parity_blend_cases()] + [E.blend_inputs(E.LAYER_CASE, s) for s in E.STORAGES]
    for h in hs:
        assert all(survives(h[n]) for n in ("x0", "x2", "k0", "k1", "o0", "o1", "gout"))
        for x, f, k, o in (("x0", "f0", "k0", "o0"), ("x2", "f1", "k1", "o1")):
            go = h["gout"] * h[o]
            prove_fi(oracle, oracle64, h[x], h[f], h[k], go, "blend direction " + x)
            m = E.budget(oracle64, h[x], h[f], h[k], h["gout"], h[o])
            assert E.holds(m), m


@pytest.mark.parametrize("name", E.PROJECTION)
def test_projection_sums(oracle, oracle64, name):
    """the numpy scatter of _exact.project_sums IS the oracle's: equal counts, and the oracle's quotient is the correctly
    rounded s / c; the sums stay below 2^24 quanta"""
    flow, dep = E.projection_inputs(name)
    assert survives(dep) and flow.shape[2] <= 200 and flow.shape[3] <= 320
    for d, q in ((None, "proj"), (dep, "dproj")):
        s, c = E.project_sums(flow, d)
        if d is None:
            out32, cnt32 = oracle.flow_projection_forward(flow, 0)
            out64, cnt64 = oracle64.flow_projection_forward(flow, 0)
        else:
            out32, cnt32 = oracle.depth_flow_projection_forward(flow, d, 0)
            out64, cnt64 = oracle64.depth_flow_projection_forward(flow, d, 0)
        same(cnt32, cnt64, name + " count")
        assert np.array_equal(cnt64, c), name
        hit = np.broadcast_to(c > 0, s.shape)
        assert hit.mean() > 0.02 and (~hit).sum() > 0, (name, hit.mean())     # cells that collect and cells that do not
        want = np.where(hit, s / np.where(c > 0, c, 1.0), 0.0)
        assert np.array_equal(out64, want), name
        assert np.array_equal(out32, want.astype(np.float32)), name
        # sum of absolute terms: the scatter of |flow| (times the depth)
        sa, _ = E.project_sums(np.abs(flow), d)
        m = {q: float(np.abs(sa).max())}
        print("%s %s: %s, count up to %g" % (name, q, m, c.max()))
        assert E.holds(m) and c.max() * 8 < E.LIMIT
