"""The proof obligations of tests/_exact.py, on the CPU: for every case tests/test_gpu_exact.py runs,
  * every input is a number of fp16 and of bf16 (a flow: of the format it is stored in);
  * the fp32 oracle and the same source built in double (oracle/Makefile: libmemc_oracle64.so) return the same numbers
    for every output -- nothing rounded anywhere in the fp32 build;
  * the sum of absolute terms of every output stays below 2^24 quanta (budget()): no partial sum rounds in ANY order;
  * the quantised flow of a census-table case still reaches the in-kernel paths tests/test_lowp_path_census.py states
    for it, in each of its three storages;
  * sites sit exactly on the edges of the validity test;
  * the projection backward on synthetic power-of-two counts: the same three proofs, and a census of the in-kernel
    branches (uncovered sites, boxes clipped in x and in y, empty tiles, tail columns, the one-lane-per-site route) that
    _lowp_paths.proj_bwd_census restates from flow_projection.hip and memc_tile.hpp;
  * the projection forward with hole filling: the oracle's count is the numpy scatter's under signed depths too, a cell
    with count <= 0 holds the raw sum, the oracle's own fp32 fill stays within 2 * 2^-24 * S of a float64 restatement
    (_exact.fill_expectation, itself held to a cell-by-cell transcription of project_fillhole); the route launch_proj_fwd
    takes and the 64 x 32 tiles, restated in _lowp_paths and held to the sources' text; a census of what the cases reach
    (filled holes by their number of neighbours, walks that leave their tile, cross nine tiles or more, or find nothing,
    tiles nothing lands in, and the four things only signed depths do); and a floor on how far a walk that is one cell off
    moves the result -- a condition on the cases;
  * the context features beside the frames, and split lanes and slow sites in both directions of a context case;
  * the x4 upsampling: the scaled flow is exact and torch's CPU result is the same in fp32 and float64.
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


# ------------------------------------------------------------------------------------------------------------------
# projection forward with hole filling: the oracle against a float64 restatement of its fill, the routes and a census
# ------------------------------------------------------------------------------------------------------------------
def proj_oracle(oracle, name, op):
    """(output without fill, count, output with fill) of the fp32 oracle, once per session"""
    def make():
        flow, d = E.projection_operator(name, op)
        run = (lambda fill: oracle.flow_projection_forward(flow, fill)) if d is None else \
            (lambda fill: oracle.depth_flow_projection_forward(flow, d, fill))
        (o0, c0), (o1, c1) = run(0), run(1)
        assert np.array_equal(c0, c1)
        return o0, c0, o1
    return E._once(("proj-oracle", name, op), make)


def test_signed_depth_is_on_the_grid():
    d = E.signed_depth(1, 2, 40, 50)
    assert survives(d) and set(np.unique(d * 8)) == set(range(-9, 10))
    assert sorted(E.PROJECTION_SIGNED) == sorted(n for n, op in E.PROJECTION_OPS if op == "signed")
    for name in E.PROJECTION_ALL:
        flow, dep = E.projection_inputs(name)
        assert np.array_equal(flow * 4, np.round(flow * 4)) and survives(dep) and dep.min() > 0
        assert max(flow.shape[2:]) in (600, 1280) or (flow.shape[2] <= 200 and flow.shape[3] <= 320), name


@pytest.mark.parametrize("name,op", E.PROJECTION_OPS, ids=E.PROJECTION_OP_IDS)
def test_projection_fill_cases(oracle, name, op):
    """Per case and operator: the oracle's count is project_sums' bit for bit (signed depths included: every sign is certain);
    the sums of absolute terms stay below 2^24 quanta; without hole filling a cell with count <= 0 holds float32(s), the raw
    sum nothing divided; with it, a kept hole still does, every other cell outside the filled holes is unchanged, and a
    filled hole is within 2 * 2^-24 * S of fill_expectation on the oracle's own unfilled output.  Observed: 1.989 at the
    worst (2x70x134-patch-empty, flow), printed per case.  (Two additions and a division each rounding once give 3 a
    priori; the oracle stays below 2 on these cases.)"""
    flow, d = E.projection_operator(name, op)
    s, c = E.project_sums(flow, d)
    o0, c0, o1 = proj_oracle(oracle, name, op)
    assert c0.dtype == np.float32 and np.array_equal(c0.astype(np.float64), c), name
    sa, ca = E.project_sums(np.abs(flow), None if d is None else np.abs(d))
    m = {"proj" if d is None else "dproj": float(np.abs(sa).max())}
    assert E.holds(m) and ca.max() * 8 < E.LIMIT, (name, m)
    s32 = s.astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), s)
    low = np.broadcast_to(c <= 0, s.shape)
    assert np.array_equal(o0[low], s32[low]), "%s %s: a cell with count <= 0 must hold the raw sum" % (name, op)
    v, S, n, filled, kept = E.fill_expectation(o0, c0)
    f2, k2 = np.broadcast_to(filled, v.shape), np.broadcast_to(kept, v.shape)
    assert np.array_equal(filled | kept, c <= 0) and not (filled & kept).any()
    assert np.array_equal(o1[k2], s32[k2]), "%s %s: a kept hole must hold the raw sum" % (name, op)
    assert np.array_equal(o1[~f2], o0[~f2]), "%s %s: the fill wrote a cell that is no filled hole" % (name, op)
    err = np.abs(o1.astype(np.float64) - v)[f2]
    worst = float((err / np.maximum(S[f2], 1e-300)).max()) * 2.0 ** 24 if err.size else 0.0
    print("%s %s: sum of absolute terms %s, oracle's fill within %.3f * 2^-24 * S over %d filled holes" % (name, op, m, worst, int(filled.sum())))
    assert bool((err <= 2.0 * 2.0 ** -24 * S[f2]).all()), (name, op, worst)
    one = np.broadcast_to(filled & (n == 1), v.shape)
    assert np.array_equal(o1[one].astype(np.float64), v[one])       # one neighbour: its value, unrounded


def test_projection_forward_constants_are_the_sources():
    """_lowp_paths.proj_fwd_route and the 64 x 32 tiles of proj_fwd_census restate launch_proj_fwd (flow_projection.hip),
    vec4_ok (memc_tile.hpp) and the masks of proj_fill.hpp; a change there must change them here too."""
    import re
    csrc = os.path.join(LP.ROOT, "memc-net_amd", "csrc")
    with open(os.path.join(csrc, "flow_projection.hip")) as f:
        proj = f.read()
    with open(os.path.join(csrc, "memc_tile.hpp")) as f:
        tile = f.read()
    with open(os.path.join(csrc, "proj_fill.hpp")) as f:
        fill = f.read()

    def one(text, pattern, what):
        m = re.findall(pattern, text, re.M)
        assert len(m) == 1, "expected exactly one `%s` (%s), found %d" % (pattern, what, len(m))
        return m[0]

    assert int(one(proj, r"^constexpr int kOwnerTH = (\d+), kOwnerSW = \d+;", "the owner tile's height")) == LP.PF_TH
    launcher = proj[proj.index("static int launch_proj_fwd(const ProjFwdCall &a)"):]
    launcher = launcher[:launcher.index("\n}\n")]
    one(launcher, r"const bool vec = vec4_ok\(w, ", "the quad precondition")
    one(launcher, r"if \(!vec && w >= 8 && g_proj_variant < 0\) \{", "a ragged width of two quads or more")
    one(launcher, r"const int r = run_proj_fwd<DEPTH, kOwnerTH, true>\(a, kOwnerSW\);", "the ragged-row instantiation")
    one(launcher, r"if \(vec && g_proj_variant != 0\) \{", "whole quads")
    one(launcher, r"return run_proj_fwd<DEPTH, kOwnerTH>\(a, kOwnerSW\);", "the owner route")
    one(launcher, r'MEMC_PATH\(DEPTH \? "dproj_fwd:scalar" : "proj_fwd:scalar"\);', "the scalar route")
    one(launcher, r"hipLaunchKernelGGL\(proj_fillhole, ", "the scalar route's hole filling")
    one(proj, r'MEMC_PATH\(r\.flag \? \(DEPTH \? "dproj_fwd:owner" : "proj_fwd:owner"\)', "both owner instantiations record `owner`")
    one(tile, r"inline bool vec4_ok\(int w,[^{]*\{\s*\(void\)strides;\s*\(void\)ptrs;\s*return w % 4 == 0;", "vec4_ok: the width alone")
    one(proj, r"r\.ntx = \(a\.w \+ 63\) / 64;\s+r\.nty = \(a\.h \+ TH - 1\) / TH;", "64 x TH tiles")
    one(fill, r"unsigned long long row\[TH\];\s*// bit c: cell \(row, c\) of the tile has a non-zero count", "64 columns per tile")
    assert len(re.findall(r"if \(in_row && oc\[j\] != 0\.0f\) nz \|= 1u << j;", fill)) == 1           # what stops a walk
    assert len(re.findall(r"if \(in_row && oc\[j\] <= 0\.0f\) hole \|= 1u << j;", fill)) == 1         # what is filled
    assert (LP.PF_TW, LP.PF_TH) == (64, 32)
    assert LP.proj_fwd_route(128) == ("owner", False) and LP.proj_fwd_route(8) == ("owner", False)
    assert LP.proj_fwd_route(134) == ("owner", True) and LP.proj_fwd_route(9) == ("owner", True)
    assert LP.proj_fwd_route(7) == ("scalar", False) and LP.proj_fwd_route(4) == ("owner", False)


def test_fill_expectation_is_the_oracle_walk():
    """fill_expectation against a cell-by-cell transcription of oracle/memc_oracle.c project_fillhole on small planes of
    signed counts: a negative count stops a walk and contributes nothing, a walk that finds nothing contributes nothing, a
    hole is kept when its stops' counts sum to <= 0.  (The oracle itself: test_projection_fill_cases.)"""
    rng = np.random.default_rng(77)
    seen = set()
    for trial in range(20):
        B, H, W = 2, int(rng.integers(1, 8)), int(rng.integers(1, 10))
        c = rng.choice([0.0, 0.0, 0.0, -0.5, -1.0, 0.25, 2.0], (B, 1, H, W))
        o = (rng.integers(-64, 65, (B, 2, H, W)) / 4.0).astype(np.float32)
        v, S, n, filled, kept = E.fill_expectation(o, c)
        for b in range(B):
            for y in range(H):
                for x in range(W):
                    cn = c[b, 0]
                    if not cn[y, x] <= 0:
                        assert not filled[b, 0, y, x] and not kept[b, 0, y, x]
                        continue
                    lo, lt = x, 0.0
                    while lt == 0.0 and lo - 1 >= 0:
                        lo -= 1
                        lt = cn[y, lo]
                    ro, rt = x, 0.0
                    while rt == 0.0 and ro + 1 <= W - 1:
                        ro += 1
                        rt = cn[y, ro]
                    uo, ut = y, 0.0
                    while ut == 0.0 and uo - 1 >= 0:
                        uo -= 1
                        ut = cn[uo, x]
                    if lt + rt + ut <= 0.0:
                        assert kept[b, 0, y, x] and not filled[b, 0, y, x] and (v[b, :, y, x] == 0).all()
                        seen.add("kept-beside-positive" if max(lt, rt, ut) > 0 else "kept")
                        continue
                    fl, fr, fu = float(lt > 0), float(rt > 0), float(ut > 0)
                    assert filled[b, 0, y, x] and not kept[b, 0, y, x] and n[b, 0, y, x] == fl + fr + fu
                    seen.add("n%d" % (fl + fr + fu))
                    if min(lt, rt, ut) < 0:
                        seen.add("past-negative")
                    for k in (0, 1):
                        p = o[b, k].astype(np.float64)
                        assert v[b, k, y, x] == (fl * p[y, lo] + fr * p[y, ro] + fu * p[uo, x]) / (fl + fr + fu)
                        assert S[b, k, y, x] == (fl * abs(p[y, lo]) + fr * abs(p[y, ro]) + fu * abs(p[uo, x])) / (fl + fr + fu)
    assert seen == {"kept", "kept-beside-positive", "n1", "n2", "n3", "past-negative"}, seen


# what the case list as a whole must reach (a count: at least five cells or one tile), and each signed case on its own
PF_REACHED = ["n1", "n2", "n3", "other_tile_l", "other_tile_r", "other_tile_u", "nothing_l", "nothing_r", "nothing_u", "empty_tiles"]
PF_SIGNED = ["negative", "zero_count_nonzero_sum", "kept_beside_positive", "filled_past_negative"]


def test_projection_fill_census(oracle):
    total = {}
    for name, op in E.PROJECTION_OPS:
        flow, d = E.projection_operator(name, op)
        s, c = E.project_sums(flow, d)
        cen = LP.proj_fwd_census(s, c)
        o0, c0, _o1 = proj_oracle(oracle, name, op)
        cen["sensitivity"] = round(E.fill_sensitivity(o0, c0)[0], 3)
        print("%s %s: %s" % (name, op, " ".join("%s=%s" % kv for kv in cen.items())))
        W = flow.shape[3]
        assert cen["route"] == ("scalar" if name == "2x9x7-iid2" else "owner") and cen["ragged"] == (W % 4 != 0 and W >= 8)
        assert cen["filled"] == cen["n1"] + cen["n2"] + cen["n3"] and cen["holes"] == cen["filled"] + cen["kept"]
        for k, val in cen.items():
            if isinstance(val, (int, np.integer)) and not isinstance(val, bool):
                total[k] = max(total.get(k, 0), int(val)) if k.startswith("borders_") else total.get(k, 0) + int(val)
        if op == "signed":
            assert all(cen[k] > 0 for k in PF_SIGNED), (name, cen)
        else:
            assert all(cen[k] == 0 for k in PF_SIGNED), (name, cen)
        if name == "2x70x134-patch-empty":                      # image 1: nothing lands, every cell an unfilled hole
            assert (c[1] == 0).all() and cen["kept"] >= c[1].size and cen["empty_tiles"] >= 9
    print("all cases:", total)
    assert all(total[k] >= 5 for k in PF_REACHED if k != "empty_tiles") and total["empty_tiles"] >= 1, total
    assert total["borders_u"] >= 9 and total["borders_r"] >= 9, total        # the pending filler's rounds of eight make a second trip
    assert any(LP.proj_fwd_route(E.projection_inputs(n)[0].shape[3]) == ("owner", True) for n in E.PROJECTION_ALL)
    assert any(LP.proj_fwd_route(E.projection_inputs(n)[0].shape[3])[0] == "scalar" for n in E.PROJECTION_ALL)


@pytest.mark.parametrize("name,op", E.PROJECTION_OPS, ids=E.PROJECTION_OP_IDS)
def test_projection_fill_sensitivity(oracle, name, op):
    """A condition on the cases, not a measurement: where a walk ends one cell too far, the fill must move by more than four
    times the bound the GPU test allows, at half of the filled holes at least (0.9 in three cases).  If a case misses its
    floor its flow changes, not the floor."""
    o0, c0, _o1 = proj_oracle(oracle, name, op)
    share, n_filled = E.fill_sensitivity(o0, c0)
    print("%s %s: sensitivity %.3f over %d filled holes" % (name, op, share, n_filled))
    if n_filled > 100:
        assert share >= (0.9 if name in E.PROJECTION_SENSITIVE else 0.5), (name, op, share)


# ------------------------------------------------------------------------------------------------------------------
# projection backward: synthetic power-of-two counts make every quotient exact
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_depth", [False, True], ids=["flow", "depth"])
@pytest.mark.parametrize("name", E.PB_IDS)
def test_projection_backward_cases(oracle, oracle64, name, with_depth):
    h = E.proj_bwd_inputs(name, with_depth)
    flow, cnt, gout = h["flow"], h["count"], h["gout"]
    assert np.array_equal(flow * 4, np.round(flow * 4))              # (stored in fp32, unclipped: the operator has no other storage)
    assert survives(cnt) and survives(gout) and np.abs(gout).max() <= E.G and np.array_equal(gout, np.round(gout))
    # the premise: a power of two (signed, with a depth) exactly where the true scatter puts anything, exactly 0 elsewhere
    hit = E.project_sums(flow)[1] > 0
    assert np.array_equal(cnt != 0, hit)
    m, e = np.frexp(cnt[hit])
    assert np.array_equal(np.abs(m), np.full(m.shape, 0.5)) and (-1 if with_depth else 1) <= e.min() and e.max() <= 5
    if with_depth:                                                   # real depth counts can be negative
        assert hit.sum() < 8 or ((cnt[hit] > 0).any() and (cnt[hit] < 0).any())
    else:
        assert (cnt[hit] > 0).all()
    zero = ~hit[:, 0]
    if zero.sum() >= 2:                                              # both kinds of gradoutput on the cells of count 0
        assert (gout[:, 0][zero] == 0).any() and (gout[:, 0][zero] != 0).any(), name
    if with_depth:
        assert survives(h["depth"]) and survives(h["fwd_out"]) and np.abs(h["fwd_out"]).max() <= 64
        assert np.array_equal(h["fwd_out"] * 4, np.round(h["fwd_out"] * 4))
        got32 = oracle.depth_flow_projection_backward(flow, h["depth"], cnt, h["fwd_out"], gout)
        got64 = oracle64.depth_flow_projection_backward(flow, h["depth"], cnt, h["fwd_out"], gout)
        for a, b, n in zip(got32, got64, ("gradinput1", "gradinput2")):
            same(a, b, "DepthFlowProjection backward %s %s" % (name, n))
    else:
        got64 = (oracle64.flow_projection_backward(flow, cnt, gout),)
        same(oracle.flow_projection_backward(flow, cnt, gout), got64[0], "FlowProjection backward %s gradinput1" % name)
    assert all(np.isfinite(g).all() for g in got64), "%s: a valid site read a count of zero" % name
    m = E.proj_bwd_budget(h)
    print("%s %s: budget %s" % (name, "depth" if with_depth else "flow", m))
    assert E.holds(m), (name, m)
    # the sums of absolute terms bound the results
    keys = ("dpb_g1", "dpb_g2") if with_depth else ("pb_g1",)
    assert all(np.abs(g).max() <= m[k] for g, k in zip(got64, keys)), (name, m)


def test_projection_backward_constants_are_the_sources():
    """The census of _lowp_paths.proj_bwd_census restates flow_projection.hip and memc_tile.hpp (kPitch = kTW + 32, kTW = 4 * LX:
    test_lowp_path_census.test_census_constants_are_the_headers); a change there must change it here too."""
    import re
    csrc = os.path.join(LP.ROOT, "memc-net_amd", "csrc")
    with open(os.path.join(csrc, "flow_projection.hip")) as f:
        proj = f.read()
    with open(os.path.join(csrc, "memc_tile.hpp")) as f:
        tile = f.read()

    def one(text, pattern, what):
        m = re.findall(pattern, text, re.M)
        assert len(m) == 1, "expected exactly one `%s` (%s), found %d" % (pattern, what, len(m))
        return m[0]

    launcher = proj[proj.index("static int launch_proj_bwd(const ProjBwdCall &k)"):]
    launcher = launcher[:launcher.index("\n}\n")]
    assert int(one(launcher, r"^\s*launch_proj_bwd_tiled<DEPTH,\s*(\d+)>\(k\);", "the product build's staging budget")) == LP.PB_CAP
    one(launcher, r"const int ws = k\.w & ~3;", "whole quads")
    one(launcher, r"if \(\(vec \|\| \(ws >= 8 && g_proj_variant < 0\)\) && g_proj_variant != 0\)", "the routing")
    one(launcher, r"if \(ws < k\.w\) launch_proj_bwd_direct<DEPTH>\(k, ws\);", "the tail columns' launch")
    one(tile, r"inline bool vec4_ok\(int w,[^{]*\{\s*\(void\)strides;\s*\(void\)ptrs;\s*return w % 4 == 0;", "vec4_ok: the width alone")
    kernel = proj[proj.index("void proj_bwd_tiled("):proj.index("MEMC_KNOB_STATIC(g_proj_variant")]
    assert int(one(kernel, r"constexpr int LX = (\d+);", "lanes per tile row")) == LP.LX
    one(kernel, r"Region r = tile_region<LX, true, CAP>\(cmin, cmax, rmin, rmax, tile_x0, tile_y0, bb\);", "the dynamic-pitch region")
    one(kernel, r"st\[j\] = bl_locate<false>\(x \+ j, y, W, H, fx4\[j\], fy4\[j\]\);", "the projection's validity test")
    one(kernel, r"if \(r\.covers\(s\.L, s\.R, s\.T, s\.Bm\)\)", "the covered branch")
    one(tile, r"static constexpr int kTH = kThreads / LX;", "the tile height")
    assert LP.TW + int(one(tile, r"static constexpr int kPitch\s*=\s*kTW\s*\+\s*(\d+)\s*;", "kPitch = kTW + pad")) == LP.PITCH
    one(tile, r"int x0 = cmin & ~3, w = \(cmax \| 3\) \+ 1 - x0;", "4-alignment of the box")
    one(tile, r"x0 = min\(max\(\(tile_x0 \+ G::kTW / 2 - G::kPitch / 2\) & ~3, lo\), hi\);", "the clip in x")
    one(tile, r"const int pitch = DYN \? \(\(w \+ 15\) & ~15\) : G::kPitch;", "the dynamic pitch")
    one(tile, r"const int rows = DYN \? G::kCapPx / pitch : G::kRows;", "the rows that fit")
    one(tile, r"y0 = min\(max\(tile_y0 \+ G::kTH / 2 - rows / 2, lo\), hi\);", "the clip in y")
    one(tile, r"return cmin >= x0 && cmax < x0 \+ w && rmin >= y0 && rmax < y0 \+ h;", "Region::covers")
    assert (LP.LX, LP.TW, LP.TH, LP.PITCH, LP.PB_CAP // LP.PITCH, LP.PB_CAP // 64) == (16, 64, 16, 96, 26, 39)
    # tile_region on its own: a box that fits, one clipped in x, one clipped in y
    assert LP.tile_region(5, 70, 3, 20, 0, 0) == (4, 3, 68, 18, False, False)
    assert LP.tile_region(0, 255, 0, 9, 64, 0) == (48, 0, 96, 10, True, False)           # centred on the tile: 64 + 32 - 48
    assert LP.tile_region(64, 127, 0, 63, 64, 16) == (64, 5, 64, 39, False, True)        # pitch 64: 39 rows, 19 above row 24
    assert LP.proj_bwd_route(7) == ("scalar", 4) and LP.proj_bwd_route(3) == ("scalar", 0)
    assert LP.proj_bwd_route(4) == ("tiled", 4) and LP.proj_bwd_route(9) == ("tiled", 8) and LP.proj_bwd_route(131) == ("tiled", 128)


# what tests/test_gpu_exact.py relies on per projection-backward case: classes of at least five sites (one tile for the tile
# classes).  Conditions, not measurements: if a case misses one, its seed or sigma changes.
PB_UNCOVERED = ["1x96x256-smooth25", "2x64x256-iid20", "1x112x320-iid30", "1x200x320-smooth40", "2x100x132-smooth8",
                "1x20x1280-far", "2x33x131-iid12"]
PB_CONDITIONS = {
    "1x96x256-smooth25": dict(clip_x=1, clip_y=1),
    "2x64x256-iid20": dict(clip_x=32, clip_y=32),                   # every tile
    "1x20x1280-far": dict(empty=1, clip_x=1),
    "2x100x132-smooth8": dict(empty=1, clip_y=1),
    "4x40x40-edges": dict(L_eq_R=5, T_eq_Bm=5, x2_0=5, y2_0=5),
    "W50-C3": dict(tail_valid=5), "W133-C3": dict(tail_valid=5), "1x17x9-iid2": dict(tail_valid=5),
    "1x40x134-smooth6": dict(tail_valid=5),
    "2x33x131-iid12": dict(clip_x=1, clip_y=1, tail_valid=5),
    "2x9x7-iid1.5": dict(tail_valid=5), "2x6x3-iid1": dict(tail_valid=5),      # (every site on the one-lane-per-site kernel)
}


@pytest.mark.parametrize("name", E.PB_IDS)
def test_projection_backward_census(name):
    flow = E.pb_flow(name)
    c, mask = LP.proj_bwd_census(flow)
    print("%s: %s" % (name, " ".join("%s=%s" % kv for kv in c.items())))
    B, _, H, W = flow.shape
    assert c["route"] == ("scalar" if name in E.PB_SCALAR else "tiled")
    if c["route"] == "tiled":
        assert c["tiles"] == B * ((H + 15) // 16) * (((W & ~3) + 63) // 64) and c["tiled_valid"] + c["tail_valid"] == c["valid"]
        assert (W % 4 != 0) == (name in E.PB_SHAPES[:2] or name in [E._pb_id(k) for k in E.PB_SMALL])
    assert int(mask.sum()) == c["uncovered"] and c["valid"] >= 5
    if name in PB_UNCOVERED:
        assert 5 <= c["uncovered"] < c["tiled_valid"] - 5, c          # both branches of Region::covers
    else:
        assert c["uncovered"] == 0, c
    for k, least in PB_CONDITIONS.get(name, {}).items():
        assert c[k] >= least, (name, k, c)


# ------------------------------------------------------------------------------------------------------------------
# the context warp (fi_fwd_ctx_img) and the x4 upsampling
# ------------------------------------------------------------------------------------------------------------------
def prove_context(oracle, oracle64, c, flow, filt, what):
    assert survives(c) and c.min() >= 0
    w64 = oracle64.filter_interpolation_forward(c, flow, filt)
    same(oracle.filter_interpolation_forward(c, flow, filt), w64, what)
    assert E.holds(dict(fi_fwd=float(w64.max()))), what


@pytest.mark.parametrize("ci", range(len(E.TABLE)), ids=E.TABLE_IDS)
def test_context_cases(oracle, oracle64, ci):
    """the context features of both directions (the frames and their blend: test_blend_directions)"""
    h = E.blend_inputs(E.TABLE[ci])
    for C in E.CTX_CHANNELS[ci]:
        c0, c2 = E.ctx_inputs(E.TABLE[ci], C)
        assert c0.shape[1] == C and not np.array_equal(c0, c2)
        prove_context(oracle, oracle64, c0, h["f0"], h["k0"], "%s context 0, C%d" % (E.TABLE_IDS[ci], C))
        prove_context(oracle, oracle64, c2, h["f1"], h["k1"], "%s context 2, C%d" % (E.TABLE_IDS[ci], C))


def test_context_cases_reach_split_lanes_and_slow_sites_in_both_directions():
    """fi_fwd_ctx_img's blend of ONE element (`blend1`) runs for lanes whose sites are split over bands and for the sites
    no band covers; its bands are make_bands<16>'s defaults, the census of _lowp_paths"""
    split = slow = 0
    for ci, case in enumerate(E.TABLE):
        c = [LP.census(E.table_flow(case, "fp32", second)) for second in (False, True)]
        print("%s: split lanes %d / %d, slow sites %d / %d" % (E.TABLE_IDS[ci], c[0]["split_lanes"], c[1]["split_lanes"],
                                                               c[0]["slow"], c[1]["slow"]))
        split += min(c[0]["split_lanes"], c[1]["split_lanes"]) >= 5
        slow += min(c[0]["slow"], c[1]["slow"]) >= 5
    assert split >= 1 and slow >= 1


def test_context_layer_cases(oracle, oracle64):
    for name in E.CTX_LAYER:
        h = E.ctx_layer_inputs(name)
        assert all(survives(h[n]) for n in ("x0", "x2", "c0", "c2", "k0", "k1", "o0", "o1"))
        w = []
        for x, c, f, k, o in (("x0", "c0", "f0", "k0", "o0"), ("x2", "c2", "f1", "k1", "o1")):
            prove_context(oracle, oracle64, h[c], h[f], h[k], "%s %s" % (name, c))
            w32, w64 = oracle.filter_interpolation_forward(h[x], h[f], h[k]), oracle64.filter_interpolation_forward(h[x], h[f], h[k])
            same(w32, w64, "%s warp %s" % (name, x))
            w.append((h[o] * w32, h[o].astype(np.float64) * w64))
            assert E.holds(dict(blend_fwd=2.0 * float(w64.max())))
        same(w[0][0] + w[1][0], w[0][1] + w[1][1], name + " blend forward")


@pytest.mark.parametrize("mul,div", E.UPSAMPLE_SCALES)
@pytest.mark.parametrize("shape", E.UPSAMPLE_SHAPES, ids=["%dx%dx%dx%d" % s for s in E.UPSAMPLE_SHAPES])
def test_upsample_inputs(shape, mul, div):
    """(mul * f) / div is exact in fp32 in either order, and torch's CPU bilinear x4 (align_corners = False: weights k / 8
    per axis) returns the same numbers in fp32 and in float64 -- an exact expectation"""
    import torch.nn.functional as F
    f = E.upsample_input(shape)
    assert survives(f) and np.abs(f).max() <= 64 and np.array_equal(f * 4, np.round(f * 4))
    t = torch.from_numpy(f)
    s64 = mul * t.double() / div
    for s32 in (mul * t / div, (mul * t) * (1.0 / div) if div == 2.0 else (mul * t) / div):
        assert s32.dtype == torch.float32 and torch.equal(s32.double(), s64)
    assert torch.equal(s64 * 2, torch.round(s64 * 2)) and float(s64.abs().max()) * 2.0 ** 7 < E.LIMIT      # quantum 2^-1 * 2^-6
    up32 = F.interpolate(mul * t / div, scale_factor=4, mode="bilinear", align_corners=False)
    up64 = F.interpolate(s64, scale_factor=4, mode="bilinear", align_corners=False)
    assert up32.dtype == torch.float32 and torch.equal(up32.double(), up64)
    assert torch.equal(up64 * 128, torch.round(up64 * 128))
