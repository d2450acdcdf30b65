#!/usr/bin/env python
"""tools/bench_lowp_grad.py -- the half-precision adaptive-warp backward: the widened route against the native kernel, in
one process.

    python tools/bench_lowp_grad.py [--rounds 7] [--iters 10] [--only SUBSTRING] [--json out.json]

The widened route is what every half backward took before libmemc_hip_lp_grad.so, and what uncovered shapes still take
(FilterInterpolationLayer._backward_fp32 on the inputs cast to float32, each gradient cast back; for the blend,
_blend_backward on the widened inputs).  The native route is the code the autograd Functions now run (_backward_lp;
_blend_backward with the half tensors).  Both are timed as whole backward passes, casts and allocations included,
ALTERNATELY, round after round, so that clock and thermal drift fall on both alike; each launch rotates over input sets
that together exceed the 256 MiB Infinity Cache several times.  Printed per row: the per-round medians of both routes,
the median over the rounds, the spread (max - min over the rounds, relative to the median) and the ratio.

The `mixed` group (--only mixed) is the same comparison for the call torch.autocast makes -- a float32 image and a float32
gradoutput beside half taps: the promoted route (the saved taps and flow cast to float32, _backward_fp32, the tap and flow
gradients cast back: what _FilterInterpolationMxFunction.backward ran before libmemc_hip_mx_grad.so and still runs where
that library declines) against the one kernel on the tensors as they are (_backward_mx).  (--only mixed_bwd: that group
alone.)

The `mixed_blend` group (--only mixed_blend) is ONE direction of the blend layer's backward for such a call with frames
that are data: the promoted route (the direction's saved flow, taps and occlusion cast to float32, the float32 fused kernel
of libmemc_hip_blend_grad.so, the three gradients cast back: what _FilterInterpolationBlendMxFunction.backward ran before
libmemc_hip_mx_blend_grad.so and still runs where that library declines) against the one kernel on the tensors as they
are (_direction_backward_fused).

The `half_blend` group (--only half_blend) is ONE direction of the blend layer's backward for a PURE half call (a model cast
to bfloat16 / float16) with frames that are data: the composed route, which stays the layer's default (the direction's four
saved tensors and the gradoutput widened, a float32 forward recomputation, two elementwise passes and a channel sum, a
zero-filled image gradient, the warp's whole backward on libmemc_hip_lp_grad.so, four narrowing casts: what
_FilterInterpolationBlendLpFunction.backward runs per direction) against the one kernel of libmemc_hip_lp_blend_grad.so on
the tensors as they are (_direction_backward_fused: what FilterInterpolationBlendLayer(fused_half_backward=True) runs).
In these rows `widened` is the composed route and `native` the one kernel.

The `half_proj` group (--only half_proj) is ONE FlowProjection backward as a model cast to bfloat16 / float16 makes it: a
half flow, the float32 count of the forward, a half gradoutput, a half gradient.  `widened` is the route through
_common.host_widened (gradoutput cast to float32, my_lib.FlowProjectionLayer_gpu_backward on the float32 flow autograd kept,
the gradient cast back); `native` is the one call of libmemc_hip_lp_proj_grad.so on the tensors as they are
(_FlowProjectionLpFunction.backward).  Casts and allocations are included on both sides.

The `half_dproj` group (--only half_dproj) is ONE DepthFlowProjection backward as a model cast to bfloat16 / float16 makes
it: a half flow and depth, the float32 count and output of the forward, a half gradoutput, two half gradients.  `widened`
is the route through _common.host_widened, what DepthFlowProjectionLayer.native_half_backward = False runs (gradoutput cast
to float32, my_lib.DepthFlowProjectionLayer_gpu_backward on the float32 flow and depth autograd kept, both gradients cast
back); `native` is the one call of libmemc_hip_lp_dproj_grad.so on the tensors as they are
(_DepthFlowProjectionLpFunction.backward).  Casts and allocations are included on both sides.

The `half_bilinear` group (--only half_bilinear) is ONE RGB Interpolation backward as a model cast to bfloat16 / float16
makes it: a half image and gradoutput, the flow in float32 or that dtype.  `widened` is the route through
_common.host_widened (gradoutput cast to float32, a zero-filled float32 image gradient, my_lib.InterpolationLayer_gpu_backward
on the float32 image and flow autograd kept, both gradients cast back); `native` is the one call of libmemc_hip_lp_bl.so on
the tensors as they are (_InterpolationLpFunction.backward: a zero-filled float32 image gradient cast afterwards, the flow
gradient in the flow's dtype).  Casts and allocations are included on both sides.  Below 2^21 sites a backward is a few tens
of microseconds in four or five launches, and one backward between two events measures the host's enqueue as much as the
GPU (tools/bench_ops.time_launches): this group times bursts of 10 there, as tools/bench_lowp.py does for its small shape."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tools.bench_ops import time_launches      # noqa: E402
from tools import synth                        # noqa: E402

ROTATE_BYTES = 1 << 30


def _sets(shape, n, blend, T, half_flow, seed, mixed=False):
    B, C, H, W = shape
    ft = T if half_flow else torch.float32
    out = []
    it = torch.float32 if mixed else T                        # the image and gradoutput of a mixed call stay float32
    if blend == "one":                                        # one direction of the mixed (or the pure half) blend
        for i in range(n):
            t = synth.torch_inputs("cuda", B, C, H, W, flow_kind="smooth", seed=seed + 97 * i)
            g = torch.Generator("cuda").manual_seed(seed + i)
            out.append({"x": t["x"].to(it), "flow": t["flow"].to(ft), "filt": t["filt"].to(T),
                        "occ": torch.rand(B, 1, H, W, device="cuda", generator=g).to(T),
                        "gout": torch.randn(B, C, H, W, device="cuda", generator=g).to(it)})
        return out
    for i in range(n):
        t = synth.torch_inputs("cuda", B, C, H, W, flow_kind="smooth", seed=seed + 97 * i)
        g = torch.Generator("cuda").manual_seed(seed + i)
        s = {"x": t["x"].to(it), "flow": t["flow"].to(ft), "filt": t["filt"].to(T),
             "gout": torch.randn(B, C, H, W, device="cuda", generator=g).to(it)}
        if blend:
            u = synth.torch_inputs("cuda", B, C, H, W, flow_kind="smooth", seed=seed + 97 * i + 1)
            o = torch.rand(B, 1, H, W, device="cuda", generator=g)
            s.update(x2=u["x"].to(T), flow2=u["flow"].to(ft), filt2=u["filt"].to(T), occ0=o.to(T), occ1=(1 - o).to(T))
        out.append(s)
    return out


def _proj_sets(shape, n, T, seed):
    """flow (T), flow32 (what the widened route's autograd keeps), count (the float32 forward's, fillhole = 0), gout (T)"""
    import my_package._ext.my_lib as my_lib
    B, _, H, W = shape
    out = []
    for i in range(n):
        flow = synth.torch_inputs("cuda", B, 1, H, W, flow_kind="smooth", seed=seed + 97 * i)["flow"].to(T)
        g = torch.Generator("cuda").manual_seed(seed + i)
        flow32 = flow.float()
        count, fwd = flow32.new_empty((B, 1, H, W)), torch.empty_like(flow32)
        ws = my_lib.flow_projection_workspace(flow32, 0)
        assert my_lib.FlowProjectionLayer_gpu_forward_ws(flow32, count, fwd, 0, ws) == 0
        out.append({"flow": flow, "flow32": flow32, "count": count,
                    "gout": torch.randn(B, 2, H, W, device="cuda", generator=g).to(T)})
        del fwd, ws
    torch.cuda.synchronize()
    return out


def _dproj_sets(shape, n, T, seed):
    """flow, depth (T), flow32, depth32 (what the widened route's autograd keeps), count and out (the float32 forward's,
    fillhole = 0), gout (T)"""
    import my_package._ext.my_lib as my_lib
    B, _, H, W = shape
    out = []
    for i in range(n):
        flow = synth.torch_inputs("cuda", B, 1, H, W, flow_kind="smooth", seed=seed + 97 * i)["flow"].to(T)
        g = torch.Generator("cuda").manual_seed(seed + i)
        depth = (0.1 + torch.rand(B, 1, H, W, device="cuda", generator=g)).to(T)
        flow32, depth32 = flow.float(), depth.float()
        count, fwd = flow32.new_empty((B, 1, H, W)), torch.empty_like(flow32)
        ws = my_lib.flow_projection_workspace(flow32, 0, depth=True)
        assert my_lib.DepthFlowProjectionLayer_gpu_forward_ws(flow32, depth32, count, fwd, 0, ws) == 0
        out.append({"flow": flow, "depth": depth, "flow32": flow32, "depth32": depth32, "count": count, "out": fwd,
                    "gout": torch.randn(B, 2, H, W, device="cuda", generator=g).to(T)})
        del ws
    torch.cuda.synchronize()
    return out


def _bilinear_sets(shape, n, T, half_flow, seed):
    """x, flow, gout as the network holds them; x32, flow32: what the widened route's autograd keeps"""
    B, C, H, W = shape
    ft = T if half_flow else torch.float32
    out = []
    for i in range(n):
        g = torch.Generator("cuda").manual_seed(seed + i)
        flow = synth.torch_inputs("cuda", B, 1, H, W, flow_kind="smooth", seed=seed + 97 * i)["flow"].to(ft)
        x = torch.rand(B, C, H, W, device="cuda", generator=g).to(T)
        out.append({"x": x, "flow": flow, "x32": x.float(), "flow32": flow.float(),
                    "gout": torch.randn(B, C, H, W, device="cuda", generator=g).to(T)})
    torch.cuda.synchronize()
    return out


def _callers(op, sets, want1):
    from my_package.functions import FilterInterpolationLayer as FL
    from my_package.functions import FilterInterpolationBlendLayer as BL
    state = {"i": 0}

    def pick():
        i = state["i"]
        state["i"] = (i + 1) % len(sets)
        return sets[i]

    if op == "fi":
        def widened():
            s = pick()
            saved = (s["x"], s["flow"], s["filt"])
            x, flow, filt = (t.float().contiguous() for t in saved)
            grads = FL._backward_fp32(x, flow, filt, s["gout"].float().contiguous(), want1)
            return tuple(None if g is None else g.to(t.dtype) for g, t in zip(grads, saved))

        def native():
            s = pick()
            saved = (s["x"], s["flow"], s["filt"])
            grads = FL._backward_lp(*saved, s["gout"], want1)
            assert grads is not None, "not covered"
            return tuple(None if g is None else g.to(t.dtype) for g, t in zip(grads, saved))
    elif op == "mx":
        def widened():                                       # the promoted route
            s = pick()
            saved = (s["x"], s["flow"], s["filt"])
            x, flow, filt = (t.float() for t in saved)
            grads = FL._backward_fp32(x, flow, filt, s["gout"], want1)
            return tuple(None if g is None else g.to(t.dtype) for g, t in zip(grads, saved))

        def native():
            s = pick()
            grads = FL._backward_mx(s["x"], s["flow"], s["filt"], s["gout"], want1)
            assert grads is not None, "not covered"
            return grads
    elif op == "mxblend":
        def widened():                                       # the promoted route of one direction
            s = pick()
            saved = (s["x"], s["flow"], s["filt"], s["occ"])
            grads = BL._direction_grads(tuple(t.float() for t in saved), s["gout"], None, False)
            return tuple(None if g is None else g.to(t.dtype) for g, t in zip(grads, saved))

        def native():
            s = pick()
            grads = BL._direction_backward_fused(s["x"], s["flow"], s["filt"], s["occ"], s["gout"])
            assert grads is not None, "not covered"
            return grads
    elif op == "proj":
        import my_package._ext.my_lib as my_lib
        import my_package._ext.my_lib_lp_proj_grad as my_lib_lp_proj_grad

        def widened():                                       # host_widened's backward
            s = pick()
            gout = s["gout"].float()
            gin = torch.empty_like(s["flow32"])
            assert my_lib.FlowProjectionLayer_gpu_backward(s["flow32"], s["count"], gout, gin) == 0
            return gin.to(s["flow"].dtype)

        def native():
            s = pick()
            gin = torch.empty_like(s["flow"])
            assert my_lib_lp_proj_grad.FlowProjectionLayer_gpu_backward_lp(s["flow"], s["count"], s["gout"], gin) == 0, "not covered"
            return gin
    elif op == "dproj":
        import my_package._ext.my_lib as my_lib
        import my_package._ext.my_lib_lp_dproj_grad as my_lib_lp_dproj_grad

        def widened():                                       # host_widened's backward
            s = pick()
            gout = s["gout"].float()
            g1, g2 = torch.empty_like(s["flow32"]), torch.empty_like(s["depth32"])
            assert my_lib.DepthFlowProjectionLayer_gpu_backward(s["flow32"], s["depth32"], s["count"], s["out"], gout, g1, g2) == 0
            return g1.to(s["flow"].dtype), g2.to(s["depth"].dtype)

        def native():
            s = pick()
            g1, g2 = torch.empty_like(s["flow"]), torch.empty_like(s["depth"])
            assert my_lib_lp_dproj_grad.DepthFlowProjectionLayer_gpu_backward_lp(
                s["flow"], s["depth"], s["count"], s["out"], s["gout"], g1, g2) == 0, "not covered"
            return g1, g2
    elif op == "bl":
        import my_package._ext.my_lib as my_lib
        import my_package._ext.my_lib_lp_bl as my_lib_lp_bl

        def widened():                                       # host_widened's backward
            s = pick()
            gout = s["gout"].float()
            g1, g2 = torch.zeros_like(s["x32"]), torch.empty_like(s["flow32"])
            assert my_lib.InterpolationLayer_gpu_backward(s["x32"], s["flow32"], gout, g1, g2) == 0
            return g1.to(s["x"].dtype), g2.to(s["flow"].dtype)

        def native():
            s = pick()
            g1, g2 = torch.zeros_like(s["x"], dtype=torch.float32), torch.empty_like(s["flow"])
            assert my_lib_lp_bl.InterpolationLayer_gpu_backward_lp(s["x"], s["flow"], s["gout"], g1, g2) == 0, "not covered"
            return g1.to(s["x"].dtype), g2
    elif op == "lpblend":
        def widened():                                       # the composed route of one direction: the layer's default
            s = pick()
            saved = (s["x"], s["flow"], s["filt"], s["occ"])
            grads = BL._direction_grads(tuple(t.float().contiguous() for t in saved), s["gout"].float().contiguous(),
                                        saved[:3], True)
            return tuple(g.to(t.dtype) for g, t in zip(grads, saved))

        def native():
            s = pick()
            grads = BL._direction_backward_fused(s["x"], s["flow"], s["filt"], s["occ"], s["gout"])
            assert grads is not None, "not covered"
            return grads
    else:
        def _blend(half):
            s = pick()
            saved = tuple(s[k] for k in ("x", "x2", "flow", "flow2", "filt", "filt2", "occ0", "occ1"))
            wide = tuple(t.float().contiguous() for t in saved)
            grads = BL._blend_backward(wide, s["gout"].float().contiguous(), half=saved if half else None)
            return tuple(g.to(t.dtype) for g, t in zip(grads, saved))

        def widened():
            return _blend(False)

        def native():
            return _blend(True)
    return {"widened": widened, "native": native}


def run_case(name, op, shape, T, half_flow, want1, rounds, iters):
    B, C, H, W = shape
    per_set = B * H * W * (2 * C + 16 + 2 * 4) * (2 if op == "blend" else 1) * 2        # half bytes, roughly
    if op == "mx":
        per_set = B * H * W * (2 * C * 4 + 16 * 2 + 2 * 4)    # float32 image and gradoutput, half taps
    if op == "mxblend":
        per_set = B * H * W * (2 * C * 4 + 16 * 2 + 2 * 4 + 2)
    if op == "lpblend":
        per_set = B * H * W * (2 * C * 2 + 16 * 2 + 2 * 4 + 2)
    if op == "proj":
        per_set = B * H * W * (2 * 2 + 2 * 4 + 4 + 2 * 2)       # half flow, float32 flow, count, half gradoutput
    if op == "dproj":
        per_set = B * H * W * (3 * 2 + 3 * 4 + 4 + 2 * 4 + 2 * 2)   # half flow and depth, their float32 copies, count, output, half gradoutput
    if op == "bl":
        per_set = B * H * W * (2 * C * (2 + 4) + 2 * 4)         # half image and gradoutput, their float32 copies, the flow
    n = max(2, math.ceil(ROTATE_BYTES / per_set))
    sets = _proj_sets(shape, n, T, seed=2468) if op == "proj" else _dproj_sets(shape, n, T, seed=2468) if op == "dproj" else _bilinear_sets(shape, n, T, half_flow, seed=2468) if op == "bl" else _sets(shape, n, "one" if op in ("mxblend", "lpblend") else op == "blend", T, half_flow, seed=2468,
                 mixed=op in ("mx", "mxblend"))
    calls = _callers(op, sets, want1)
    burst = 10 if op == "bl" and B * H * W < (1 << 21) else 1
    times = {"widened": [], "native": []}
    for _ in range(rounds):
        for route in ("widened", "native"):
            med, _mn = time_launches(calls[route], warmup=2, iters=iters, burst=burst)
            times[route].append(med)
    row = {"case": name, "rounds": rounds, "iters": iters, "input_sets": n, "burst": burst}
    for route in ("widened", "native"):
        ts = times[route]
        m = statistics.median(ts)
        row[route + "_us_per_round"] = [round(t * 1e6, 1) for t in ts]
        row[route + "_us"] = round(m * 1e6, 1)
        row[route + "_spread"] = round((max(ts) - min(ts)) / m, 4)
    row["ratio"] = round(row["native_us"] / row["widened_us"], 3)
    del sets, calls
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default=None, help="run the cases whose name contains this string")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    big = (32, 3, 720, 1280)
    cases = []
    for tname, T in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        for half_flow in (False, True):
            for want1 in (True, False):
                cases.append(("fi_bwd %s 32x3x720x1280 %s flow %s" % (tname, "T" if half_flow else "fp32",
                                                                      "image" if want1 else "noimage"),
                              "fi", big, T, half_flow, want1))
    cases.append(("fi_bwd bf16 8x3x256x448 fp32 flow noimage", "fi", (8, 3, 256, 448), torch.bfloat16, False, False))
    cases.append(("fi_bwd bf16 8x3x256x448 fp32 flow image", "fi", (8, 3, 256, 448), torch.bfloat16, False, True))
    cases.append(("blend_bwd bf16 32x3x720x1280 fp32 flow", "blend", big, torch.bfloat16, False, True))
    # the mixed group: float32 image and gradoutput, half taps; the promoted route against libmemc_hip_mx_grad.so
    for shape in (big, (8, 3, 256, 448)):
        for tname, T in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            for half_flow in (False, True):
                for want1 in (True, False):
                    cases.append(("mixed_bwd %s %s %s flow %s" % (tname, "x".join(map(str, shape)),
                                                                   "T" if half_flow else "fp32",
                                                                   "image" if want1 else "noimage"),
                                  "mx", shape, T, half_flow, want1))
    # the mixed blend group: one direction, frames that are data; the promoted route against libmemc_hip_mx_blend_grad.so
    for shape in (big, (8, 3, 256, 448)):
        for tname, T in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            for half_flow in (False, True):
                cases.append(("mixed_blend_bwd %s %s %s flow" % (tname, "x".join(map(str, shape)),
                                                                 "T" if half_flow else "fp32"),
                              "mxblend", shape, T, half_flow, False))
    # the pure half blend group: one direction, frames that are data; the composed route (the default) against
    # libmemc_hip_lp_blend_grad.so
    for shape in (big, (8, 3, 256, 448)):
        for tname, T in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            for half_flow in (False, True):
                cases.append(("half_blend_bwd %s %s %s flow" % (tname, "x".join(map(str, shape)),
                                                                "T" if half_flow else "fp32"),
                              "lpblend", shape, T, half_flow, False))
    # the half projection group: one FlowProjection backward of a cast model; host_widened's route against
    # libmemc_hip_lp_proj_grad.so
    for shape in ((32, 2, 720, 1280), (8, 2, 256, 448)):
        for tname, T in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            cases.append(("half_proj_bwd %s %s" % (tname, "x".join(map(str, shape))), "proj", shape, T, True, False))
    # the half depth projection group: one DepthFlowProjection backward of a cast model; host_widened's route (the layer
    # with native_half_backward off) against libmemc_hip_lp_dproj_grad.so
    for shape in ((32, 2, 720, 1280), (8, 2, 256, 448)):
        for tname, T in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            cases.append(("half_dproj_bwd %s %s" % (tname, "x".join(map(str, shape))), "dproj", shape, T, True, False))
    # the half bilinear group: one RGB Interpolation backward of a cast model; host_widened's route against
    # libmemc_hip_lp_bl.so
    for shape in (big, (8, 3, 256, 448)):
        for tname, T in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            for half_flow in (False, True):
                cases.append(("half_bilinear_bwd %s %s %s flow" % (tname, "x".join(map(str, shape)),
                                                                   "T" if half_flow else "fp32"),
                              "bl", shape, T, half_flow, True))
    rows = []
    for name, op, shape, T, half_flow, want1 in cases:
        if a.only and a.only not in name:
            continue
        r = run_case(name, op, shape, T, half_flow, want1, a.rounds, a.iters)
        rows.append(r)
        print("%-44s widened %9.1f us (spread %5.1f%%)  native %9.1f us (spread %5.1f%%)  x%.3f" % (
            r["case"], r["widened_us"], 100 * r["widened_spread"], r["native_us"], 100 * r["native_spread"], r["ratio"]))
        print("    per round  widened %s" % r["widened_us_per_round"])
        print("               native  %s" % r["native_us_per_round"], flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
