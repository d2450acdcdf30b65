#!/usr/bin/env python
"""tools/bench_lowp.py -- fp32 / fp16 / bf16 adaptive warps side by side, in one process.

    python tools/bench_lowp.py [--rounds 3] [--iters 10] [--json out.json] [--only lowp|mixed|bilinear]

Cases: FilterInterpolation forward 32x3x720x1280 (smooth flow; fp32 flow and half flow), the fused dual warp + occlusion
blend 32x3x720x1280, and FilterInterpolation forward 8x64x720x1280 (the context warp).  Each case times fp32 (libmemc_hip.so),
fp16 and bf16 (libmemc_hip_lp.so) ALTERNATELY, round after round, so that clock and thermal drift fall on all three alike;
every launch rotates over enough input sets to cycle more than 1 GB, as bench.py does (no set fits the 256 MiB Infinity
Cache).  Printed per row: median launch time over the rounds, algorithmic bytes per site and per launch, TB/s, the fraction
of the 8 TB/s HBM peak and the ratio of the time to fp32's.

Mixed rows (--only mixed, or after the others): the call torch.autocast makes -- fp32 frames, fp16 / bf16 taps and occlusions,
the flow in fp32 or that dtype -- on the RGB warp and the fused blend at 8x3x256x448 and 32x3x720x1280, each AS THE LAYER RUNS
IT, allocations included: `mixed` (libmemc_hip_mx.so on the tensors as they are) against `promoted` (the .to(float32) casts of
taps, occlusions and half flows, then libmemc_hip.so: the layers' route before that library existed), and for the blend
`fp32` (libmemc_hip.so on fp32 inputs, for orientation).  The arms run in ALTERNATING windows of 8 timed launches (bursts of
10 for the small shape), six windows each; per row the median of the window medians, the spread (largest minus smallest
window median) and the bytes per site the route moves.

Bilinear rows (--only bilinear; not part of a run without --only): the forward of InterpolationLayer / InterpolationChLayer for
a model cast to fp16 / bf16, AS THE LAYER RUNS IT, casts and allocations included: `widened` (_common.host_widened: the image
and a half flow cast to float32, libmemc_hip.so, the output cast back -- the layers' only route before libmemc_hip_lp_bl.so)
against `native` (libmemc_hip_lp_bl.so on the tensors as they are), at 32x3x720x1280, 8x3x256x448 and 8x64x720x1280, both
dtypes, both flow storages.  The two alternate in windows (--rounds of them, at least seven; bursts of 10 launches for the
small shape), a device synchronise inside each; per group the median of the window medians, the spread of either side
(largest minus smallest window median over the median) and the ratio native / widened."""
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

HBM_PEAK_BPS = 8.0e12
ROTATE_BYTES = 1 << 30


def _bytes_per_site(op, C, t, flow):
    """algorithmic bytes per output site: every tensor element read or written once"""
    e, f = t.itemsize, flow.itemsize
    if op == "fi":
        return C * e + 2 * f + 16 * e + C * e
    return 2 * (C * e + 2 * f + 16 * e) + 2 * e + C * e          # blend: two warps' inputs, two occlusions, one output


def _sets(B, C, H, W, n, blend, seed):
    out = []
    for i in range(n):
        t = synth.torch_inputs("cuda", B, C, H, W, flow_kind="smooth", seed=seed + 97 * i)
        s = {"x": t["x"], "flow": t["flow"], "filt": t["filt"]}
        if blend:
            u = synth.torch_inputs("cuda", B, C, H, W, flow_kind="smooth", seed=seed + 97 * i + 1)
            s.update(x2=u["x"], flow2=u["flow"], filt2=u["filt"])
            o = torch.rand(B, 1, H, W, device="cuda", generator=torch.Generator("cuda").manual_seed(seed + i))
            s.update(occ0=o, occ1=1 - o)
        out.append(s)
    return out


def _cast(s, dt, flow_dt):
    return {k: v.to(flow_dt if k.startswith("flow") else dt).contiguous() for k, v in s.items()}


def _caller(op, sets):
    import my_package._ext.my_lib as my_lib
    import my_package._ext.my_lib_lp as my_lib_lp
    lp = sets[0]["x"].dtype != torch.float32
    outs = [torch.empty_like(s["x"]) for s in sets]
    state = {"i": 0}

    def call():
        i = state["i"]
        state["i"] = (i + 1) % len(sets)
        s, o = sets[i], outs[i]
        if op == "fi":
            f = my_lib_lp.FilterInterpolationLayer_gpu_forward_lp if lp else my_lib.FilterInterpolationLayer_gpu_forward
            err = f(s["x"], s["flow"], s["filt"], o)
        else:
            f = (my_lib_lp.FilterInterpolationBlendLayer_gpu_forward_lp if lp
                 else my_lib.FilterInterpolationBlendLayer_gpu_forward)
            err = f(s["x"], s["x2"], s["flow"], s["flow2"], s["filt"], s["filt2"], s["occ0"], s["occ1"], o)
        if err != 0:
            raise RuntimeError("%s returned %d" % (op, err))

    return call


def run_case(name, op, shape, half_flow, rounds, iters):
    B, C, H, W = shape
    sites = B * H * W
    fp32_set_bytes = sites * _bytes_per_site(op, C, torch.empty(0), torch.empty(0))
    n = max(2, math.ceil(ROTATE_BYTES / (fp32_set_bytes / 2)))       # the half sets are about half as large
    base = _sets(B, C, H, W, n, op == "blend", seed=4321)
    variants = [("fp32", torch.float32, torch.float32)]
    for tname, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        variants.append((tname, dt, dt if half_flow else torch.float32))
    sets = {v[0]: ([_cast(s, v[1], v[2]) for s in base] if v[1] != torch.float32 else base) for v in variants}
    calls = {v[0]: _caller(op, sets[v[0]]) for v in variants}
    times = {v[0]: [] for v in variants}
    for _ in range(rounds):
        for tname, _dt, _ft in variants:
            med, _mn = time_launches(calls[tname], warmup=3, iters=iters)
            times[tname].append(med)
    rows = []
    t32 = statistics.median(times["fp32"])
    for tname, dt, ft in variants:
        t = statistics.median(times[tname])
        bps = _bytes_per_site(op, C, torch.empty(0, dtype=dt), torch.empty(0, dtype=ft))
        alg = bps * sites
        rows.append({"case": name, "dtype": tname, "flow": str(ft).replace("torch.", ""), "us": round(t * 1e6, 1),
                     "bytes_per_site": bps, "alg_bytes": alg, "TBps": round(alg / t / 1e12, 3),
                     "frac_8TBps": round(alg / t / HBM_PEAK_BPS, 4), "ratio_to_fp32": round(t / t32, 3),
                     "input_sets": n, "rounds": rounds})
    del sets, base, calls
    torch.cuda.empty_cache()
    return rows


# ---- mixed precision: fp32 frames beside half taps ---------------------------------------------------------------------
def mixed_bytes_per_site(op, route, half_flow):
    """bytes a route moves per site, from the layouts: (casts, kernel)"""
    f = 2 if half_flow else 4
    if op == "fi":
        if route == "mixed":
            return 0, 12 + 2 * f + 32 + 12
        casts = 16 * (2 + 4) + (2 * (2 + 4) if half_flow else 0)
        return casts, 96
    if route == "mixed":
        return 0, 24 + 4 * f + 64 + 4 + 12
    if route == "fp32":
        return 0, 188
    casts = 2 * 16 * (2 + 4) + 2 * (2 + 4) + (4 * (2 + 4) if half_flow else 0)
    return casts, 188


def _mixed_arm(op, route, sets):
    import my_package._ext.my_lib as my_lib
    import my_package._ext.my_lib_mx as my_lib_mx
    state = {"i": 0}
    names = ("x", "flow", "filt") if op == "fi" else ("x", "x2", "flow", "flow2", "filt", "filt2", "occ0", "occ1")
    f32 = my_lib.FilterInterpolationLayer_gpu_forward if op == "fi" else my_lib.FilterInterpolationBlendLayer_gpu_forward
    mx = (my_lib_mx.FilterInterpolationLayer_gpu_forward_mx if op == "fi"
          else my_lib_mx.FilterInterpolationBlendLayer_gpu_forward_mx)

    def call():
        i = state["i"]
        state["i"] = (i + 1) % len(sets)
        args = [sets[i][n] for n in names]
        out = torch.empty_like(args[0])                      # the layer allocates its output per call
        if route == "mixed":
            err = mx(*args, out)
        else:                                                # promoted: the casts are per-call allocations and passes
            err = f32(*[a.to(torch.float32) for a in args], out)
        if err != 0:
            raise RuntimeError("%s %s returned %d" % (op, route, err))

    return call


def run_mixed(shape, windows=6, iters=8):
    B, C, H, W = shape
    sites = B * H * W
    burst = 10 if sites < (1 << 21) else 1
    n = max(2, math.ceil(ROTATE_BYTES / (sites * 112)))
    base = _sets(B, C, H, W, n, True, seed=8765)
    rows = []
    for op in ("fi", "blend"):
        for tname, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            for half_flow in (False, True):
                ft = dt if half_flow else torch.float32
                mixed_sets = [{k: (v if k.startswith("x") else v.to(ft if k.startswith("flow") else dt).contiguous())
                               for k, v in s.items()} for s in base]
                arms = [("mixed", mixed_sets), ("promoted", mixed_sets)] + ([("fp32", base)] if op == "blend" else [])
                calls = {r: _mixed_arm(op, r, ss) for r, ss in arms}
                meds = {r: [] for r, _ in arms}
                for _ in range(windows):
                    for r, _ss in arms:
                        med, _mn = time_launches(calls[r], warmup=2, iters=iters, burst=burst)
                        meds[r].append(med)
                for r, _ss in arms:
                    casts, kern = mixed_bytes_per_site(op, r, half_flow)
                    t = statistics.median(meds[r])
                    rows.append({"case": "%s %dx%dx%dx%d" % (op, B, C, H, W), "taps": tname,
                                 "flow": str(ft).replace("torch.", ""), "route": r, "us": round(t * 1e6, 1),
                                 "windows_us": [round(m * 1e6, 1) for m in meds[r]],
                                 "spread_us": round((max(meds[r]) - min(meds[r])) * 1e6, 1),
                                 "bytes_per_site": casts + kern, "cast_bytes_per_site": casts,
                                 "TBps_moved": round((casts + kern) * sites / t / 1e12, 3), "input_sets": n, "burst": burst})
                    print("%-22s %-4s flow %-8s %-8s %9.1f us  spread %5.1f us  %3d B/site (%3d casts)  %6.3f TB/s moved"
                          "   windows: %s" % (rows[-1]["case"], tname, rows[-1]["flow"], r, rows[-1]["us"],
                                              rows[-1]["spread_us"], casts + kern, casts, rows[-1]["TBps_moved"],
                                              " ".join("%.1f" % w for w in rows[-1]["windows_us"])), flush=True)
                m, p = rows[-len(arms)], rows[-len(arms) + 1]
                print("    mixed / promoted: x%.3f (%.1f us saved, larger spread %.1f us)" % (
                    m["us"] / p["us"], p["us"] - m["us"], max(m["spread_us"], p["spread_us"])), flush=True)
                del mixed_sets, calls
                torch.cuda.empty_cache()
    del base
    torch.cuda.empty_cache()
    return rows


# ---- the bilinear warp of a cast model: host_widened against libmemc_hip_lp_bl.so -----------------------------------------
def bilinear_bytes_per_site(route, C, half_flow):
    """bytes a route moves per site, from the layouts: (casts, kernel)"""
    f = 2 if half_flow else 4
    if route == "native":
        return 0, 2 * C + 2 * f + 2 * C
    casts = C * (2 + 4) + (2 * (2 + 4) if half_flow else 0) + C * (4 + 2)      # image and half flow widened, output narrowed
    return casts, 4 * C + 8 + 4 * C


def _bilinear_arm(route, C, sets):
    import my_package._ext.my_lib as my_lib
    import my_package._ext.my_lib_lp_bl as my_lib_lp_bl
    which = "InterpolationLayer_gpu_forward" if C == 3 else "InterpolationChLayer_gpu_forward"
    f32, lp = getattr(my_lib, which), getattr(my_lib_lp_bl, which + "_lp")
    state = {"i": 0}

    def call():
        i = state["i"]
        state["i"] = (i + 1) % len(sets)
        x, flow = sets[i]
        if route == "native":
            out = torch.empty_like(x)
            err = lp(x, flow, out)
        else:                                                # host_widened: the casts are per-call allocations and passes
            x32, flow32 = x.float(), flow.float()
            wide = torch.empty_like(x32)
            err = f32(x32, flow32, wide)
            out = wide.to(x.dtype)
        if err != 0:
            raise RuntimeError("bilinear %s returned %d" % (route, err))
        return out

    return call


def run_bilinear(shape, rounds, iters):
    B, C, H, W = shape
    sites = B * H * W
    burst = 10 if sites < (1 << 21) else 1
    n = max(2, math.ceil(ROTATE_BYTES / (sites * (2 * C + 4))))
    rows = []
    for tname, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
        for half_flow in (False, True):
            ft = dt if half_flow else torch.float32
            sets = []
            for i in range(n):
                g = torch.Generator("cuda").manual_seed(9753 + i)
                flow = synth.torch_inputs("cuda", B, 1, H, W, flow_kind="smooth", seed=9753 + 97 * i)["flow"].to(ft)
                sets.append((torch.rand(B, C, H, W, device="cuda", generator=g).to(dt), flow))
            calls = {r: _bilinear_arm(r, C, sets) for r in ("widened", "native")}
            meds = {r: [] for r in calls}
            for _ in range(max(rounds, 7)):
                for r in ("widened", "native"):
                    med, _mn = time_launches(calls[r], warmup=2, iters=iters, burst=burst)
                    meds[r].append(med)
            group = {}
            for r in ("widened", "native"):
                casts, kern = bilinear_bytes_per_site(r, C, half_flow)
                t = statistics.median(meds[r])
                group[r] = {"case": "bilinear_fwd %dx%dx%dx%d" % shape, "dtype": tname, "flow": str(ft).replace("torch.", ""),
                            "route": r, "us": round(t * 1e6, 1), "windows_us": [round(m * 1e6, 1) for m in meds[r]],
                            "spread": round((max(meds[r]) - min(meds[r])) / t, 4), "bytes_per_site": casts + kern,
                            "cast_bytes_per_site": casts, "TBps_moved": round((casts + kern) * sites / t / 1e12, 3),
                            "input_sets": n, "burst": burst}
                rows.append(group[r])
            w, nv = group["widened"], group["native"]
            nv["ratio"] = round(nv["us"] / w["us"], 3)
            print("%-30s %-4s flow %-8s widened %9.1f us (spread %5.1f%%, %3d B/site)  native %9.1f us (spread %5.1f%%, %3d B/site)"
                  "  x%.3f" % (w["case"], tname, w["flow"], w["us"], 100 * w["spread"], w["bytes_per_site"], nv["us"],
                               100 * nv["spread"], nv["bytes_per_site"], nv["ratio"]))
            print("    per window  widened %s" % w["windows_us"])
            print("                native  %s" % nv["windows_us"], flush=True)
            del sets, calls
            torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("lowp", "mixed", "bilinear"), default=None,
                    help="the half rows, the mixed rows or the bilinear rows alone")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    cases = [("fi_fwd 32x3x720x1280 fp32 flow", "fi", (32, 3, 720, 1280), False),
             ("fi_fwd 32x3x720x1280 half flow", "fi", (32, 3, 720, 1280), True),
             ("blend 32x3x720x1280", "blend", (32, 3, 720, 1280), False),
             ("fi_fwd 8x64x720x1280", "fi", (8, 64, 720, 1280), False)]
    rows = []
    if a.only == "bilinear":
        for shape in ((32, 3, 720, 1280), (8, 3, 256, 448), (8, 64, 720, 1280)):
            rows += run_bilinear(shape, a.rounds, a.iters)
        cases = []
    for name, op, shape, half_flow in ([] if a.only == "mixed" else cases):
        for r in run_case(name, op, shape, half_flow, a.rounds, a.iters):
            rows.append(r)
            print("%-32s %-5s flow %-8s %9.1f us  %3d B/site  %6.3f TB/s  %.3f of 8 TB/s  x%.3f vs fp32" % (
                r["case"], r["dtype"], r["flow"], r["us"], r["bytes_per_site"], r["TBps"], r["frac_8TBps"],
                r["ratio_to_fp32"]), flush=True)
    if a.only in (None, "mixed"):
        for shape in ((8, 3, 256, 448), (32, 3, 720, 1280)):
            rows += run_mixed(shape)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
