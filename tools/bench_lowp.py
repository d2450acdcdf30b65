#!/usr/bin/env python
"""tools/bench_lowp.py -- fp32 / fp16 / bf16 adaptive warps side by side, in one process.

    python tools/bench_lowp.py [--rounds 3] [--iters 10] [--json out.json]

Cases: FilterInterpolation forward 32x3x720x1280 (smooth flow; fp32 flow and half flow), the fused dual warp + occlusion
blend 32x3x720x1280, and FilterInterpolation forward 8x64x720x1280 (the context warp).  Each case times fp32 (libmemc_hip.so),
fp16 and bf16 (libmemc_hip_lp.so) ALTERNATELY, round after round, so that clock and thermal drift fall on all three alike;
every launch rotates over enough input sets to cycle more than 1 GB, as bench.py does (no set fits the 256 MiB Infinity
Cache).  Printed per row: median launch time over the rounds, algorithmic bytes per site and per launch, TB/s, the fraction
of the 8 TB/s HBM peak and the ratio of the time to fp32's."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    cases = [("fi_fwd 32x3x720x1280 fp32 flow", "fi", (32, 3, 720, 1280), False),
             ("fi_fwd 32x3x720x1280 half flow", "fi", (32, 3, 720, 1280), True),
             ("blend 32x3x720x1280", "blend", (32, 3, 720, 1280), False),
             ("fi_fwd 8x64x720x1280", "fi", (8, 64, 720, 1280), False)]
    rows = []
    for name, op, shape, half_flow in cases:
        for r in run_case(name, op, shape, half_flow, a.rounds, a.iters):
            rows.append(r)
            print("%-32s %-5s flow %-8s %9.1f us  %3d B/site  %6.3f TB/s  %.3f of 8 TB/s  x%.3f vs fp32" % (
                r["case"], r["dtype"], r["flow"], r["us"], r["bytes_per_site"], r["TBps"], r["frac_8TBps"],
                r["ratio_to_fp32"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
