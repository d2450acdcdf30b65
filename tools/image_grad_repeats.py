#!/usr/bin/env python
"""tools/image_grad_repeats.py -- the RGB adaptive-warp backward's image gradient, repeated in ONE process: how far the fp32
kernel (libmemc_hip.so) and the half kernel (libmemc_hip_lp_grad.so) land from the float64 restatement of the operation,
measured in units of the derived per-cell bound (tests/_image_grad.py), run after run.

    python tools/image_grad_repeats.py [--reps 150] [--cases 2] [--tnames fp16] [--limit 300] [--lib PATH] [--json out.json]

Per case of tests/_lowp_paths.CASES, dtype and storage combination (flow and gradoutput in T or float32) it makes the inputs
and the restatement once, then repeats: the fp32 kernel twice and the half kernel once on the same tensors.  Recorded:
  * cells beyond the bound, per kernel (expected: 0), and the largest err / bound of any run;
  * the distribution of err / bound over all cells and repetitions (mean, median, 99th centile, maximum), per kernel;
  * what the earlier rule saw (both results rounded to T, at most one ulp_T apart everywhere, 99.9 % equal): the number of
    repetitions it fails for "fp32 twice" and for "half against fp32", and the largest distance in ulp_T;
  * the share of cells whose fp32 bits differ between the two fp32 runs, and between the half run and the first fp32 run.
The whole run is under one time limit (--limit seconds: SIGALRM ends the process); nothing is retried.  --lib loads another
build of libmemc_hip_lp_grad.so (a scratch build with a deliberate defect: the mutation table of
profiles/lowp_paths_observed.md).  It is a measurement, not a test: it asserts nothing and exits 0 unless a call fails.
"""
import argparse
import json
import os
import signal
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _image_grad as IG     # noqa: E402
import _lowp_paths as LP     # noqa: E402

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
MANT = {"fp16": (10, -14), "bf16": (7, -126)}
EDGES = [0.0, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0, float("inf")]


def ulp(v, tname):
    mant, emin = MANT[tname]
    _, e = torch.frexp(v)
    return torch.ldexp(torch.ones_like(v), torch.clamp(e - 1, min=emin) - mant)


def old_rule(a, b, tname):
    """(largest distance in ulp_T after rounding to T, share of equal elements)"""
    T = DTYPES[tname]
    ra, rb = a.to(T).float(), b.to(T).float()
    d = (ra - rb).abs() / ulp(torch.maximum(ra.abs(), rb.abs()), tname)
    return float(d.max()), float((ra == rb).float().mean())


class Spread:
    """err / bound over cells and repetitions: a histogram on EDGES, the count beyond 1 and the largest value"""

    def __init__(self):
        self.hist = torch.zeros(len(EDGES) - 1, dtype=torch.float64)
        self.total, self.sum, self.beyond, self.max = 0, 0.0, 0, 0.0

    def add(self, r):
        self.hist += torch.histogram(r.cpu(), bins=torch.tensor(EDGES[:-1] + [1e300], dtype=torch.float64))[0]
        self.total += r.numel()
        self.sum += float(r.sum())
        self.beyond += int((r > 1).sum())
        self.max = max(self.max, float(r.max()))

    def centile(self, q):
        """upper edge of the histogram bin that holds the q-th centile"""
        c = torch.cumsum(self.hist, 0) / max(self.total, 1)
        return EDGES[1:][int((c >= q).nonzero()[0])]

    def row(self):
        return dict(mean=self.sum / max(self.total, 1), median_below=self.centile(0.5), p99_below=self.centile(0.99),
                    max=self.max, beyond=self.beyond, cells_times_reps=self.total,
                    hist={("<= %g" % e): int(n) for e, n in zip(EDGES[1:], self.hist.tolist())})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=150)
    ap.add_argument("--cases", default="2", help="indices into tests/_lowp_paths.CASES, comma separated, or 'all'")
    ap.add_argument("--tnames", default="fp16")
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    signal.alarm(args.limit)                                   # one limit for the whole run

    import my_package._ext.my_lib as F32
    import my_package._ext.my_lib_lp_grad as LPG
    if args.lib:
        LPG._SAT.path = os.path.abspath(args.lib)
    print("half library: %s (%s)" % (LPG._SAT.path, LPG.version()))
    cases = range(len(LP.CASES)) if args.cases == "all" else [int(c) for c in args.cases.split(",")]
    rows = []
    for ci in cases:
        for tname in args.tnames.split(","):
            T = DTYPES[tname]
            x, flow, filt, gout = LP.case_inputs(LP.CASES[ci], 3)
            for flow_T, gout_T in ((True, True), (False, False), (True, False), (False, True)):
                dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dt)      # noqa: E731
                tx, tf, tk, tg = dev(x, T), dev(flow, T if flow_T else torch.float32), dev(filt, T), dev(gout, T if gout_T else torch.float32)
                ref = IG.Reference(tf, tk, tg)
                want = torch.from_numpy(ref.want).cuda()
                bound = torch.from_numpy(ref.bound()).cuda()
                live = torch.from_numpy(np.ascontiguousarray(ref.live)).cuda()
                wide = [t.float().contiguous() for t in (tx, tf, tk, tg)]

                def fp32_run():
                    g1, g2, g3 = torch.zeros_like(wide[0]), torch.empty_like(wide[1]), torch.empty_like(wide[2])
                    assert F32.FilterInterpolationLayer_gpu_backward(*wide, g1, g2, g3) == 0
                    return g1

                def half_run():
                    g1 = torch.zeros_like(wide[0])
                    g2, g3 = torch.empty_like(tf), torch.empty_like(tk)
                    assert LPG.FilterInterpolationLayer_gpu_backward_lp(tx, tf, tk, tg, g1, g2, g3) == 0
                    return g1

                def ratio(g):
                    return ((g.double() - want).abs() / bound)[live]

                spread = {"fp32": Spread(), "half": Spread()}
                old = {"fp32 twice": [0, 0.0], "half vs fp32": [0, 0.0]}
                bits = {"fp32 twice": 0.0, "half vs fp32": 0.0}
                runs_beyond = {"fp32": 0, "half": 0}
                for _ in range(args.reps):
                    a1, b1, h1 = fp32_run(), fp32_run(), half_run()
                    torch.cuda.synchronize()
                    for name, gs in (("fp32", (a1, b1)), ("half", (h1,))):
                        for g in gs:
                            r = ratio(g)
                            spread[name].add(r)
                            runs_beyond[name] += int(bool((r > 1).any()))
                    for name, (p, q) in (("fp32 twice", (a1, b1)), ("half vs fp32", (h1, a1))):
                        d, same = old_rule(p, q, tname)
                        old[name][0] += int(d > 1 or same < 0.999)
                        old[name][1] = max(old[name][1], d)
                        bits[name] += float((p != q).float().mean()) / args.reps
                row = dict(case=LP.CASE_IDS[ci], tname=tname, flow="T" if flow_T else "fp32", gradoutput="T" if gout_T else "fp32",
                           reps=args.reps, live_cells=int(live.sum()), bound_max=float(bound[live].max()),
                           runs_beyond_bound=runs_beyond, old_rule_failures={k: v[0] for k, v in old.items()},
                           old_rule_max_ulp={k: v[1] for k, v in old.items()}, differing_fp32_bits=bits,
                           err_over_bound={k: v.row() for k, v in spread.items()})
                rows.append(row)
                e = row["err_over_bound"]
                print("%s %s flow %s gout %s, %d reps: beyond the bound fp32 %d of %d runs, half %d of %d (max err / bound %.3f | %.3f; "
                      "mean %.4f | %.4f; 99 %% below %g | %g); old rule fails fp32 twice %d (max %.3g ulp_T), half vs fp32 %d (max %.3g); "
                      "cells with different fp32 bits: fp32 twice %.4f, half vs fp32 %.4f"
                      % (row["case"], tname, row["flow"], row["gradoutput"], args.reps, runs_beyond["fp32"], 2 * args.reps,
                         runs_beyond["half"], args.reps, e["fp32"]["max"], e["half"]["max"], e["fp32"]["mean"], e["half"]["mean"],
                         e["fp32"]["p99_below"], e["half"]["p99_below"], old["fp32 twice"][0], old["fp32 twice"][1],
                         old["half vs fp32"][0], old["half vs fp32"][1], bits["fp32 twice"], bits["half vs fp32"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
