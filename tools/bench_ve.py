#!/usr/bin/env python
"""tools/bench_ve.py -- MEMC_Net_VE's rectifier input by its two routes, side by side in one process.

    python tools/bench_ve.py [--rounds 7] [--iters 8] [--out profiles/r24_ve_stack.txt] [--no-network] [--no-resources]
                             [--precision bf16 fp16]

Composed: twelve FilterInterpolationModule calls (six RGB, six on 64 context channels) and the torch.cat's, the reference's
sequence.  Stacked: the rectifier input allocated once, two FilterInterpolationStackModule calls (the contexts; the frames
with the flow and tap pass-through) and the two copies of the centre's context and frame.  Both AS THE NETWORK RUNS THEM,
allocations included, on the same tensors: 1 and 4 septuplets of 320 x 512 (a 256 x 448 Vimeo frame padded as the demo
pads it), flows and taps drawn as tools/synth.py draws them (smooth, sigma 4), the seven context tensors random.  What
both routes share -- the estimators, ctxNet, the rectifier -- is not in these rows.

The two arms run in ALTERNATING windows of --iters calls, --rounds windows each, a device synchronise inside each window;
two input sets alternate between calls.  Per group: the median of the window medians, the spread of either arm (largest
minus smallest window median over the median) and the ratio stacked / composed.  Then one whole-network inference step
(random initialisation, 1 x 320 x 512) under both settings of `fused_stack`, timed the same way, so that the share of
the step is visible; and the registers, LDS and scratch of the stack kernels from the compiler's remarks
(tools/kernel_resources.py).

--precision bf16 fp16: the same for a model cast to that dtype, every tensor in it -- composed is then twelve
libmemc_hip_lp.so warps and the torch.cat's, stacked two libmemc_hip_lp_stack.so launches
(FilterInterpolationStackLayer.native_half, switched on here whatever it ships as) -- per dtype and size.  Each side is also
reported as the smallest and largest window median, and the verdict per group is the one the default of `native_half` rests
on: stacked counts as faster only where the composed median exceeds the stacked one by more than the larger of the two
sides' spreads (largest minus smallest window median)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tools import synth      # noqa: E402

H, W, CTX, NBR = 320, 512, 64, 6


def input_set(batch, seed, dtype=torch.float32):
    """the seven frames, (flow, taps) of the six neighbours stacked neighbour-major, the seven contexts; all of `dtype`"""
    t = synth.torch_inputs("cuda", NBR * batch, 3, H, W, flow_kind="smooth", seed=seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    frames = [torch.rand((batch, 3, H, W), device="cuda", generator=g).to(dtype) for _ in range(7)]
    # the contexts as ctxNet returns them in either route: one tensor of the six neighbours' rows and the centre's for the
    # stacked route, and its rows frame by frame (views) for the composed one
    stacked = torch.randn((7 * batch, CTX, H, W), device="cuda", generator=g).to(dtype)
    order = [0, 1, 2, 4, 5, 6, 3]
    contexts = [stacked[order.index(i) * batch:(order.index(i) + 1) * batch] for i in range(7)]
    return frames, t["flow"].to(dtype), t["filt"].to(dtype), contexts, stacked


def window(fn, iters):
    """median call time of one window, seconds; the window ends in a device synchronise"""
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    torch.cuda.synchronize()
    return statistics.median(ts)


def alternate(arms, rounds, iters, warmup=3):
    """{name: [window medians]} of callables run in alternating windows"""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    seen = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            seen[k].append(window(fn, iters))
    return seen


def row(name, ws):
    med = statistics.median(ws)
    return "%-44s %9.1f us   spread %4.1f %%   (windows: %s)" % (name, med * 1e6, 100.0 * (max(ws) - min(ws)) / med,
                                                             " ".join("%.0f" % (w * 1e6) for w in ws))


def verdict(composed, stacked):
    """(stacked faster by more than the larger spread, the line that says so) of two lists of window medians"""
    c, s = statistics.median(composed), statistics.median(stacked)
    spread = max(max(composed) - min(composed), max(stacked) - min(stacked))
    won = c - s > spread
    return won, ("  composed %.0f..%.0f us, stacked %.0f..%.0f us (smallest..largest window median); composed - stacked = "
                 "%.1f us against a larger spread of %.1f us: stacked %s" % (
                     min(composed) * 1e6, max(composed) * 1e6, min(stacked) * 1e6, max(stacked) * 1e6, (c - s) * 1e6,
                     spread * 1e6, "FASTER" if won else "NOT faster by more than the spread"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-network", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--precision", nargs="+", default=[], choices=["bf16", "fp16"],
                    help="measure a model cast to these dtypes instead of the float32 one")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured without one")
    import networks
    lines = ["tools/bench_ve.py --rounds %d --iters %d%s   (%s, torch %s, %s)" % (
        a.rounds, a.iters, " --precision " + " ".join(a.precision) if a.precision else "", torch.cuda.get_device_name(0),
        torch.__version__, time.strftime("%Y-%m-%d"))]
    from my_package.functions.FilterInterpolationStackLayer import FilterInterpolationStackLayer
    half = {"bf16": torch.bfloat16, "fp16": torch.float16}
    ships = FilterInterpolationStackLayer.native_half
    FilterInterpolationStackLayer.native_half = True       # the route under measurement, whatever the default is
    ratios, verdicts = [], []
    for tname in a.precision or ["fp32"]:
        dtype = half.get(tname, torch.float32)
        tag = "" if dtype == torch.float32 else "%s: " % tname
        net = networks.MEMC_Net_VE(training=False).cuda().to(dtype).eval()
        with torch.no_grad():
            for batch in (1, 4):
                sets = [input_set(batch, 500 + 10 * batch + i, dtype) for i in range(2)]
                state = {"i": 0}

                def route(method, which):
                    def call():
                        s = sets[state["i"] % len(sets)]
                        state["i"] += 1
                        return method(s[0], s[1], s[2], s[which])[0]
                    return call
                arms = {"composed (12 warps + cat)": route(net._rectifier_input_composed, 3),
                        "stacked (2 stacked warps + centre copies)": route(net._rectifier_input_stacked, 4)}
                s0 = sets[0]                               # the same set through both routes
                same = torch.equal(net._rectifier_input_composed(s0[0], s0[1], s0[2], s0[3])[0],
                                   net._rectifier_input_stacked(s0[0], s0[1], s0[2], s0[4])[0])
                seen = alternate(arms, a.rounds, a.iters)
                lines.append("")
                lines.append("%srectifier input, %d x 577 x %d x %d (both routes give the same bits: %s)" % (tag, batch, H, W, same))
                for k, ws in seen.items():
                    lines.append("  " + row(k, ws))
                c, s = (statistics.median(ws) for ws in seen.values())
                ratios.append(s / c)
                lines.append("  stacked / composed = %.3f" % (s / c))
                if a.precision:
                    won, text = verdict(*seen.values())
                    verdicts.append(("%s, %d septuplet%s" % (tname, batch, "s" if batch > 1 else ""), won))
                    lines.append(text)
                del sets, arms
                torch.cuda.empty_cache()
            if not a.no_network:
                g = torch.Generator(device="cuda").manual_seed(7)
                xs = [torch.rand((1, 3, H, W), device="cuda", generator=g).to(dtype) for _ in range(7)]

                def step(fused):
                    def call():
                        net.fused_stack = fused
                        return net(xs)
                    return call
                seen = alternate({"fused_stack=False": step(False), "fused_stack=True": step(True)}, a.rounds,
                                 max(3, a.iters // 2))
                lines.append("")
                lines.append("%sone inference step of MEMC_Net_VE, 1 x 320 x 512, random initialisation%s" % (
                    tag, " (not a criterion)" if a.precision else ""))
                for k, ws in seen.items():
                    lines.append("  " + row(k, ws))
                c, s = (statistics.median(ws) for ws in seen.values())
                lines.append("  fused_stack=True / fused_stack=False = %.3f" % (s / c))
        del net
        torch.cuda.empty_cache()
    FilterInterpolationStackLayer.native_half = ships
    lines.append("")
    lines.append("stacked faster in every measured group: %s (ratios %s)" % (
        all(r < 1.0 for r in ratios), ", ".join("%.3f" % r for r in ratios)))
    if a.precision:
        lost = [name for name, won in verdicts if not won]
        lines.append("stacked faster by more than the larger spread in every group: %s%s -> native_half = %s" % (
            not lost, "" if not lost else " (lost: %s)" % "; ".join(lost), not lost))
    unit = "lp_fi_stack.hip" if a.precision else "fi_stack.hip"
    if not a.no_resources:
        from tools import kernel_resources as KR
        lines.append("")
        lines.append("kernel resources of %s (hipcc -Rpass-analysis=kernel-resource-usage; dynamic LDS per workgroup: "
                     "49216 bytes, the tiled forward's)" % unit)
        for k in KR.resources_of(unit):
            lines.append("  %-64s VGPRs %s  SGPRs %s  scratch %s B/lane  occupancy %s waves/SIMD  static LDS %s B" % (
                k["name"][:64], k.get("vgprs"), k.get("sgprs"), k.get("scratch"), k.get("occupancy"), k.get("lds")))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
