#!/usr/bin/env python
"""tools/bench_ve.py -- MEMC_Net_VE's rectifier input by its two routes, side by side in one process.

    python tools/bench_ve.py [--rounds 7] [--iters 8] [--out profiles/r24_ve_stack.txt] [--no-network] [--no-resources]

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
(tools/kernel_resources.py)."""
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


def input_set(batch, seed):
    """the seven frames, (flow, taps) of the six neighbours stacked neighbour-major, the seven contexts"""
    t = synth.torch_inputs("cuda", NBR * batch, 3, H, W, flow_kind="smooth", seed=seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    frames = [torch.rand((batch, 3, H, W), device="cuda", generator=g) for _ in range(7)]
    # the contexts as ctxNet returns them in either route: one tensor of the six neighbours' rows and the centre's for the
    # stacked route, and its rows frame by frame (views) for the composed one
    stacked = torch.randn((7 * batch, CTX, H, W), device="cuda", generator=g)
    order = [0, 1, 2, 4, 5, 6, 3]
    contexts = [stacked[order.index(i) * batch:(order.index(i) + 1) * batch] for i in range(7)]
    return frames, t["flow"], t["filt"], contexts, stacked


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-network", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured without one")
    import networks
    lines = ["tools/bench_ve.py --rounds %d --iters %d   (%s, torch %s, %s)" % (
        a.rounds, a.iters, torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d"))]
    net = networks.MEMC_Net_VE(training=False).cuda().eval()
    ratios = []
    with torch.no_grad():
        for batch in (1, 4):
            sets = [input_set(batch, 500 + 10 * batch + i) for i in range(2)]
            state = {"i": 0}

            def route(method, which):
                def call():
                    s = sets[state["i"] % len(sets)]
                    state["i"] += 1
                    return method(s[0], s[1], s[2], s[which])[0]
                return call
            arms = {"composed (12 warps + cat)": route(net._rectifier_input_composed, 3),
                    "stacked (2 stacked warps + centre copies)": route(net._rectifier_input_stacked, 4)}
            s0 = sets[0]                                   # the same set through both routes
            same = torch.equal(net._rectifier_input_composed(s0[0], s0[1], s0[2], s0[3])[0],
                               net._rectifier_input_stacked(s0[0], s0[1], s0[2], s0[4])[0])
            seen = alternate(arms, a.rounds, a.iters)
            lines.append("")
            lines.append("rectifier input, %d x 577 x %d x %d (both routes give the same bits: %s)" % (batch, H, W, same))
            for k, ws in seen.items():
                lines.append("  " + row(k, ws))
            c, s = (statistics.median(ws) for ws in seen.values())
            ratios.append(s / c)
            lines.append("  stacked / composed = %.3f" % (s / c))
            del sets, arms
            torch.cuda.empty_cache()
        if not a.no_network:
            g = torch.Generator(device="cuda").manual_seed(7)
            xs = [torch.rand((1, 3, H, W), device="cuda", generator=g) for _ in range(7)]

            def step(fused):
                def call():
                    net.fused_stack = fused
                    return net(xs)
                return call
            seen = alternate({"fused_stack=False": step(False), "fused_stack=True": step(True)}, a.rounds, max(3, a.iters // 2))
            lines.append("")
            lines.append("one inference step of MEMC_Net_VE, 1 x 320 x 512, random initialisation")
            for k, ws in seen.items():
                lines.append("  " + row(k, ws))
            c, s = (statistics.median(ws) for ws in seen.values())
            lines.append("  fused_stack=True / fused_stack=False = %.3f" % (s / c))
    lines.append("")
    lines.append("stacked faster in every measured group: %s (ratios %s)" % (
        all(r < 1.0 for r in ratios), ", ".join("%.3f" % r for r in ratios)))
    if not a.no_resources:
        from tools import kernel_resources as KR
        lines.append("")
        lines.append("kernel resources of fi_stack.hip (hipcc -Rpass-analysis=kernel-resource-usage; dynamic LDS per workgroup: "
                     "49216 bytes, the tiled forward's)")
        for k in KR.resources_of("fi_stack.hip"):
            lines.append("  %-40s VGPRs %s  SGPRs %s  scratch %s B/lane  occupancy %s waves/SIMD  static LDS %s B" % (
                k["name"][:40], k.get("vgprs"), k.get("sgprs"), k.get("scratch"), k.get("occupancy"), k.get("lds")))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
