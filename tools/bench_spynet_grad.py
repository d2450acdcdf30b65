#!/usr/bin/env python
"""tools/bench_spynet_grad.py -- a SPyNet pyramid level's forward + backward by its two training routes, side by side in one
process.

    python tools/bench_spynet_grad.py [--rounds 7] [--iters 12] [--out profiles/r27_spynet_level_backward.txt]
                                      [--no-network] [--no-resources]

Parent route (`SPyNet.fused_level_backward = False`, the default): a level whose coarse flow wants a gradient runs the torch
expression (interpolate x2, doubled, replicate pad, normalise, grid, grid_sample, cat: nine or ten ATen launches) and
torch's autograd through it, about twice that backward.  Native route (`fused_level_backward = True`): one launch of
libmemc_hip_spynet.so forward and one of libmemc_hip_spynet_grad.so backward (plus the slice / contiguous copy autograd
asks for).  Both AS THE NETWORK RUNS THEM, through `SPyNet.level_input`, allocations included, on the same tensors, batch 1:

  * forward + backward of one level input at every level size of the pyramids of a 256 x 448 frame (16 x 28 ... 256 x 448)
    and of a 768 x 1344 frame (24 x 42 ... 768 x 1344): frames that are data, a smooth coarse flow of sigma 4 that requires
    a gradient, a fixed dense gradoutput;
  * a whole SPyNet forward + backward (loss: mean |flow|) at both sizes;
  * one MEMC_Net_s training step (forward, the sum of the mean absolute losses, backward) at 256 x 448.

The two arms run in ALTERNATING windows of --iters calls, --rounds windows each, a device synchronise inside each window; two
input sets alternate between calls.  Per group: the median of the window medians, the spread of either arm, the ratio
native / parent, and whether native is faster by more than the larger of the two sides' spreads (tools/bench_ve.verdict).
The verdict line says whether that holds in EVERY group.  `SPyNet.fused_level_backward` stays False whatever it says (the
default training route is pinned by the existing tests); this file is what a later change of the default rests on.  Then
the registers, LDS and scratch of the kernel from the compiler's remarks (tools/kernel_resources.py)."""
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

from tools.bench_spynet import SIZES, level_set, level_sizes      # noqa: E402
from tools.bench_ve import alternate, row, verdict                # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-network", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured without one")
    import networks
    from networks._spynet import SPyNet
    lines = ["tools/bench_spynet_grad.py --rounds %d --iters %d   (%s, torch %s, %s)" % (
        a.rounds, a.iters, torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d"))]
    lines.append("max |native - parent| below: the warp's derivative jumps where a sample position crosses an integer; at the large "
                 "levels a few sites lie within fp32 rounding of one and two fp32 routes take different sides there, which moves a "
                 "cell's gradient by about a pixel difference (torch's own float32 and float64 autograd through the torch "
                 "expression differ by 1.25 in 4 of 57344 cells at 256 x 448, 3e-5 at 64 x 112).  tests/test_gpu_spynet_level_bwd.py "
                 "holds the kernel to the float64 rule on cases without such sites.")
    spy = SPyNet().cuda().eval()
    criteria = []                                          # (group, native faster by more than the larger spread, ratio)

    def group(title, arms, iters):
        seen = alternate(arms, a.rounds, iters)
        lines.append("")
        lines.append(title)
        for k, ws in seen.items():
            lines.append("  " + row(k, ws))
        p, n = (statistics.median(ws) for ws in seen.values())
        lines.append("  native / parent = %.3f" % (n / p))
        won, text = verdict(*seen.values())
        lines.append(text.replace("composed", "parent").replace("stacked", "native"))
        criteria.append((title, won, n / p))

    def rotating(fn, sets):
        state = {"i": 0}

        def call():
            s = sets[state["i"] % len(sets)]
            state["i"] += 1
            return fn(*s)
        return call

    def level_step(native):
        def fn(first, second, coarse, g):
            spy.fused_level_backward = native
            coarse.grad = None
            out = spy.level_input(first, second, coarse)
            assert ("SpyNetLevelFunction" in type(out.grad_fn).__name__) == native
            out.backward(g)
            return coarse.grad
        return fn

    for h, w in SIZES:
        for lh, lw in level_sizes(h, w):
            sets = []
            for i in range(2):
                first, second, coarse = level_set(lh, lw, 700 + i)
                g = torch.randn((1, 8, lh, lw), device="cuda", generator=torch.Generator(device="cuda").manual_seed(900 + i))
                sets.append((first, second, coarse.requires_grad_(True), g / 4.0))
            parent = level_step(False)(*sets[0]).clone()
            native = level_step(True)(*sets[0]).clone()
            diff, scale = float((native - parent).abs().max()), float(parent.abs().max())
            group("level input %d x %d of the %d x %d pyramid, forward + backward, batch 1 (max |native - parent| of the coarse "
                  "gradient = %.2g of %.2g)" % (lh, lw, h, w, diff, scale),
                  {"parent (torch expression, autograd)": rotating(level_step(False), sets),
                   "native (one launch each way)": rotating(level_step(True), sets)}, a.iters)
            del sets

    def spynet_step(native):
        def fn(x0, x1):
            spy.fused_level_backward = native
            spy.zero_grad(set_to_none=True)
            spy(x0, x1).abs().mean().backward()
        return fn

    for h, w in SIZES:
        gen = torch.Generator(device="cuda").manual_seed(h)
        sets = [tuple(torch.rand((1, 3, h, w), device="cuda", generator=gen) for _ in range(2)) for _ in range(2)]
        group("whole SPyNet forward + backward, 1 x 3 x %d x %d, random initialisation" % (h, w),
              {"fused_level_backward=False": rotating(spynet_step(False), sets),
               "fused_level_backward=True": rotating(spynet_step(True), sets)}, max(3, a.iters // 2))
        del sets
        spy.zero_grad(set_to_none=True)
        torch.cuda.empty_cache()
    if not a.no_network:
        h, w = SIZES[0]
        net = networks.MEMC_Net_s(training=False).cuda().eval()
        gen = torch.Generator(device="cuda").manual_seed(7)
        x = torch.rand((3, 1, 3, h, w), device="cuda", generator=gen)

        def train_step(native):
            def call():
                net.flownets.fused_level_backward = native
                net.zero_grad(set_to_none=True)
                net.training = True            # the class's own flag; the sub-modules stay in eval mode
                try:
                    losses = net(x)[0]
                    sum(l.abs().mean() for l in losses).backward()
                finally:
                    net.training = False
            return call
        group("one training step of MEMC_Net_s, 1 x %d x %d, random initialisation" % (h, w),
              {"fused_level_backward=False": train_step(False), "fused_level_backward=True": train_step(True)},
              max(3, a.iters // 2))
    lost = [t for t, won, _r in criteria if not won]
    lines.append("")
    lines.append("native faster by more than the larger spread in every group: %s (ratios %s)" % (
        not lost, ", ".join("%.3f" % r for _t, _w, r in criteria)))
    for t in lost:
        lines.append("  not faster beyond the spread: " + t)
    lines.append("-> SPyNet.fused_level_backward stays False (the default training route is pinned by the existing tests); "
                 "this file is what a change of the default would rest on.")
    lines.append("")
    lines.append("not measured: the kernel alone under a profiler, batches above 1, tile sizes other than 16 x 16, a training step "
                 "of MEMC_Net_s at 768 x 1344, a captured graph of the step, an optimiser step, any route with a gradient for "
                 "`second` (it keeps the torch expression).")
    if not a.no_resources:
        from tools import kernel_resources as KR
        lines.append("")
        lines.append("kernel resources of spynet_level_bwd.hip (hipcc -Rpass-analysis=kernel-resource-usage; no scratch)")
        for k in KR.resources_of("spynet_level_bwd.hip"):
            lines.append("  %-64s VGPRs %s  SGPRs %s  scratch %s B/lane  occupancy %s waves/SIMD  LDS %s B" % (
                k["name"][:64], k.get("vgprs"), k.get("sgprs"), k.get("scratch"), k.get("occupancy"), k.get("lds")))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
