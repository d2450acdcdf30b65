#!/usr/bin/env python
"""tools/bench_spynet.py -- SPyNet's pyramid-level input by its two routes, side by side in one process.

    python tools/bench_spynet.py [--rounds 7] [--iters 12] [--out profiles/r26_spynet_level.txt] [--no-network] [--no-resources]
                                 [--precision bf16 fp16]

Composed: the torch expression (interpolate x2, doubled, replicate pad where the size is odd, normalise, add the linspace
grid, permute, grid_sample, torch.cat), the reference's sequence: nine or ten ATen launches.  Fused: one launch of
libmemc_hip_spynet.so (my_package.modules.SpyNetLevelModule).  Both AS THE NETWORK RUNS THEM, through `SPyNet.level_input`,
allocations included, on the same tensors, batch 1:

  * the level input alone at every level of the pyramids of a 256 x 448 frame (16 x 28 ... 256 x 448) and of a 768 x 1344
    frame (24 x 42 ... 768 x 1344), frames drawn like preprocessed frames, a smooth coarse flow of sigma 4;
  * the whole SPyNet forward (pyramid, level inputs, the 7 x 7 convolution stacks) at both sizes;
  * one MEMC_Net_s inference step at 256 x 448 (not a criterion: it shows the share of the step).

The two arms run in ALTERNATING windows of --iters calls, --rounds windows each, a device synchronise inside each window; two
input sets alternate between calls.  Per group: the median of the window medians, the spread of either arm and the ratio
fused / composed, and the verdict `SPyNet.fused_level`'s default rests on: fused counts as faster only where the composed
median exceeds the fused one by more than the larger of the two sides' spreads (largest minus smallest window median).  The
default is True only if that holds in EVERY group of the level-input and whole-SPyNet measurements.  Then the registers, LDS
and scratch of the two kernels from the compiler's remarks (tools/kernel_resources.py).

--precision bf16 fp16: the same groups for a model and inputs cast to that dtype, per dtype.  Composed is then the torch
expression on half tensors (what a cast model runs while `SPyNet.fused_level_half` is False, as it ships), fused one launch
of libmemc_hip_spynet_lp.so (`fused_level_half = True`, switched on here whatever it ships as).  The two routes do not
compute the same values -- the torch expression rounds its sampling grid and normalised flow to the half dtype, the kernel
forms the position in float32 -- so the accuracy of both is recorded as well, per dtype, for the 256 x 448 level with a
N(0, 4^2) coarse flow: the largest and the mean absolute error of the warped frame out[:, 3:6] against the float64 rule
(tests/_spynet_spec.level) on the same half-representable inputs, and against that reference rounded once to the dtype
(the best a half result can do).  No threshold applies to either."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tools.bench_ve import alternate, row, verdict      # noqa: E402

SIZES = ((256, 448), (768, 1344))


def level_sizes(h, w):
    """the pyramid's level sizes, coarsest first (SPyNet.pyramid's rule)"""
    sizes = [(h, w)]
    for _ in range(5):
        if sizes[0][0] > 32 or sizes[0][1] > 32:
            sizes.insert(0, (sizes[0][0] // 2, sizes[0][1] // 2))
    return sizes


def level_set(h, w, seed):
    """(first, second, coarse) of one level: frames like preprocessed frames, a smooth coarse flow of sigma 4"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    first = (torch.rand((1, 3, h, w), device="cuda", generator=g) - 0.45) / 0.225
    second = (torch.rand((1, 3, h, w), device="cuda", generator=g) - 0.45) / 0.225
    ch, cw = h // 2, w // 2
    knots = torch.randn((1, 2, max(2, ch // 8 + 1), max(2, cw // 8 + 1)), device="cuda", generator=g)
    coarse = 4.0 * F.interpolate(knots, size=(ch, cw), mode="bicubic", align_corners=True)
    return first, second, coarse.contiguous()


def accuracy(spy, dtype, h, w):
    """the 256 x 448 level with a N(0, 4^2) coarse flow on inputs representable in `dtype`: per route (max, mean) absolute
    error of out[:, 3:6] against the float64 rule, and the same for that reference rounded once to `dtype`"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _spynet_spec as S
    g = torch.Generator(device="cuda").manual_seed(2800)
    first = ((torch.rand((1, 3, h, w), device="cuda", generator=g) - 0.45) / 0.225).to(dtype)
    second = ((torch.rand((1, 3, h, w), device="cuda", generator=g) - 0.45) / 0.225).to(dtype)
    coarse = (4.0 * torch.randn((1, 2, h // 2, w // 2), device="cuda", generator=g)).to(dtype)
    case = tuple(t.float().cpu().numpy().astype(np.float64) for t in (first, second, coarse))
    want = torch.from_numpy(S.level(*case, int(spy.align_upsample), int(spy.align_sample), np.float64)[:, 3:6])
    seen = {}
    for name, on in (("composed (torch expression on half tensors)", False), ("fused (libmemc_hip_spynet_lp.so)", True)):
        spy.fused_level_half = on
        err = (spy.level_input(first, second, coarse)[:, 3:6].double().cpu() - want).abs()
        seen[name] = (float(err.max()), float(err.mean()))
    err = (want.to(dtype).double() - want).abs()
    seen["the float64 reference rounded once"] = (float(err.max()), float(err.mean()))
    return seen


def main_half(a):
    """--precision: the groups of main() for a cast model, composed half route against the half kernel, and the accuracy"""
    import networks
    from networks._spynet import SPyNet
    import my_package._ext.my_lib_spynet_lp as LPLIB
    half = {"bf16": torch.bfloat16, "fp16": torch.float16}
    lines = ["tools/bench_spynet.py --rounds %d --iters %d --precision %s   (%s, torch %s, %s)" % (
        a.rounds, a.iters, " ".join(a.precision), torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d"))]
    lines.append("composed: SPyNet.fused_level_half = False (as it ships: the torch expression on half tensors); fused: True "
                 "(one launch of %s).  SPyNet.fused_level is True throughout." % LPLIB.version())
    criteria, table = [], []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for tname in a.precision:
        dtype = half[tname]
        spy = SPyNet().cuda().to(dtype).eval()

        def group(title, arms, iters, criterion=True):
            seen = alternate(arms, a.rounds, iters)
            say("")
            say("%s: %s" % (tname, title))
            for k, ws in seen.items():
                say("  " + row(k, ws))
            c, f = (statistics.median(ws) for ws in seen.values())
            say("  fused / composed = %.3f" % (f / c))
            won, text = verdict(*seen.values())
            say(text.replace("stacked", "fused"))
            if criterion:
                criteria.append(("%s: %s" % (tname, title), won, f / c))

        def route(fn, on, sets, owner):
            state = {"i": 0}

            def call():
                owner.fused_level_half = on
                s = sets[state["i"] % len(sets)]
                state["i"] += 1
                return fn(*s)
            return call

        with torch.no_grad():
            for h, w in SIZES:
                for lh, lw in level_sizes(h, w):
                    sets = [tuple(t.to(dtype) for t in level_set(lh, lw, 700 + i)) for i in range(2)]
                    spy.fused_level_half = True
                    fused = spy.level_input(*sets[0])
                    path = LPLIB.last_kernel_path()
                    spy.fused_level_half = False
                    diff = float((fused.float() - spy.level_input(*sets[0]).float()).abs().max())
                    group("level input %d x %d of the %d x %d pyramid, batch 1 (%s; max |fused - composed| = %.2g)" % (
                              lh, lw, h, w, path, diff),
                          {"composed (torch expression)": route(spy.level_input, False, sets, spy),
                           "fused (one launch)": route(spy.level_input, True, sets, spy)}, a.iters)
                    del sets
            for h, w in SIZES:
                g = torch.Generator(device="cuda").manual_seed(h)
                sets = [tuple(torch.rand((1, 3, h, w), device="cuda", generator=g).to(dtype) for _ in range(2)) for _ in range(2)]
                group("whole SPyNet forward, 1 x 3 x %d x %d, random initialisation" % (h, w),
                      {"fused_level_half=False": route(spy, False, sets, spy), "fused_level_half=True": route(spy, True, sets, spy)},
                      max(3, a.iters // 2))
                del sets
                torch.cuda.empty_cache()
            if not a.no_network:
                h, w = SIZES[0]
                net = networks.MEMC_Net_s(training=False).cuda().to(dtype).eval()
                g = torch.Generator(device="cuda").manual_seed(7)
                x = torch.rand((2, 1, 3, h, w), device="cuda", generator=g).to(dtype)
                group("one inference step of MEMC_Net_s, 1 x %d x %d, random initialisation (not a criterion)" % (h, w),
                      {"fused_level_half=False": route(net, False, [(x,)], net.flownets),
                       "fused_level_half=True": route(net, True, [(x,)], net.flownets)}, max(3, a.iters // 2), criterion=False)
                del net
                torch.cuda.empty_cache()
            table.append((tname, accuracy(spy, dtype, *SIZES[0])))
        del spy
    lost = [t for t, won, _r in criteria if not won]
    say("")
    say("fused faster by more than the larger spread in every level-input and whole-SPyNet group: %s (ratios %s)" % (
        not lost, ", ".join("%.3f" % r for _t, _w, r in criteria)))
    for t in lost:
        say("  lost: " + t)
    say("(no speed-up is required of this route, and SPyNet.fused_level_half ships False whatever this says: it changes the "
        "values a cast model computes)")
    say("")
    say("accuracy of the warped frame out[:, 3:6], level 256 x 448, coarse flow N(0, 4^2), inputs representable in the dtype; "
        "absolute error against the float64 rule (tests/_spynet_spec.level, np.float64); no threshold applies")
    for tname, seen in table:
        for name, (worst, mean) in seen.items():
            say("  %-5s %-46s max %.4g   mean %.4g" % (tname, name, worst, mean))
    say("")
    say("not measured: the kernels alone under a profiler, batches above 1, a training step (half calls that want a gradient "
        "keep the torch expression), an LDS-staged source box (not written), MEMC_Net_s at 768 x 1344, the accuracy at other "
        "sizes or flow magnitudes, the effect on a trained model's interpolation error.")
    if not a.no_resources:
        from tools import kernel_resources as KR
        say("")
        say("kernel resources of lp_spynet_level.hip (hipcc -Rpass-analysis=kernel-resource-usage; no LDS, no scratch)")
        for k in KR.resources_of("lp_spynet_level.hip"):
            say("  %-64s VGPRs %s  SGPRs %s  scratch %s B/lane  occupancy %s waves/SIMD  LDS %s B" % (
                k["name"][:64], k.get("vgprs"), k.get("sgprs"), k.get("scratch"), k.get("occupancy"), k.get("lds")))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-network", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--precision", nargs="+", default=[], choices=["bf16", "fp16"],
                    help="measure a model cast to these dtypes (composed half route against libmemc_hip_spynet_lp.so) "
                         "instead of the float32 one")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: nothing here is measured without one")
    if a.precision:
        return main_half(a)
    import networks
    from networks._spynet import SPyNet
    lines = ["tools/bench_spynet.py --rounds %d --iters %d   (%s, torch %s, %s)" % (
        a.rounds, a.iters, torch.cuda.get_device_name(0), torch.__version__, time.strftime("%Y-%m-%d"))]
    spy = SPyNet().cuda().eval()
    criteria = []                                          # (group, fused faster by more than the larger spread)

    def group(title, arms, iters, criterion=True):
        seen = alternate(arms, a.rounds, iters)
        lines.append("")
        lines.append(title)
        for k, ws in seen.items():
            lines.append("  " + row(k, ws))
        c, f = (statistics.median(ws) for ws in seen.values())
        lines.append("  fused / composed = %.3f" % (f / c))
        won, text = verdict(*seen.values())
        lines.append(text.replace("stacked", "fused"))
        if criterion:
            criteria.append((title, won, f / c))

    def route(fn, fused, sets):
        state = {"i": 0}

        def call():
            spy.fused_level = fused
            s = sets[state["i"] % len(sets)]
            state["i"] += 1
            return fn(*s)
        return call

    with torch.no_grad():
        for h, w in SIZES:
            for lh, lw in level_sizes(h, w):
                sets = [level_set(lh, lw, 700 + i) for i in range(2)]
                spy.fused_level = True
                fused = spy.level_input(*sets[0])
                spy.fused_level = False
                diff = float((fused - spy.level_input(*sets[0])).abs().max())
                group("level input %d x %d of the %d x %d pyramid, batch 1 (max |fused - composed| = %.2g)" % (lh, lw, h, w, diff),
                      {"composed (torch expression)": route(spy.level_input, False, sets),
                       "fused (one launch)": route(spy.level_input, True, sets)}, a.iters)
                del sets
        for h, w in SIZES:
            g = torch.Generator(device="cuda").manual_seed(h)
            sets = [tuple(torch.rand((1, 3, h, w), device="cuda", generator=g) for _ in range(2)) for _ in range(2)]
            group("whole SPyNet forward, 1 x 3 x %d x %d, random initialisation" % (h, w),
                  {"fused_level=False": route(spy, False, sets), "fused_level=True": route(spy, True, sets)},
                  max(3, a.iters // 2))
            del sets
            torch.cuda.empty_cache()
        if not a.no_network:
            h, w = SIZES[0]
            net = networks.MEMC_Net_s(training=False).cuda().eval()
            g = torch.Generator(device="cuda").manual_seed(7)
            x = torch.rand((2, 1, 3, h, w), device="cuda", generator=g)

            def step(fused):
                def call():
                    net.flownets.fused_level = fused
                    return net(x)
                return call
            group("one inference step of MEMC_Net_s, 1 x %d x %d, random initialisation (not a criterion)" % (h, w),
                  {"fused_level=False": step(False), "fused_level=True": step(True)}, max(3, a.iters // 2), criterion=False)
    lost = [t for t, won, _r in criteria if not won]
    lines.append("")
    lines.append("fused faster by more than the larger spread in every level-input and whole-SPyNet group: %s (ratios %s)" % (
        not lost, ", ".join("%.3f" % r for _t, _w, r in criteria)))
    for t in lost:
        lines.append("  lost: " + t)
    lines.append("-> SPyNet.fused_level = %s" % (not lost))
    lines.append("")
    lines.append("not measured: the kernels alone under a profiler, batches above 1, a training step (only its coarsest level, whose inputs "
                 "want no gradient, reaches the kernel), an LDS-staged source box (not written: the gathers go to global memory), "
                 "MEMC_Net_s at 768 x 1344.")
    if not a.no_resources:
        from tools import kernel_resources as KR
        lines.append("")
        lines.append("kernel resources of spynet_level.hip (hipcc -Rpass-analysis=kernel-resource-usage; no LDS, no scratch)")
        for k in KR.resources_of("spynet_level.hip"):
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
