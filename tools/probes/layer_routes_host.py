#!/usr/bin/env python
"""tools/probes/layer_routes_host.py -- what one forward + backward of the two warp layers costs on the wall clock at
1x3x128x128, where the kernels take a few microseconds and the layers' Python decides: one row per precision route of
FilterInterpolationLayer and FilterInterpolationBlendLayer (float32, bfloat16, mixed; frames that are data, and "+image":
frames that want a gradient; fused_half_backward).  300 calls between two synchronisations, seven rounds.  The first two
rows run twice: a process's first second is slower on any tree.

    python tools/probes/layer_routes_host.py [TREE]      # TREE: the checkout to import my_package from (default: this one)

To compare two checkouts, alternate them in one session on one card."""
import os
import sys
import time

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else \
    os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "memc-net_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from my_package.functions.FilterInterpolationBlendLayer import FilterInterpolationBlendLayer  # noqa: E402
from my_package.functions.FilterInterpolationLayer import FilterInterpolationLayer  # noqa: E402
import my_package.functions.FilterInterpolationLayer as FL  # noqa: E402

assert os.path.abspath(FL.__file__).startswith(ROOT), FL.__file__
dev = torch.device("cuda:0")
g = torch.Generator(device="cpu").manual_seed(3)
B, H, W = 1, 128, 128


def rnd(c, dtype, grad, scale=1.0):
    t = (torch.rand(B, c, H, W, generator=g) * scale).to(dev).to(dtype)
    return t.requires_grad_(grad)


def warp_case(idt, tdt, image_grad):
    x, f, k = rnd(3, idt, image_grad), rnd(2, torch.float32, True, 3.0), rnd(16, tdt, True)
    go = rnd(3, idt, False)
    layer = FilterInterpolationLayer()

    def step():
        for t in (x, f, k):
            t.grad = None
        layer(x, f, k).backward(go)
    return step


def blend_case(idt, tdt, image_grad, **kw):
    a = [rnd(3, idt, image_grad), rnd(3, idt, image_grad), rnd(2, torch.float32, True, 3.0), rnd(2, torch.float32, True, 3.0),
         rnd(16, tdt, True), rnd(16, tdt, True), rnd(1, tdt, True), rnd(1, tdt, True)]
    go = rnd(3, idt, False)
    layer = FilterInterpolationBlendLayer(**kw)

    def step():
        for t in a:
            t.grad = None
        layer(*a).backward(go)
    return step


f32, bf = torch.float32, torch.bfloat16
cases = [("warp f32", warp_case(f32, f32, False)), ("warp f32 +image", warp_case(f32, f32, True)),
         ("warp bf16", warp_case(bf, bf, False)), ("warp bf16 +image", warp_case(bf, bf, True)),
         ("warp mixed", warp_case(f32, bf, False)),
         ("blend f32", blend_case(f32, f32, False)), ("blend f32 +image", blend_case(f32, f32, True)),
         ("blend mixed", blend_case(f32, bf, False)), ("blend mixed +image", blend_case(f32, bf, True)),
         ("blend bf16", blend_case(bf, bf, False)),
         ("blend bf16 fused", blend_case(bf, bf, False, fused_half_backward=True)),
         ("blend bf16 fused +image", blend_case(bf, bf, True, fused_half_backward=True))]
N = 300
for name, step in cases[:2] + cases:          # the first two again: what a cold start does to them is seen apart
    for _ in range(30):
        step()
    rounds = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(N):
            step()
        torch.cuda.synchronize()
        rounds.append((time.perf_counter() - t0) / N * 1e6)
    rounds.sort()
    print("%-26s min %7.1f  median %7.1f  max %7.1f us" % (name, rounds[0], rounds[3], rounds[-1]), flush=True)
