"""What the tests of the stacked half-precision adaptive warp share (tests/test_gpu_lp_stack.py): the shapes with the paths
each must reach, the channel layout of `out`, and a stub enhancer that takes half planes.  The shapes, the census cases and
the path expectations are those of tests/test_gpu_stack.py's SHAPES, restated (no test module imports another); the census
runs on the flow as rounded to the storage under test."""
import numpy as np
import torch

import _lowp_paths as LP
from tools import synth

N, B = 6, 2                                # neighbours, batch elements
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}

# name -> (H, W, the census case whose flow kind, sigma and seed are used, what tests/_lowp_paths.census must report)
SHAPES = {
    "20x72-smooth": (20, 72, LP.CASES[4], dict(one_band=True, empty=True, invalid=True, mixed=True)),
    "20x72-iid": (20, 72, LP.CASES[5], dict(one_band=True, invalid=True, mixed=True)),
    "16x8": (16, 8, LP.CASES[4], dict(one_band=True, empty=True, invalid=True)),
    "96x256-bands": (96, 256, LP.CASES[0], dict(bands=True, capped=True, slow=True, split=True, invalid=True)),
    "112x320-slow": (112, 320, LP.CASES[2], dict(bands=True, capped=True, slow=True, split=True, invalid=True)),
}
PATH = {3: "fi_fwd_stack_lp:tiled_c3", 8: "fi_fwd_stack_lp:tiled_c4n"}
LP_PATH = {3: "fi_fwd_lp:tiled_c3", 8: "fi_fwd_lp:tiled_c4n"}

_CACHE = {}


def once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def inputs(name, C):
    """(image [12, C, H, W], flow, taps) as fp32 numpy, the flow drawn first as the census cases draw theirs; never written"""
    def make():
        H, W, (_b, _h, _w, kind, sigma, seed), _paths = SHAPES[name]
        rng = np.random.default_rng(seed)
        flow = synth.np_flow(rng, N * B, H, W, kind, sigma)
        return synth.np_image(rng, N * B, C, H, W), flow, synth.np_filter(rng, N * B, H, W)
    return once(("inputs", name, C), make)


def check_census(name, tname):
    """the paths the flow AS ROUNDED TO `tname` reaches (the half grid is unshifted: the census is the kernel's own)"""
    c = once(("census", name, tname), lambda: LP.census(LP.rounded(inputs(name, 3)[1], tname)))
    want = SHAPES[name][3]
    print(name, tname, c)
    assert c["valid"] > 0
    if want.get("one_band"):
        assert c["max_bands_run"] == 1 and c["nbx_gt1"] == 0 and c["nby_gt1"] == 0 and c["slow"] == 0
    if want.get("bands"):
        assert c["nbx_gt1"] > 0 and c["nby_gt1"] > 0 and c["max_bands_run"] > 1
    if want.get("capped"):
        assert c["capped"] > 0
    if want.get("slow"):
        assert c["slow"] > 0
    if want.get("split"):
        assert c["split_lanes"] > 0
    if want.get("empty"):
        assert c["empty"] > 0
    if want.get("invalid"):
        assert c["valid"] < c["sites"]
    if want.get("mixed"):
        assert c["mixed_lanes"] > 0
    return c


class Layout:
    """channel layout of `out`: a gap, the warps (with or without the centre's slot), a gap, the flows, a gap, the taps, a gap"""

    def __init__(self, C, skip, passthrough=True):
        self.C, self.skip = C, skip
        slots = N + (1 if skip >= 0 else 0)
        self.c_base = 1
        self.flow_base = self.c_base + slots * C + 2 if passthrough else -1
        self.tap_base = self.flow_base + 2 * N + 1 if passthrough else -1
        self.ctot = (self.tap_base + 16 * N + 3) if passthrough else self.c_base + slots * C + 2

    def slot(self, n):
        return n + (1 if 0 <= self.skip <= n else 0)

    def warp(self, n):
        return slice(self.c_base + self.slot(n) * self.C, self.c_base + (self.slot(n) + 1) * self.C)

    def flow(self, n):
        return slice(self.flow_base + 2 * n, self.flow_base + 2 * n + 2)

    def taps(self, n):
        return slice(self.tap_base + 16 * n, self.tap_base + 16 * n + 16)

    def args(self):
        return (N, self.c_base, self.skip, self.flow_base, self.tap_base)


def ff_filled(dtype, *shape):
    """a float16 / bfloat16 tensor of `shape` whose every byte is 0xFF"""
    return torch.full(shape[:-1] + (2 * shape[-1],), 0xFF, dtype=torch.uint8, device="cuda").view(dtype)


def all_ff(t):
    return bool((t.contiguous().view(torch.int16) == -1).all())


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def check_out(out, lay, want, flow, taps):
    """written slots == want's rows, pass-through == the bits of flow.to(T) / taps, every other channel still 0xFF bytes"""
    touched = torch.zeros(out.size(1), dtype=torch.bool)
    for n in range(N):
        rows = slice(n * B, (n + 1) * B)
        assert torch.equal(out[:, lay.warp(n)], want[rows]), "neighbour %d" % n
        touched[lay.warp(n)] = True
        if lay.flow_base >= 0:
            assert same_bits(out[:, lay.flow(n)], flow[rows].to(out.dtype)), "flow %d" % n
            assert same_bits(out[:, lay.taps(n)], taps[rows]), "taps %d" % n
            touched[lay.flow(n)] = True
            touched[lay.taps(n)] = True
    rest = out[:, (~touched).nonzero().flatten().cuda()]
    assert rest.size(1) >= 3 + (lay.C if lay.skip >= 0 else 0)
    assert all_ff(rest), "a channel outside the written slices was touched"


class HalfStubEnhancer(torch.nn.Module):
    """tests/_septuplets.StubEnhancer's arithmetic on planes of `dtype` (that stub insists on float32): the same single
    operations in the same order whichever way the planes were made, so equal planes give equal bytes"""

    def __init__(self, dtype):
        super().__init__()
        self.dtype, self.shapes = dtype, []

    def forward(self, xs, y=None):
        assert len(xs) == 7 and all(x.shape == xs[0].shape and x.dtype == self.dtype for x in xs)
        self.shapes.append(tuple(xs[0].shape))
        h, w = xs[0].shape[2:]
        ramp = ((torch.arange(w)[None, :] + 2 * torch.arange(h)[:, None]) % 16).to(torch.float32) / 64
        return (xs[3] * 0.5 + xs[2] * 0.25 + xs[4] * 0.25) * 1.25 - 0.125 + ramp.to(xs[0].device, self.dtype)
