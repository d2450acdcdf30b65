"""tests/_lp_dproj_cases.py -- the inputs of the fp16 / bf16 depth projection backward's tests
(libmemc_hip_lp_dproj_grad.so), shared by tests/test_lp_dproj_grad_cases.py (the premises, on the CPU) and
tests/test_gpu_lp_dproj_grad.py (the kernel).

Exact cases: every tests/_exact.PB_IDS case through _exact.proj_bwd_inputs(name, True).  Those whose width is a multiple of
four from 8 on are COVERED (the kernel runs), the others DECLINED (return code 1): the split of tests/_lp_proj_cases.py.
`exact_inputs(name, tname)` hands out _exact.proj_bwd_inputs(name, True) as it is wherever its flow is a number of T (the
depth k / 8, the integer gradoutput and the synthetic count and forward output are numbers of T, or float32 by contract,
in every case).  Where the flow is not -- the quarter grid beyond +-63.75 in bf16, beyond +-511.75 in fp16 -- a half
tensor cannot hold it at all, so the case is restated by _exact's own recipe on the flow clipped to what T holds on the
grid (_exact.table_flow(case, storage)), as _lp_proj_cases.exact_inputs does, with the depth operator's draw: the same seed,
the synthetic count +-2^e (e = -2 .. 4, a random sign) where the scatter of THAT flow puts anything and exactly 0 elsewhere,
the same gradoutput rule, the depth k / 8, the forward output k / 4.  No case is dropped for either dtype.

Random cases: flow, depth and gradoutput rounded to T, the depth in [0.1, 1.1); count and forward output come from the
float32 forward (or, on the CPU, the oracle's).
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import _exact as E            # noqa: E402
import _lowp_paths as LP      # noqa: E402
import _lp_proj_cases as PC   # noqa: E402

TNAMES = PC.TNAMES
covered_width = PC.covered_width
is_number_of = PC.is_number_of
COVERED, DECLINED = PC.COVERED, PC.DECLINED        # the split is by the flow's width alone

# (B, H, W, flow kind, sigma, seed): the bit-for-bit cases against the float32 library
#   1x8x8      the minimum width, one partial tile
#   2x20x72    2 x 2 tiles of 64 x 16, partial in both directions, a batch stride
#   1x40x136   an i.i.d. flow of sigma 12: boxes clipped in y, sites gathered from global memory
RANDOM = [(1, 8, 8, "smooth", 2.0, 401), (2, 20, 72, "smooth", 4.0, 402), (1, 40, 136, "iid", 12.0, 403)]
RANDOM_IDS = ["%dx2x%dx%d" % c[:3] for c in RANDOM]
ORDINARY = RANDOM[1]          # the case held to the oracle under tests/_netcalls.rule_rounded


def exact_inputs(name, tname):
    """dict flow, depth, count, fwd_out, gout (float32 numpy; flow, depth and gout numbers of T) of an exact case for
    storage `tname`"""
    h = E.proj_bwd_inputs(name, True)
    if is_number_of(h["flow"], tname):
        return h

    def make():
        assert name in E.TABLE_IDS, "%s: a flow beyond %s that is no table case" % (name, tname)
        flow = E.table_flow(E.TABLE[E.TABLE_IDS.index(name)], tname)
        B, _, H, W = flow.shape
        rng = np.random.default_rng(E._pb_seed(name) + 1)      # proj_bwd_inputs' recipe (with a depth) from here on, on this flow
        hit = E.project_sums(flow)[1] > 0
        e = rng.integers(-2, 5, hit.shape)
        sign = np.where(rng.integers(0, 2, hit.shape) == 1, -1.0, 1.0)
        count = np.where(hit, sign * 2.0 ** e, 0.0).astype(np.float32)
        gout = rng.integers(-E.G, E.G + 1, (B, 2, H, W)).astype(np.float32)
        z = np.flatnonzero(~hit[:, 0])
        g0 = gout[:, 0].copy().reshape(-1)
        g0[z[0::2]] = 0.0
        g0[z[1::2]] = np.where(g0[z[1::2]] == 0, 5.0, g0[z[1::2]])
        gout[:, 0] = g0.reshape(B, H, W)
        depth = E.depth(E._pb_seed(name), B, H, W)
        fwd_out = (rng.integers(-256, 257, (B, 2, H, W)) / 4.0).astype(np.float32)
        return dict(flow=flow, count=count, gout=gout, depth=depth, fwd_out=fwd_out)
    return E._once(("dpb-lp", name, tname), make)


def random_inputs(case, tname):
    """(flow, depth, gout): float32 numpy, numbers of T; the depth in [0.1, 1.1)"""
    from tools import synth
    B, H, W, kind, sigma, seed = case
    rng = np.random.default_rng(seed)
    flow = LP.rounded(synth.np_flow(rng, B, H, W, kind, sigma), tname)
    depth = LP.rounded((0.1 + rng.random((B, 1, H, W))).astype(np.float32), tname)
    gout = LP.rounded(rng.standard_normal((B, 2, H, W)).astype(np.float32), tname)
    return flow, depth, gout
