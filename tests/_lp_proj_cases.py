"""tests/_lp_proj_cases.py -- the inputs of the fp16 / bf16 projection backward's tests (libmemc_hip_lp_proj_grad.so), shared
by tests/test_lp_proj_grad_cases.py (the premises, on the CPU) and tests/test_gpu_lp_proj_grad.py (the kernel).

Exact cases: every tests/_exact.PB_IDS case.  Those whose width is a multiple of four from 8 on are COVERED (the kernel
runs), the others DECLINED (return code 1).  `exact_inputs(name, tname)` hands out tests/_exact.proj_bwd_inputs(name,
False) as it is wherever its flow is a number of T.  Where it is not -- the quarter grid beyond +-63.75 in bf16, beyond
+-511.75 in fp16: five cases in bf16, one in fp16 -- a half tensor cannot hold that flow at all, so the case is restated by
_exact's own recipe on the flow clipped to what T holds on the grid (_exact.table_flow(case, storage), as the warps' exact
cases do): the same seed, the synthetic count +-2^e where the scatter of THAT flow puts anything and exactly 0 elsewhere,
the same gradoutput rule.  No case is dropped for either dtype.

Random cases: flows and gradoutputs rounded to T; the count comes from the float32 forward (or, on the CPU, the oracle's).
"""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import _exact as E            # noqa: E402
import _lowp_paths as LP      # noqa: E402
from tools import synth       # noqa: E402

TNAMES = ("fp16", "bf16")


def covered_width(W):
    return W % 4 == 0 and W >= 8


def _width(name):
    return E.pb_flow(name).shape[3]


COVERED = [n for n in E.PB_IDS if covered_width(_width(n))]
DECLINED = [n for n in E.PB_IDS if not covered_width(_width(n))]

# (B, H, W, flow kind, sigma, seed): the bit-for-bit cases against the float32 library
#   1x8x8      the minimum width, one partial tile
#   2x20x72    2 x 2 tiles of 64 x 16, partial in both directions, a batch stride
#   1x40x136   an i.i.d. flow of sigma 12: boxes clipped in y, sites gathered from global memory
RANDOM = [(1, 8, 8, "smooth", 2.0, 301), (2, 20, 72, "smooth", 4.0, 302), (1, 40, 136, "iid", 12.0, 303)]
RANDOM_IDS = ["%dx2x%dx%d" % c[:3] for c in RANDOM]
ORDINARY = RANDOM[1]          # the case held to the oracle under tests/_netcalls.rule_rounded


def is_number_of(a, tname):
    return bool((LP.rounded(a, tname) == np.asarray(a, dtype=np.float32)).all())


def exact_inputs(name, tname):
    """dict flow, count, gout (float32 numpy; flow and gout numbers of T) of an exact case for storage `tname`"""
    h = E.proj_bwd_inputs(name, False)
    if is_number_of(h["flow"], tname):
        return h

    def make():
        assert name in E.TABLE_IDS, "%s: a flow beyond %s that is no table case" % (name, tname)
        flow = E.table_flow(E.TABLE[E.TABLE_IDS.index(name)], tname)
        B, _, H, W = flow.shape
        rng = np.random.default_rng(E._pb_seed(name))          # proj_bwd_inputs' recipe from here on, on this flow
        hit = E.project_sums(flow)[1] > 0
        e = rng.integers(0, 5, hit.shape)
        count = np.where(hit, 2.0 ** e, 0.0).astype(np.float32)
        gout = rng.integers(-E.G, E.G + 1, (B, 2, H, W)).astype(np.float32)
        z = np.flatnonzero(~hit[:, 0])
        g0 = gout[:, 0].copy().reshape(-1)
        g0[z[0::2]] = 0.0
        g0[z[1::2]] = np.where(g0[z[1::2]] == 0, 5.0, g0[z[1::2]])
        gout[:, 0] = g0.reshape(B, H, W)
        return dict(flow=flow, count=count, gout=gout, depth=None, fwd_out=None)
    return E._once(("pb-lp", name, tname), make)


def random_inputs(case, tname):
    """(flow, gout): float32 numpy, numbers of T"""
    B, H, W, kind, sigma, seed = case
    rng = np.random.default_rng(seed)
    flow = LP.rounded(synth.np_flow(rng, B, H, W, kind, sigma), tname)
    gout = LP.rounded(rng.standard_normal((B, 2, H, W)).astype(np.float32), tname)
    return flow, gout
