"""The RGB adaptive-warp forward on its shifted tile grid (fi_fwd_tiled_fs4 with XOFF = 32: tile tx covers the sites
[64 tx - 32, 64 tx + 32)), which the launcher takes when the image's and the filter's rows are a multiple of 1 KiB
(DESIGN.md section 3).  GPU only.

Every case runs on three layouts of the same values: contiguous, rows padded to a multiple of 256 floats (the shifted
grid, whatever the width) and rows of such a multiple plus 64 floats (the plain grid), against the oracle with
tests/_parity.py's rule.  Padded rows also show that no lane of the shifted grid stores outside the view: the padding
must come back untouched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _parity as P                        # noqa: E402
from tools import synth                    # noqa: E402

pytestmark = pytest.mark.gpu

PAD = 123.0


def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a GPU: the HIP path cannot be exercised (no fallback exists)")
    return torch.device("cuda:0")


def _up(n, m):
    return (n + m - 1) // m * m


def _pitches(W):
    """row strides in floats: contiguous, a multiple of 256 (1 KiB), and one that is not"""
    return {"contiguous": W, "rows of n KiB": _up(W, 256), "rows of n KiB + 256 B": _up(W, 256) + 64}


def _view(a, pitch):
    """numpy [B, ch, H, W] -> (a view of the same values in rows of `pitch` floats, the tensor it lies in)"""
    B, ch, H, W = a.shape
    t = torch.full((B, ch, H, pitch), PAD, device=dev())
    v = t[..., :W]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev()))
    return v, t


def _check(oracle, xn, fn, kn, what):
    import my_package._ext.my_lib as my_lib
    B, _, H, W = xn.shape
    want = oracle.filter_interpolation_forward(xn, fn, kn)
    for name, pitch in _pitches(W).items():
        (x, _), (f, _), (k, _) = _view(xn, pitch), _view(fn, pitch), _view(kn, pitch)
        out, whole = _view(np.full(xn.shape, np.nan, np.float32), pitch)
        assert my_lib.FilterInterpolationLayer_gpu_forward(x, f, k, out) == 0
        assert my_lib.last_kernel_path() == "fi_fwd:tiled_c3"
        P.close(out.contiguous().cpu().numpy(), want, "%s, %s (pitch %d)" % (what, name, pitch))
        if pitch > W:
            assert bool((whole[..., W:] == PAD).all()), "%s, %s: a store outside the view" % (what, name)


# every edge of the shifted grid (a tile ends at 32 + 64 k), widths below one tile, the headline width
WIDTHS = [4, 28, 32, 36, 60, 64, 68, 96, 256, 1024, 1280]


@pytest.mark.parametrize("W", WIDTHS)
def test_widths_around_the_shifted_grid(oracle, W):
    rng = np.random.default_rng(9100 + W)
    B, H = 2, 21
    xn, kn = synth.np_image(rng, B, 3, H, W), synth.np_filter(rng, B, H, W)
    fn = synth.np_flow(rng, B, H, W, "smooth", 3.0)
    _check(oracle, xn, fn, kn, "W %d" % W)


@pytest.mark.parametrize("W", [1277, 1278, 1279])
def test_ragged_widths(oracle, W):
    """widths that are not a multiple of four: the ragged-row instantiation and the tail kernel (unshifted), same results"""
    rng = np.random.default_rng(9200 + W)
    B, H = 1, 18
    xn, kn = synth.np_image(rng, B, 3, H, W), synth.np_filter(rng, B, H, W)
    fn = synth.np_flow(rng, B, H, W, "smooth", 3.0)
    _check(oracle, xn, fn, kn, "W %d" % W)


@pytest.mark.parametrize("H", [1, 7, 17, 31, 45])
def test_heights_off_the_tile(oracle, H):
    rng = np.random.default_rng(9300 + H)
    B, W = 2, 256
    xn, kn = synth.np_image(rng, B, 3, H, W), synth.np_filter(rng, B, H, W)
    fn = synth.np_flow(rng, B, H, W, "iid", 2.0)
    _check(oracle, xn, fn, kn, "H %d" % H)


@pytest.mark.parametrize("pan", [-24.0, -10.0, 10.0, 24.0])
def test_pans_past_the_left_edge_and_band_sweeps(oracle, pan):
    """a horizontal pan moves the first tile column's sources past the left edge (invalid sites copy the input pixel, boxes
    clamp at column 0) or the last column's past the right one; the i.i.d. flow on top makes boxes wider than the LDS
    budget, which the tiles sweep in bands -- some sites even reach the scalar path"""
    rng = np.random.default_rng(9400 + int(pan))
    B, H, W = 2, 40, 256
    xn, kn = synth.np_image(rng, B, 3, H, W), synth.np_filter(rng, B, H, W)
    for kind, sigma in (("iid", 14.0), ("smooth", 12.0)):
        fn = synth.np_flow(rng, B, H, W, kind, sigma)
        fn[:, 0] += np.float32(pan)
        fn[:, 1] -= np.float32(pan / 4)
        _check(oracle, xn, fn, kn, "pan %+g, %s flow" % (pan, kind))
