#!/usr/bin/env python
"""Records tests/golden/ssim_cases.json: the SSIM of seeded plane pairs under the SCIPY FORMULATION of skimage's
compare_ssim at its defaults (five scipy.ndimage.uniform_filter passes in float64), so that tests/test_ssim_host.py can
hold networks/yuv_io.py::ssim_from_planes to it on a machine without scipy.

    python tests/golden/make_ssim_cases.py          # needs numpy and scipy; rewrites the fixture beside it

The planes of a case come from `planes(kind, seed, h, w)`, which tests/test_ssim_host.py repeats: the fixture holds the
seeds, shapes, kinds and values only."""
import json
import os

import numpy as np

SIZES = [(7, 7), (8, 10), (22, 70), (23, 71), (40, 136), (720, 1280)]
KINDS = ["iid", "near", "equal", "checker"]


def planes(kind, seed, h, w):
    """two uint8 planes: iid bytes; the second within +-3 of the first; equal; a 0 / 255 checkerboard of period 7 against
    itself moved by (2, 3), where whole windows are 255 in both planes"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "iid":
        return a, rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "near":
        return a, np.clip(a.astype(np.int16) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)
    if kind == "equal":
        return a, a.copy()
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        board = lambda y, x: ((((y // 7) + (x // 7)) & 1) * 255).astype(np.uint8)
        return board(yy, xx), board(yy + 2, xx + 3)
    raise ValueError(kind)


def scipy_ssim(x, y):
    """skimage's compare_ssim(x, y) for two uint8 planes at its defaults, written out: 7 x 7 uniform filter, sample
    covariance, K1 = 0.01, K2 = 0.03, data range 255, the mean over the map cropped by 3"""
    from scipy.ndimage import uniform_filter
    x, y = x.astype(np.float64), y.astype(np.float64)
    win, n = 7, 49
    cov_norm = n / (n - 1.0)
    ux, uy = uniform_filter(x, size=win), uniform_filter(y, size=win)
    uxx, uyy, uxy = uniform_filter(x * x, size=win), uniform_filter(y * y, size=win), uniform_filter(x * y, size=win)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    pad = (win - 1) // 2
    return float(s[pad:s.shape[0] - pad, pad:s.shape[1] - pad].mean(dtype=np.float64))


def main():
    cases = []
    for i, (h, w) in enumerate(SIZES):
        for j, kind in enumerate(KINDS):
            seed = 1700 + 10 * i + j
            a, b = planes(kind, seed, h, w)
            v = scipy_ssim(a, b)
            cases.append({"h": h, "w": w, "kind": kind, "seed": seed, "ssim": v, "ssim_hex": v.hex()})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ssim_cases.json")
    with open(path, "w") as f:
        json.dump({"formulation": "scipy.ndimage.uniform_filter, float64 (skimage compare_ssim defaults)", "cases": cases}, f,
                  indent=1)
        f.write("\n")
    print("wrote %d cases to %s" % (len(cases), path))


if __name__ == "__main__":
    main()
