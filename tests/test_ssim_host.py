"""The host rule of the HD demo's third score (networks/yuv_io.py: ssim_from_planes, luma_ssim, interpolate_yuv_sequence's
`ssim` keyword), on the CPU: against the scipy formulation of skimage's compare_ssim written out here (where scipy exists),
against the values that formulation gave when tests/golden/ssim_cases.json was recorded (everywhere), the exact 1.0 of
equal planes, the size check, and the loop's tuples with and without the keyword.

Worst |ssim_from_planes - scipy formulation| seen over the 24 cases when the fixture was recorded: 7.77e-16 (the 7 x 7
near-equal case; 4.09e-16 at 720 x 1280, the checkerboard); profiles/r17_ssim.txt."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "memc-net_amd")
SIZES = [(7, 7), (8, 10), (22, 70), (23, 71), (40, 136), (720, 1280)]
KINDS = ["iid", "near", "equal", "checker"]
# The float formulation cancels uxx - ux^2 at magnitudes up to 65025 in front of a denominator >= 58.5: about
# 4 * 2^-53 * 65025 / 58.5 = 5e-13 per position; the integer form has no cancellation.
BOUND = 1e-12


def _load(name):
    # networks/__init__ imports the HIP-backed operators; the IO helpers are plain numpy / torch: load them by path
    if "networks_ssim_host" not in sys.modules:
        pkg = importlib.util.module_from_spec(importlib.util.spec_from_loader("networks_ssim_host", loader=None, is_package=True))
        pkg.__path__ = [os.path.join(PKG, "networks")]
        sys.modules["networks_ssim_host"] = pkg
    full = "networks_ssim_host." + name
    if full not in sys.modules:
        spec = importlib.util.spec_from_file_location(full, os.path.join(PKG, "networks", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
    return sys.modules[full]


def planes(kind, seed, h, w):
    """tests/golden/make_ssim_cases.py's planes: iid bytes; the second within +-3 of the first; equal; a 0 / 255 checkerboard
    of period 7 against itself moved by (2, 3)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "iid":
        return a, rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "near":
        return a, np.clip(a.astype(np.int16) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)
    if kind == "equal":
        return a, a.copy()
    yy, xx = np.mgrid[0:h, 0:w]
    board = lambda y, x: ((((y // 7) + (x // 7)) & 1) * 255).astype(np.uint8)
    return board(yy, xx), board(yy + 2, xx + 3)


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


@pytest.fixture(scope="module")
def fixture_cases():
    with open(os.path.join(HERE, "golden", "ssim_cases.json")) as f:
        cases = json.load(f)["cases"]
    assert sorted((c["h"], c["w"], c["kind"]) for c in cases) == sorted((h, w, k) for h, w in SIZES for k in KINDS)
    return cases


@pytest.fixture(scope="module")
def computed(fixture_cases):
    """ssim_from_planes of every case, once: {(h, w, kind): (value, the planes)}"""
    Y = _load("yuv_io")
    out = {}
    for c in fixture_cases:
        a, b = planes(c["kind"], c["seed"], c["h"], c["w"])
        out[(c["h"], c["w"], c["kind"])] = (Y.ssim_from_planes(a, b), a, b)
    return out


def test_against_the_scipy_formulation(fixture_cases, computed):
    pytest.importorskip("scipy")
    worst = 0.0
    for c in fixture_cases:
        got, a, b = computed[(c["h"], c["w"], c["kind"])]
        want = scipy_ssim(a, b)
        assert want == float.fromhex(c["ssim_hex"]) or abs(want - c["ssim"]) <= BOUND      # the fixture is this formulation's
        err = abs(got - want)
        worst = max(worst, err)
        print("%4d x %4d %-7s  ssim %.17g  |integer form - scipy formulation| %.3g" % (c["h"], c["w"], c["kind"], got, err))
        assert err <= BOUND, c
    print("worst: %.3g" % worst)


def test_against_the_recorded_values(fixture_cases, computed):
    for c in fixture_cases:
        got = computed[(c["h"], c["w"], c["kind"])][0]
        assert c["ssim"] == float.fromhex(c["ssim_hex"])
        assert abs(got - c["ssim"]) <= BOUND, (c, got)
        assert -1.0 <= got <= 1.0


def test_equal_planes_give_exactly_one(computed):
    Y = _load("yuv_io")
    for (h, w, kind), (got, a, b) in computed.items():
        if kind == "equal":
            assert np.array_equal(a, b) and got == 1.0, (h, w, got)
        else:
            assert got < 1.0, (h, w, kind, got)
    for value in (0, 255, 128):
        flat = np.full((9, 11), value, dtype=np.uint8)
        assert Y.ssim_from_planes(flat, flat) == 1.0


def test_the_rule_is_symmetric_and_sees_every_window(computed):
    """S is symmetric in its planes bit for bit; a single changed corner pixel enters exactly one of the N windows"""
    Y = _load("yuv_io")
    got, a, b = computed[(23, 71, "iid")]
    assert Y.ssim_from_planes(b, a) == got
    for corner in ((0, 0), (0, 70), (22, 0), (22, 70)):
        c = a.copy()
        c[corner] ^= 0x80
        v = Y.ssim_from_planes(a, c)
        n = (23 - 6) * (71 - 6)
        assert v < 1.0 and (1.0 - v) * n <= 2.0, (corner, v)            # one window's S moved, by at most 2


def test_sizes_below_the_window_raise():
    Y = _load("yuv_io")
    for h, w in ((6, 7), (7, 6), (6, 100), (100, 6), (1, 1)):
        z = np.zeros((h, w), dtype=np.uint8)
        with pytest.raises(ValueError):
            Y.ssim_from_planes(z, z)
    with pytest.raises(ValueError):
        Y.luma_ssim(np.zeros((6, 8, 3), dtype=np.uint8), np.zeros((6, 8, 3), dtype=np.uint8))
    with pytest.raises(ValueError):                                        # planes of two shapes; not bytes
        Y.ssim_from_planes(np.zeros((8, 8), dtype=np.uint8), np.zeros((8, 9), dtype=np.uint8))
    with pytest.raises(ValueError):
        Y.ssim_from_planes(np.zeros((8, 8)), np.zeros((8, 8)))


def test_luma_ssim_takes_luma_scores_planes():
    Y = _load("yuv_io")
    rng = np.random.default_rng(5)
    rec, gt = rng.integers(0, 256, (12, 20, 3), dtype=np.uint8), rng.integers(0, 256, (12, 20, 3), dtype=np.uint8)
    ry = (Y.rgb_to_yuv(rec / 255.0)[:, :, 0] * 255.0).astype(np.uint8)
    gy = (Y.rgb_to_yuv(gt / 255.0)[:, :, 0] * 255.0).astype(np.uint8)
    assert Y.luma_ssim(rec, gt) == Y.ssim_from_planes(ry, gy)
    assert Y.luma_ssim(rec, rec) == 1.0


def test_the_loop_with_and_without_the_keyword(tmp_path, monkeypatch):
    """The stub model and clip of tests/test_yuv_io.py on the host path: ssim=False returns exactly the tuples of a call
    without the keyword and writes the same file; ssim=True the same three elements and file plus luma_ssim of the very
    frames luma_scores was given."""
    Y = _load("yuv_io")
    h, w, n = 16, 32, 7
    rng = np.random.default_rng(2)
    base = rng.integers(40, 200, (h, w, 3)).astype(np.float64)
    src = str(tmp_path / "in.yuv")
    wr = Y.Yuv420Writer(src)
    for k in range(n):
        wr.write(np.clip(base + 6.0 * k, 0, 255).astype(np.uint8))
    wr.close()

    class Mean(torch.nn.Module):
        def forward(self, x):
            m = 0.5 * (x[0] + x[1])
            return [m, m], None, None, None

    scored = []
    luma_scores = Y.luma_scores
    monkeypatch.setattr(Y, "luma_scores", lambda rec, gt: (scored.append((rec.copy(), gt.copy())), luma_scores(rec, gt))[1])
    runs, files = {}, {}
    for name, kw in (("plain", dict()), ("off", dict(ssim=False)), ("on", dict(ssim=True)), ("on2", dict(ssim=True, pairs_per_step=2))):
        del scored[:]
        dst = str(tmp_path / (name + ".yuv"))
        runs[name] = Y.interpolate_yuv_sequence(Mean(), src, dst, h, w, torch.device("cpu"), first=0, last=n - 2, **kw)
        files[name] = np.fromfile(dst, dtype=np.uint8)
        frames = list(scored)
    assert runs["off"] == runs["plain"] and all(len(t) == 3 for t in runs["plain"]) and len(runs["plain"]) == 3
    assert runs["on2"] == runs["on"]
    assert [t[:3] for t in runs["on"]] == runs["plain"] and all(len(t) == 4 for t in runs["on"])
    for name in ("off", "on", "on2"):
        assert np.array_equal(files[name], files["plain"]), name
    assert len(frames) == 3
    for t, (rec, gt) in zip(runs["on2"], frames):
        assert t[3] == Y.luma_ssim(rec, gt) and 0.5 < t[3] < 1.0, t
