"""The still-image demo loop on the host route (networks/png_io.py): the scores from integer sums are rgb_scores' floats,
the RGB SSIM is the mean of three plane SSIMs, scenes_per_step batches consecutive scenes of one size without changing a
byte or a float, the new arguments are checked before a file is opened, and the defaults return what they returned.  CPU
only, with the stub model of tests/test_gpu_video_io.py (the mean of the two frames)."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "memc-net_amd")
A, B = (34, 130), (33, 47)


def _load(name):
    # networks/__init__ imports the HIP-backed operators; the loops are plain numpy / torch: load them by path
    if "networks_png_host" not in sys.modules:
        pkg = importlib.util.module_from_spec(importlib.util.spec_from_loader("networks_png_host", loader=None, is_package=True))
        pkg.__path__ = [os.path.join(PKG, "networks")]
        sys.modules["networks_png_host"] = pkg
    full = "networks_png_host." + name
    if full not in sys.modules:
        spec = importlib.util.spec_from_file_location(full, os.path.join(PKG, "networks", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
    return sys.modules[full]


@pytest.fixture(scope="module")
def png():
    return _load("png_io")


class Stub:
    """the mean of the two frames; records the batch sizes it was handed"""

    def __init__(self):
        self.batches = []

    def __call__(self, x):
        self.batches.append(x.shape[1])
        mid = (x[0] + x[1]) * 0.5
        return [mid, mid], None, None, None


def make_tree(png, root):
    """scenes s0 .. s6 of sizes A, A, B, A, A, A, A; a grey scene after s3 and a scene without its second file after s4;
    ground truth for all but s1, RGBA for s4, equal to the stub's result for s5"""
    rng = np.random.default_rng(23)
    data, gt = os.path.join(root, "data"), os.path.join(root, "gt")
    sizes = {"s0": A, "s1": A, "s2": B, "s3": A, "s4": A, "s5": A, "s6": A}
    for scene, (h, w) in sizes.items():
        os.makedirs(os.path.join(data, scene))
        os.makedirs(os.path.join(gt, scene))
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
        png.write_png(os.path.join(data, scene, "frame10.png"), a)
        png.write_png(os.path.join(data, scene, "frame11.png"), b)
        mean = (torch.from_numpy(a.astype(np.float32) / 255.0) + torch.from_numpy(b.astype(np.float32) / 255.0)) * 0.5
        rec = np.round(255.0 * mean.clamp(0.0, 1.0).numpy()).astype(np.uint8)
        truth = rec if scene == "s5" else np.clip(rec.astype(np.int16) + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
        if scene == "s4":
            truth = np.concatenate([truth, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=2)
        if scene != "s1":
            png.write_png(os.path.join(gt, scene, "frame10i11.png"), truth)
    os.makedirs(os.path.join(data, "s3a_grey"))
    for name in ("frame10.png", "frame11.png"):
        png.write_png(os.path.join(data, "s3a_grey", name), rng.integers(0, 256, A, dtype=np.uint8))
    os.makedirs(os.path.join(data, "s4a_missing"))
    png.write_png(os.path.join(data, "s4a_missing", "frame10.png"), rng.integers(0, 256, A + (3,), dtype=np.uint8))
    return data, gt


def files_of(root):
    out = {}
    for d, _dirs, names in os.walk(root):
        for n in names:
            with open(os.path.join(d, n), "rb") as f:
                out[os.path.relpath(os.path.join(d, n), root)] = f.read()
    return out


@pytest.mark.parametrize("shape", [(1, 1), (1, 5), (3, 5), (7, 9), (34, 130), (33, 47)])
def test_scores_from_sums_are_rgb_scores_floats(png, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    h, w = shape
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    pairs = [(a, rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
             (a, np.clip(a.astype(np.int16) + rng.integers(-2, 3, a.shape), 0, 255).astype(np.uint8)),
             (a, a.copy()),
             (np.zeros_like(a), np.full_like(a, 255)),
             (np.full_like(a, 255), np.zeros_like(a))]
    for rec, gt in pairs:
        d = rec.astype(np.int64) - gt.astype(np.int64)
        err, psnr, _diff = png.rgb_scores(rec, gt)
        got = png.rgb_scores_from_sums(np.uint64(np.abs(d).sum()), np.uint64((d * d).sum()), 3 * h * w)
        assert got == (err, psnr) and all(type(v) is float for v in got)
        assert png.rgb_scores_from_sums(int(np.abs(d).sum()), int((d * d).sum()), 3 * h * w) == (err, psnr)
    assert png.rgb_scores_from_sums(0, 0, 3 * h * w) == (0.0, 100.0)
    assert png.rgb_scores_from_sums(3 * h * w * 255, 3 * h * w * 65025, 3 * h * w) == (255.0, 0.0)


def test_rgb_ssim_is_the_mean_of_three_plane_ssims(png):
    Y = _load("yuv_io")
    rng = np.random.default_rng(5)
    for h, w in ((7, 7), (7, 9), (33, 47)):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
        want = float(np.mean([Y.ssim_from_planes(a[:, :, c], b[:, :, c]) for c in range(3)]))
        assert png.rgb_ssim(a, b) == want and 0.0 < want < 1.0
        assert png.rgb_ssim(a, a.copy()) == 1.0
    with pytest.raises(ValueError):
        png.rgb_ssim(np.zeros((6, 9, 3), dtype=np.uint8), np.zeros((6, 9, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        png.rgb_ssim(np.zeros((9, 9), dtype=np.uint8), np.zeros((9, 9), dtype=np.uint8))


def test_batches_of_equally_sized_scenes_change_nothing(png, tmp_path):
    data, gt = make_tree(png, str(tmp_path))
    runs = {}
    for n in (1, 3, 8):
        model, out = Stub(), str(tmp_path / ("out%d" % n))
        res = png.interpolate_png_tree(model, data, out, torch.device("cpu"), gt_dir=gt, scenes_per_step=n, ssim=True)
        runs[n] = (model.batches, res, files_of(out))
    assert runs[1][0] == [1] * 7
    assert runs[3][0] == [2, 1, 3, 1]              # skipped scenes neither enter nor end a batch
    assert runs[8][0] == [2, 1, 4]
    batches, res, files = runs[1]
    assert [r[0] for r in res] == ["s0", "s1", "s2", "s3", "s4", "s5", "s6"]
    assert res[1][1:] == (None, None, None) and all(len(r) == 4 and r[1] is not None for r in res if r[0] != "s1")
    assert res[5][1:] == (0.0, 100.0, 1.0)                         # the ground truth is the result
    assert len(files) == 7 + 6 and not any("grey" in k or "missing" in k for k in files)
    for n in (3, 8):
        assert runs[n][1] == res
        assert runs[n][2] == files
    # and the result is the restated one: the rounded mean of the two frames
    a, b = (png.read_png(os.path.join(data, "s2", f)) for f in ("frame10.png", "frame11.png"))
    mean = (torch.from_numpy(a.astype(np.float32) / 255.0) + torch.from_numpy(b.astype(np.float32) / 255.0)) * 0.5
    assert np.array_equal(png.read_png(os.path.join(str(tmp_path / "out3"), "s2", "frame10i11.png")),
                          np.round(255.0 * mean.numpy()).astype(np.uint8))


def test_the_new_arguments_are_checked_before_a_file_is_opened(png, tmp_path, monkeypatch):
    def no_file(*a, **k):
        raise AssertionError("a file was opened")
    monkeypatch.setattr(png, "read_png", no_file)
    monkeypatch.setattr(png.os, "listdir", no_file)
    nowhere = str(tmp_path / "nowhere")
    for n in (0, -2):
        with pytest.raises(ValueError):
            png.interpolate_png_tree(Stub(), nowhere, nowhere, torch.device("cpu"), scenes_per_step=n)
    with pytest.raises(ValueError):
        png.interpolate_png_tree(Stub(), nowhere, nowhere, torch.device("cpu"), gpu_io=True)
    with pytest.raises(ValueError):
        png.interpolate_png_tree(Stub(), nowhere, nowhere, "cpu", gpu_io=True, scenes_per_step=4, ssim=True)
    assert not os.path.exists(nowhere)


def test_the_default_call_returns_three_tuples_as_before(png, tmp_path):
    data, gt = make_tree(png, str(tmp_path))
    model, out = Stub(), str(tmp_path / "out")
    res = png.interpolate_png_tree(model, data, out, torch.device("cpu"), gt_dir=gt)
    assert model.batches == [1] * 7 and all(len(r) == 3 for r in res)
    assert res[1] == ("s1", None, None)
    for scene, err, psnr in res:
        if err is None:
            continue
        rec = png.read_png(os.path.join(out, scene, "frame10i11.png"))
        truth = png.read_png(os.path.join(gt, scene, "frame10i11.png"))[:, :, :3]
        want_err, want_psnr, want_diff = png.rgb_scores(rec, truth)
        assert (err, psnr) == (want_err, want_psnr)
        assert np.array_equal(png.read_png(os.path.join(out, scene, "frame10i11_diff%.4f.png" % err)), want_diff)
    with pytest.raises(ValueError):                # a 7 x 7 window does not fit
        small = str(tmp_path / "small")
        os.makedirs(os.path.join(small, "t"))
        for name in ("frame10.png", "frame11.png"):
            png.write_png(os.path.join(small, "t", name), np.zeros((6, 9, 3), dtype=np.uint8))
        png.interpolate_png_tree(Stub(), small, str(tmp_path / "out_small"), torch.device("cpu"), ssim=True)
