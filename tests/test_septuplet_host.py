"""The video-enhancement demo loop (networks/septuplet_io.py::enhance_septuplet_tree) on the host, with a stub model: a
synthetic septuplet tree in tmp_path (tests/_septuplets.py: two clips of 24 x 40 and one of 128 x 128, whose sides take the
32 + 32 branch of the padding rule).  File layout, padding and crop, the written PNG bytes, the scores against png_io's on
the same arrays, the metrics.txt text, the clip list, and gpu_io=True on a CPU device.  No GPU, no network."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _septuplets as SP      # noqa: E402


@pytest.fixture(scope="module")
def io():
    """networks/septuplet_io.py and png_io.py as modules of their own package (no operator is imported)"""
    import importlib.util
    import types
    pkg_dir = os.path.join(os.path.dirname(HERE), "memc-net_amd", "networks")
    pkg = types.ModuleType("_ve_io_pkg")
    pkg.__path__ = [pkg_dir]
    sys.modules["_ve_io_pkg"] = pkg
    mods = {}
    for name in ("png_io", "inference", "yuv_io", "septuplet_io"):
        spec = importlib.util.spec_from_file_location("_ve_io_pkg." + name, os.path.join(pkg_dir, name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mods[name]
        spec.loader.exec_module(mods[name])
    yield types.SimpleNamespace(**mods)
    for k in [k for k in sys.modules if k.startswith("_ve_io_pkg")]:
        del sys.modules[k]


@pytest.fixture(scope="module")
def tree(io, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("vimeo"))
    return root, SP.write_tree(root, io.png_io.write_png)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _s, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("ssim", [False, True])
def test_loop_on_the_synthetic_tree(io, tree, tmp_path, ssim):
    root, made = tree
    out = str(tmp_path / "out")
    model = SP.StubEnhancer()
    results = io.septuplet_io.enhance_septuplet_tree(model, os.path.join(root, "input"), os.path.join(root, "target"), out,
                                                     "cpu", ssim=ssim)
    clips = [c for c, _h, _w in SP.CLIPS]
    # every clip of the tree, sorted; each padded by the reference's rule (128 x 128 -> 192 x 192: 32 + 32 on both sides)
    assert [r[0] for r in results] == clips
    assert model.shapes == [SP.padded_shape(h, w) for _c, h, w in SP.CLIPS] == [(1, 3, 128, 128)] * 2 + [(1, 3, 192, 192)]
    assert _files(out) == sorted([c + "/im4.png" for c in clips] + ["metrics.txt"])
    want_scores = []
    for r in results:
        frames, target = made[r[0]]
        want = SP.expected_centre(frames)
        assert want.min() == 0 and want.max() == 255                   # the clip to [0, 1] is exercised
        assert np.array_equal(io.png_io.read_png(os.path.join(out, r[0], "im4.png")), want)
        ref_file = str(tmp_path / "expected.png")
        io.png_io.write_png(ref_file, want)
        assert open(os.path.join(out, r[0], "im4.png"), "rb").read() == open(ref_file, "rb").read()
        err, psnr, _diff = io.png_io.rgb_scores(want, target)
        score = (err, psnr) + ((io.png_io.rgb_ssim(want, target),) if ssim else ())
        assert r[1:] == score
        want_scores.append(score)
    mean = lambda k: str(round(sum(s[k] for s in want_scores) / len(want_scores), 4))      # noqa: E731
    text = "The average interpolation error / PSNR for all images are : " + mean(0) + ",\t  psnr " + mean(1)
    if ssim:
        text += ",\t  ssim " + mean(2)
    assert open(os.path.join(out, "metrics.txt")).read() == text + "\n"


def test_clip_list_selects_and_orders(io, tree, tmp_path):
    root, made = tree
    listing = str(tmp_path / "sep_testlist.txt")
    with open(listing, "w") as f:
        f.write("00002/0001\n\n00001/0001\n")
    out = str(tmp_path / "out")
    results = io.septuplet_io.enhance_septuplet_tree(SP.StubEnhancer(), os.path.join(root, "input"),
                                                     os.path.join(root, "target"), out, "cpu", list_file=listing)
    assert [r[0] for r in results] == ["00002/0001", "00001/0001"]
    assert _files(out) == ["00001/0001/im4.png", "00002/0001/im4.png", "metrics.txt"]
    assert io.septuplet_io.list_clips(os.path.join(root, "input")) == [c for c, _h, _w in SP.CLIPS]


def test_a_model_that_returns_a_tuple_gives_its_first_element(io, tree, tmp_path):
    root, made = tree
    stub = SP.StubEnhancer()

    class Debug(torch.nn.Module):                                      # MEMC_Net_VE under debug=True
        def forward(self, xs):
            return stub(xs), None, None
    listing = str(tmp_path / "one.txt")
    open(listing, "w").write("00001/0002\n")
    out = str(tmp_path / "out")
    io.septuplet_io.enhance_septuplet_tree(Debug(), os.path.join(root, "input"), os.path.join(root, "target"), out, "cpu",
                                           list_file=listing)
    assert np.array_equal(io.png_io.read_png(os.path.join(out, "00001/0002/im4.png")), SP.expected_centre(made["00001/0002"][0]))


def test_gpu_io_on_a_cpu_device_raises_before_a_file_is_read(io, tmp_path):
    missing = str(tmp_path / "nowhere")
    with pytest.raises(ValueError, match="gpu_io"):
        io.septuplet_io.enhance_septuplet_tree(SP.StubEnhancer(), missing, missing, str(tmp_path / "out"), "cpu", gpu_io=True)
    assert not os.path.exists(str(tmp_path / "out"))


def test_a_target_of_another_size_is_an_error(io, tree, tmp_path):
    root, made = tree
    other = str(tmp_path / "target")
    os.makedirs(os.path.join(other, "00001/0001"))
    io.png_io.write_png(os.path.join(other, "00001/0001/im4.png"), made["00002/0001"][1])
    listing = str(tmp_path / "one.txt")
    open(listing, "w").write("00001/0001\n")
    with pytest.raises(ValueError, match="00001/0001"):
        io.septuplet_io.enhance_septuplet_tree(SP.StubEnhancer(), os.path.join(root, "input"), other, str(tmp_path / "out"),
                                               "cpu", list_file=listing)
