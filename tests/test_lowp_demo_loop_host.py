"""The demo loops' precision arguments on the host route (networks/inference.py, networks/yuv_io.py): dtype=float16 / bfloat16
hands the model planes (float32(byte) / 255).to(dtype), padded in that dtype, and widens the result before it is rounded;
autocast= runs the model inside torch.autocast on float32 planes; the defaults change nothing.  CPU only, with stub models
that compute in the dtype they are given; every expectation is restated here in numpy / torch."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "memc-net_amd")
HALVES = [torch.float16, torch.bfloat16]
H, W, FRAMES = 34, 130, 5


def _load(name):
    # networks/__init__ imports the HIP-backed operators; the loops are plain numpy / torch: load them by path
    if "networks_lowp_host" not in sys.modules:
        pkg = importlib.util.module_from_spec(importlib.util.spec_from_loader("networks_lowp_host", loader=None, is_package=True))
        pkg.__path__ = [os.path.join(PKG, "networks")]
        sys.modules["networks_lowp_host"] = pkg
    full = "networks_lowp_host." + name
    if full not in sys.modules:
        spec = importlib.util.spec_from_file_location(full, os.path.join(PKG, "networks", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[full] = mod
        spec.loader.exec_module(mod)
    return sys.modules[full]


@pytest.fixture(scope="module")
def Y():
    return _load("yuv_io")


@pytest.fixture(scope="module")
def inf():
    return _load("inference")


class Stub:
    """which = 0: the first frame; which = 1: the mean of the two, in the dtype of x.  Records what it was handed."""

    def __init__(self, returns=None):
        self.seen, self.returns = [], returns

    def __call__(self, x):
        self.seen.append((x.dtype, tuple(x.shape), torch.is_autocast_enabled("cpu"),
                          torch.get_autocast_dtype("cpu") if torch.is_autocast_enabled("cpu") else None))
        first, mean = x[0], 0.5 * x[0] + 0.5 * x[1]
        if self.returns is not None:
            first, mean = first.to(self.returns), mean.to(self.returns)
        return [first, mean], None, None, None


@pytest.fixture(scope="module")
def clip(Y, tmp_path_factory):
    """five frames of random RGB through Yuv420Writer -> (path, what the reader gives back: uint8 [5, H, W, 3])"""
    path = str(tmp_path_factory.mktemp("lowp_host") / "in.yuv")
    rng = np.random.default_rng(19)
    wr = Y.Yuv420Writer(path, from_rgb=True)
    for _ in range(FRAMES):
        wr.write(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    wr.close()
    rd = Y.Yuv420Reader(path, H, W, to_rgb=True)
    rgb = np.stack([rd.read(k)[0] for k in range(FRAMES)])
    rd.close()
    return path, rgb


def planes_of(rgb, dtype):
    """uint8 [..., h, w, 3] -> (float32(byte) / 255).to(dtype), [..., 3, h, w]"""
    x = torch.from_numpy(np.ascontiguousarray(np.moveaxis(rgb, -1, -3)).astype(np.float32) / np.float32(255.0))
    return x if dtype is None else x.to(dtype)


def bytes_of(planes):
    """[3, h, w] of any float dtype -> uint8 [h, w, 3]: the loop's rounding, on the widened value"""
    x = planes.float().clamp(0.0, 1.0).numpy()
    return np.transpose(np.round(np.float32(255.0) * x).astype(np.uint8), (1, 2, 0))


def expected(Y, rgb, dtype, which, path, ssim=False):
    """the file and the scores, restated: frame i, then the stub's result for (i, i + 2), scored against frame i + 1"""
    wr = Y.Yuv420Writer(path, from_rgb=True)
    scores = []
    for i in range(0, FRAMES - 2, 2):
        a, b = planes_of(rgb[i], dtype), planes_of(rgb[i + 2], dtype)
        rec = bytes_of(a if which == 0 else 0.5 * a + 0.5 * b)
        wr.write(rgb[i])
        wr.write(rec)
        scores.append((i + 1,) + Y.luma_scores(rec, rgb[i + 1]) + ((Y.luma_ssim(rec, rgb[i + 1]),) if ssim else ()))
    wr.close()
    return np.fromfile(path, dtype=np.uint8), scores


def run(Y, model, src, dst, **kw):
    scores = Y.interpolate_yuv_sequence(model, src, dst, H, W, torch.device("cpu"), first=0, last=FRAMES - 2, **kw)
    return np.fromfile(dst, dtype=np.uint8), scores


@pytest.mark.parametrize("dtype", HALVES)
def test_quantise_of_decode_is_the_identity_on_bytes(dtype):
    """T(float32(b) / 255) widened, times 255, rounded to nearest even, is b for all 256 bytes"""
    b = torch.arange(256, dtype=torch.uint8)
    x = (b.float() / 255).to(dtype)
    assert x.dtype == dtype
    back = np.round(np.float32(255.0) * x.float().clamp(0.0, 1.0).numpy()).astype(np.uint8)
    assert np.array_equal(back, b.numpy())


@pytest.mark.parametrize("pairs_per_step", [1, 2])
@pytest.mark.parametrize("dtype", HALVES)
def test_a_cast_run_gives_the_restated_file_and_scores(Y, clip, tmp_path, dtype, pairs_per_step):
    src, rgb = clip
    model = Stub()
    got, scores = run(Y, model, src, str(tmp_path / "out.yuv"), dtype=dtype, pairs_per_step=pairs_per_step, ssim=True)
    want, want_scores = expected(Y, rgb, dtype, 1, str(tmp_path / "want.yuv"), ssim=True)
    assert got.size == 4 * Y.frame_bytes(H, W) and np.array_equal(got, want)
    assert scores == want_scores and [s[0] for s in scores] == [1, 3]
    # the model saw planes of that dtype, padded to the demo's extent, outside autocast
    assert [s[0] for s in model.seen] == [dtype] * len(model.seen) and not any(s[2] for s in model.seen)
    assert [s[1] for s in model.seen] == [(2, n, 3, 128, 256) for n in ([1, 1] if pairs_per_step == 1 else [2])]
    # and the half result is not the float32 one: the dtype reached the arithmetic
    assert not np.array_equal(got, expected(Y, rgb, None, 1, str(tmp_path / "f32.yuv"))[0])


@pytest.mark.parametrize("dtype", HALVES)
def test_the_first_frame_comes_back_as_its_own_bytes(Y, clip, tmp_path, dtype):
    """which = 0: the stub returns frame i; its quantised bytes are frame i's decoded bytes, so the file holds every even
    frame twice and the scores are those of frame i against frame i + 1"""
    src, rgb = clip
    got, scores = run(Y, Stub(), src, str(tmp_path / "out.yuv"), dtype=dtype, which=0)
    frames = got.reshape(4, -1)
    assert np.array_equal(frames[0], frames[1]) and np.array_equal(frames[2], frames[3])
    want, want_scores = expected(Y, rgb, dtype, 0, str(tmp_path / "want.yuv"))
    assert np.array_equal(got, want) and scores == want_scores
    assert scores == [(i + 1,) + Y.luma_scores(rgb[i], rgb[i + 1]) for i in (0, 2)]


def test_float32_and_none_are_today_s_call(Y, clip, tmp_path):
    src, rgb = clip
    outs = {}
    for name, kw in (("plain", dict()), ("none", dict(dtype=None, autocast=None)), ("f32", dict(dtype=torch.float32))):
        model = Stub()
        outs[name] = run(Y, model, src, str(tmp_path / (name + ".yuv")), **kw)
        assert [s[0] for s in model.seen] == [torch.float32] * 2 and not any(s[2] for s in model.seen)
    want = expected(Y, rgb, None, 1, str(tmp_path / "want.yuv"))
    for name in outs:
        assert np.array_equal(outs[name][0], want[0]) and outs[name][1] == want[1], name


@pytest.mark.parametrize("dtype", HALVES)
def test_autocast_hands_over_float32_planes_inside_autocast(Y, clip, tmp_path, dtype):
    src, rgb = clip
    model = Stub()
    got, scores = run(Y, model, src, str(tmp_path / "out.yuv"), autocast=dtype)
    assert model.seen == [(torch.float32, (2, 1, 3, 128, 256), True, dtype)] * 2
    assert not torch.is_autocast_enabled("cpu")                    # and the state does not outlive the call
    # the stub's own arithmetic is elementwise: autocast leaves it in float32
    want, want_scores = expected(Y, rgb, None, 1, str(tmp_path / "want.yuv"))
    assert np.array_equal(got, want) and scores == want_scores
    # a model that answers in half inside autocast (as a network's last layer may): widened before the rounding
    got, scores = run(Y, Stub(returns=dtype), src, str(tmp_path / "half.yuv"), autocast=dtype)
    wr = Y.Yuv420Writer(str(tmp_path / "want_half.yuv"), from_rgb=True)
    for i in (0, 2):
        wr.write(rgb[i])
        wr.write(bytes_of((0.5 * planes_of(rgb[i], None) + 0.5 * planes_of(rgb[i + 2], None)).to(dtype)))
    wr.close()
    assert np.array_equal(got, np.fromfile(str(tmp_path / "want_half.yuv"), dtype=np.uint8))


BAD = [(dict(dtype=torch.float16, autocast=torch.float16), ValueError),
       (dict(dtype=torch.bfloat16, autocast=torch.float16), ValueError),
       (dict(dtype=torch.float64), TypeError),
       (dict(dtype=torch.uint8), TypeError),
       (dict(dtype="bf16"), TypeError),
       (dict(autocast=torch.float32), TypeError),
       (dict(autocast=torch.float64), TypeError),
       (dict(autocast=True), TypeError),
       (dict(dtype=torch.float16, autocast=torch.float32), TypeError)]


@pytest.mark.parametrize("gpu_io", [False, True])
@pytest.mark.parametrize("kw,error", BAD)
def test_bad_precision_arguments_are_refused_before_a_file_is_opened(Y, clip, tmp_path, kw, error, gpu_io):
    src, _rgb = clip
    dst = str(tmp_path / "out.yuv")
    model = Stub()
    with pytest.raises(error):
        Y.interpolate_yuv_sequence(model, src, dst, H, W, torch.device("cpu"), first=0, last=FRAMES - 2, gpu_io=gpu_io, **kw)
    assert not os.path.exists(dst) and not model.seen
    with pytest.raises(error):                                     # nor is the input looked for
        Y.interpolate_yuv_sequence(model, str(tmp_path / "absent.yuv"), dst, H, W, torch.device("cpu"), gpu_io=gpu_io, **kw)
    assert not os.path.exists(dst)


def test_float32_autocast_is_not_an_error(Y, clip, tmp_path):
    src, _rgb = clip
    run(Y, Stub(), src, str(tmp_path / "out.yuv"), dtype=torch.float32, autocast=torch.bfloat16)


class Probe(torch.nn.Module):
    """returns its padded first frame (and that plus one), as it came; records dtype and autocast state"""

    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x):
        self.seen.append((x.dtype, tuple(x.shape), torch.is_autocast_enabled("cpu")))
        return [x[0], x[0] + 1.0], None, None, None


def test_interpolate_pairs(inf):
    f0, f2 = torch.rand(2, 3, 101, 203), torch.rand(2, 3, 101, 203)
    pads = inf.pad_amounts(101, 203)
    for dtype in HALVES:
        probe = Probe()
        out = inf.interpolate_pairs(probe, f0, f2, which=0, dtype=dtype)
        assert out.dtype == dtype and torch.equal(out, f0.to(dtype))       # what the model returns, cropped: not widened
        assert probe.seen == [(dtype, (2, 2, 3, 128, 256), False)]
        # padded in that dtype: replicate padding copies, so casting first or last is the same tensor
        seen = []
        inf.interpolate_pairs(lambda x: (seen.append(x), ([x[0], x[1]], None, None, None))[1], f0, f2, which=1, dtype=dtype)
        assert torch.equal(seen[0], torch.stack([F.pad(f.to(dtype), pads, mode="replicate") for f in (f0, f2)]))
        probe = Probe()
        out = inf.interpolate_pairs(probe, f0, f2, which=0, autocast=dtype)
        assert out.dtype == torch.float32 and torch.equal(out, f0)
        assert probe.seen == [(torch.float32, (2, 2, 3, 128, 256), True)]
    for kw in (dict(), dict(dtype=None, autocast=None), dict(dtype=torch.float32)):
        probe = Probe()
        out = inf.interpolate_pairs(probe, f0, f2, which=0, **kw)
        assert out.dtype == torch.float32 and torch.equal(out, f0)
        assert probe.seen == [(torch.float32, (2, 2, 3, 128, 256), False)]
    for kw, error in BAD:
        probe = Probe()
        with pytest.raises(error):
            inf.interpolate_pairs(probe, f0, f2, **kw)
        assert not probe.seen
