"""The kernels of libmemc_hip_still.so (include/memc_still.h) and the still-image demo loop's gpu_io route against the host
route of networks/png_io.py: decode into padded slices of the network's input in the three storages, the quantiser on every
16-bit pattern and on float32's ties, the integer sums and the difference picture, the loop's files and tuples both ways,
and the command line.  Everything is compared exactly (torch.equal, ==) but the SSIM, whose device sum runs in another order
than numpy's (tests/test_gpu_ssim.py's bound)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
SENTINEL = {torch.float32: -7.0, torch.float16: -7.0, torch.bfloat16: -7.0}
A, B = (34, 130), (33, 47)


@pytest.fixture(scope="module")
def S():
    import my_package._ext.my_lib_still as M
    M.lib()
    return M


@pytest.fixture(scope="module")
def png():
    import networks.png_io as M
    return M


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def picture(seed, frames, h, w):
    """uint8 [frames, h, w, 3] of random bytes; where it has room, the first frame starts with all 256 values"""
    rgb = np.random.default_rng(seed).integers(0, 256, (frames, h, w, 3), dtype=np.uint8)
    if h * w * 3 >= 256:
        rgb[0].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    return rgb


# ---- decode -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("pads", [(0, 0, 0, 0), (1, 2, 3, 0), (5, 6, 2, 7)])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (7, 9), (34, 130)])
def test_decode_writes_the_padded_extent_and_nothing_else(S, dev, shape, pads, frames, dtype):
    h, w = shape
    left, right, top, bottom = pads
    hp, wp = h + top + bottom, w + left + right
    rgb = picture(h * 131 + w + frames, frames, h, w)
    if shape == (34, 130):
        assert len(np.unique(rgb)) == 256
    t = torch.from_numpy(rgb).to(dev)
    ys = (torch.arange(hp, device=dev) - top).clamp(0, h - 1)
    xs = (torch.arange(wp, device=dev) - left).clamp(0, w - 1)
    # the quotient is the host's: a correctly rounded division (on the device torch multiplies by the reciprocal instead)
    want = (torch.from_numpy(rgb).float() / 255).to(dtype).to(dev).permute(0, 3, 1, 2)[:, :, ys][:, :, :, xs]
    # into x[1] of the network's input
    x = torch.full((2, frames, 3, hp, wp), SENTINEL[dtype], dtype=dtype, device=dev)
    assert S.rgb8_decode(t, x[1], pads) == 0
    assert torch.equal(x[1], want)
    assert bool((x[0] == SENTINEL[dtype]).all())
    # into a view whose row stride exceeds wp (and whose rows start on odd elements)
    big = torch.full((frames, 3, hp + 2, wp + 5), SENTINEL[dtype], dtype=dtype, device=dev)
    view = big[:, :, 1:1 + hp, 3:3 + wp]
    assert S.rgb8_decode(t, view, pads) == 0
    assert torch.equal(view, want)
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[:, :, 1:1 + hp, 3:3 + wp] = False
    assert bool((big[mask] == SENTINEL[dtype]).all())


# ---- quantise ---------------------------------------------------------------------------------------------------------

def quantised(x):
    """the host rule on a tensor of any float dtype [frames, 3, h, w] -> uint8 [frames, h, w, 3]"""
    y = torch.round(255 * x.float().clamp(0, 1))
    y = torch.where(torch.isnan(y), torch.zeros_like(y), y)
    return y.to(torch.uint8).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", [(3, 5), (7, 9), (33, 47)])
def test_quantise_of_a_crop_at_odd_offsets(S, dev, shape, dtype):
    h, w = shape
    g = torch.Generator().manual_seed(h * 100 + w)
    big = (torch.rand((2, 3, h + 4, w + 6), generator=g) * 1.5 - 0.25).to(dtype).to(dev)
    crop = big[:, :, 1:1 + h, 3:3 + w]
    out = torch.full((2, h, w, 3), 77, dtype=torch.uint8, device=dev)
    assert S.rgb8_quantise(crop, out) == 0
    assert torch.equal(out, quantised(crop))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_quantise_of_every_16_bit_pattern(S, dev, dtype):
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)          # wraps: every pattern once
    x = bits.view(dtype).to(dev)
    assert x.numel() == 65536
    # 65536 = 3 * 149 * 146 + 274: one [1, 3, 149, 146] tensor (odd rows) and the rest as a [1, 3, 1, 274] row with repeats
    head = x[:3 * 149 * 146].view(1, 3, 149, 146)
    tail = torch.cat([x[3 * 149 * 146:], x[:3 * 274 - 274]]).view(1, 3, 1, 274)
    for planes in (head, tail):
        out = torch.empty((1,) + tuple(planes.shape[2:]) + (3,), dtype=torch.uint8, device=dev)
        assert S.rgb8_quantise(planes, out) == 0
        assert torch.equal(out, quantised(planes))


def test_quantise_of_float32_ties_and_specials(S, dev):
    k = np.arange(256, dtype=np.float32)
    exact = k / np.float32(255.0)
    values = [exact, np.nextafter(exact, np.float32(2)), np.nextafter(exact, np.float32(-1))]
    # values whose float32 product with 255 is exactly k + 0.5 (found by search around (k + 0.5) / 255), and their neighbours
    ties = []
    for kk in range(255):
        v = np.float32((kk + 0.5) / 255.0)
        for _ in range(8):
            p = np.float32(255.0) * v
            if p == np.float32(kk + 0.5):
                ties.append(v)
                break
            v = np.nextafter(v, np.float32(2) if p < kk + 0.5 else np.float32(-1))
    assert len(ties) > 100
    ties = np.array(ties, dtype=np.float32)
    values += [ties, np.nextafter(ties, np.float32(2)), np.nextafter(ties, np.float32(-1))]
    values.append(np.array([0.0, -0.0, 1.0, -1.0, 1.5, 2.0, -3.0, 1e30, -1e30, np.inf, -np.inf, np.nan, -np.nan, 1e-45, 0.5,
                            0.002, 0.998039], dtype=np.float32))
    values.append(np.random.default_rng(3).uniform(-0.2, 1.2, 4000).astype(np.float32))
    flat = np.concatenate(values)
    n = 3 * 5 * 7
    flat = np.concatenate([flat, np.zeros((-flat.size) % n, dtype=np.float32)])
    x = torch.from_numpy(flat).view(-1, 3, 5, 7).to(dev)
    out = torch.empty((x.shape[0], 5, 7, 3), dtype=torch.uint8, device=dev)
    assert S.rgb8_quantise(x, out) == 0
    assert torch.equal(out, quantised(x))
    want = np.nan_to_num(np.round(np.float32(255.0) * np.clip(flat, 0, 1)), nan=0.0).astype(np.uint8)
    assert np.array_equal(out.permute(0, 3, 1, 2).reshape(-1).cpu().numpy(), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
def test_quantise_of_decode_is_the_identity(S, dev, dtype):
    b = torch.arange(256, dtype=torch.uint8).repeat(3)[:765].view(1, 15, 17, 3).contiguous().to(dev)
    assert len(torch.unique(b)) == 256
    x = torch.empty((1, 3, 15, 17), dtype=dtype, device=dev)
    back = torch.empty_like(b)
    assert S.rgb8_decode(b, x) == 0 and S.rgb8_quantise(x, back) == 0
    assert torch.equal(back, b)


# ---- score ------------------------------------------------------------------------------------------------------------

def run_score(S, dev, a, b, with_diff=True):
    """-> (uint64 sums [frames, 2] as numpy, difference picture as numpy or None); the workspace prefilled with 0xFF"""
    frames, h, w, _c = a.shape
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    sums = torch.full((frames, 2), -1, dtype=torch.int64, device=dev)
    work = torch.full((S.rgb8_score_workspace_bytes(frames, h, w),), 0xFF, dtype=torch.uint8, device=dev)
    diff = torch.full(a.shape, 7, dtype=torch.uint8, device=dev) if with_diff else None
    assert S.rgb8_score(ta, tb, sums, work, diff) == 0
    return sums.cpu().numpy().view(np.uint64), None if diff is None else diff.cpu().numpy()


def host_score(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    sums = np.stack([np.abs(d).sum(axis=(1, 2, 3)), (d * d).sum(axis=(1, 2, 3))], axis=1)
    return sums.astype(np.uint64), ((128 + d) & 0xFF).astype(np.uint8)


@pytest.mark.parametrize("frames,shape", [(1, (1, 1)), (1, (1, 5)), (3, (3, 5)), (2, (7, 9)), (2, (34, 130))])
def test_score_sums_and_difference_picture(S, dev, frames, shape):
    h, w = shape
    a, b = picture(11 + h, frames, h, w), picture(13 + w, frames, h, w)
    want_sums, want_diff = host_score(a, b)
    sums, diff = run_score(S, dev, a, b)
    assert np.array_equal(sums, want_sums) and np.array_equal(diff, want_diff)
    sums2, none = run_score(S, dev, a, b, with_diff=False)                 # without the picture: the same sums
    assert none is None and np.array_equal(sums2, want_sums)
    sums3, diff3 = run_score(S, dev, a, b)                                 # again: the same bits
    assert np.array_equal(sums3, sums) and np.array_equal(diff3, diff)
    zero, flat = run_score(S, dev, a, a.copy())                            # equal pictures
    assert not zero.any() and bool((flat == 128).all())


def test_score_of_a_frame_that_needs_a_second_trip_and_64_bits(S, dev):
    """3 h w / 16 trips exceed the header's 1024 workgroups of 256 lanes, so lanes make a second trip; all 255 against all 0
    gives 3 h w * 255^2 > 2^32."""
    h, w = 1025, 1367
    n = 3 * h * w
    assert (n + 15) // 16 > 1024 * 256 and n % 16 != 0 and n * 65025 > 1 << 32
    a, b = np.full((1, h, w, 3), 255, dtype=np.uint8), np.zeros((1, h, w, 3), dtype=np.uint8)
    sums, diff = run_score(S, dev, a, b)
    assert sums.tolist() == [[n * 255, n * 65025]] and bool((diff == 127).all())
    sums, diff = run_score(S, dev, b, a)
    assert sums.tolist() == [[n * 255, n * 65025]] and bool((diff == 129).all())
    a = picture(29, 1, h, w)
    b = np.roll(a, 5, axis=2)
    want_sums, want_diff = host_score(a, b)
    sums, diff = run_score(S, dev, a, b)
    assert np.array_equal(sums, want_sums) and np.array_equal(diff, want_diff)


# ---- the loop both ways -----------------------------------------------------------------------------------------------

def stub_model(x):
    mid = (x[0] + x[1]) * 0.5
    return [mid, mid], None, None, None


class Counting:
    def __init__(self):
        self.batches = []

    def __call__(self, x):
        self.batches.append(x.shape[1])
        return stub_model(x)


def make_tree(png, root):
    """scenes s0 .. s6 of sizes A, A, B, A, A, A, A; a grey scene after s3 and a scene without its second file after s4;
    no ground truth for s1, RGBA ground truth for s4"""
    rng = np.random.default_rng(31)
    data, gt = os.path.join(root, "data"), os.path.join(root, "gt")
    sizes = {"s0": A, "s1": A, "s2": B, "s3": A, "s4": A, "s5": A, "s6": A}
    for scene, (h, w) in sizes.items():
        os.makedirs(os.path.join(data, scene))
        os.makedirs(os.path.join(gt, scene))
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        b = np.clip(a.astype(np.int16) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
        png.write_png(os.path.join(data, scene, "frame10.png"), a)
        png.write_png(os.path.join(data, scene, "frame11.png"), b)
        truth = np.clip(a.astype(np.int16) + rng.integers(-5, 6, a.shape), 0, 255).astype(np.uint8)
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


@pytest.fixture(scope="module")
def tree(png, tmp_path_factory):
    return make_tree(png, str(tmp_path_factory.mktemp("still_tree")))


@pytest.mark.parametrize("precision", [dict(), dict(dtype=torch.bfloat16), dict(autocast=torch.float16)],
                         ids=["fp32", "bf16", "autocast-fp16"])
def test_the_loop_gives_the_same_files_and_tuples_both_ways(png, dev, tree, tmp_path, precision):
    data, gt = tree
    runs = {}
    for name, kw in (("host", dict()), ("gpu", dict(gpu_io=True)), ("gpu3", dict(gpu_io=True, scenes_per_step=3))):
        model, out = Counting(), str(tmp_path / name)
        res = png.interpolate_png_tree(model, data, out, dev, gt_dir=gt, **kw, **precision)
        runs[name] = (model.batches, res, files_of(out))
    assert runs["host"][0] == [1] * 7 and runs["gpu"][0] == [1] * 7 and runs["gpu3"][0] == [2, 1, 3, 1]
    _b, res, files = runs["host"]
    assert [r[0] for r in res] == ["s0", "s1", "s2", "s3", "s4", "s5", "s6"] and res[1] == ("s1", None, None)
    assert all(len(r) == 3 and r[1] > 0 and 0 < r[2] < 100 for r in res if r[0] != "s1")
    assert len(files) == 7 + 6
    for name in ("gpu", "gpu3"):
        assert runs[name][1] == res, name
        assert runs[name][2] == files, name


def test_the_loop_s_ssim_on_the_device(png, dev, tree, tmp_path):
    data, gt = tree
    # a second ground-truth tree in which s5's is the result itself
    first = png.interpolate_png_tree(stub_model, data, str(tmp_path / "first"), dev, gt_dir=gt)
    assert len(first) == 7
    gt2 = str(tmp_path / "gt2")
    for scene in ("s0", "s2", "s5"):
        os.makedirs(os.path.join(gt2, scene))
        src = os.path.join(str(tmp_path / "first") if scene == "s5" else gt, scene, "frame10i11.png")
        png.write_png(os.path.join(gt2, scene, "frame10i11.png"), png.read_png(src))
    host = png.interpolate_png_tree(stub_model, data, str(tmp_path / "host"), dev, gt_dir=gt2, ssim=True)
    for n in (1, 3):
        got = png.interpolate_png_tree(stub_model, data, str(tmp_path / ("gpu%d" % n)), dev, gt_dir=gt2, ssim=True,
                                       gpu_io=True, scenes_per_step=n)
        assert [r[:3] for r in got] == [r[:3] for r in host]
        for g, hst in zip(got, host):
            assert len(g) == 4
            if hst[3] is None:
                assert g[3] is None and g[0] not in ("s0", "s2", "s5")
                continue
            h, w = B if g[0] == "s2" else A
            bound = (32 + (h - 6) * (w - 6)) * 2.0 ** -53 + 2.0 ** -52     # tests/test_gpu_ssim.py::tolerance(h, w) + 2^-52
            assert abs(g[3] - hst[3]) <= bound, (g, hst)
        assert got[5][0] == "s5" and got[5][1:] == (0.0, 100.0, 1.0)
        assert 0.0 < got[0][3] < 1.0
        assert files_of(str(tmp_path / ("gpu%d" % n))) == files_of(str(tmp_path / "host"))
    with pytest.raises(ValueError):                                        # a 7 x 7 window does not fit
        small = str(tmp_path / "small")
        os.makedirs(os.path.join(small, "t"))
        for name in ("frame10.png", "frame11.png"):
            png.write_png(os.path.join(small, "t", name), np.zeros((6, 9, 3), dtype=np.uint8))
        png.interpolate_png_tree(stub_model, small, str(tmp_path / "out_small"), dev, ssim=True, gpu_io=True)


# ---- the command line -------------------------------------------------------------------------------------------------

def test_still_image_demo_command_line_on_the_device(tmp_path, capsys):
    """tools/demo_middlebury.py --gpu-io --ssim on the two 128 x 192 scenes of tests/test_gpu_network.py's command-line test
    (that size at batch 1: no new MIOpen searches).  Not compared with the host route: MIOpen's convolutions are not
    bit-reproducible."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import importlib
    demo = importlib.import_module("demo_middlebury")
    import networks
    rng = np.random.default_rng(9)
    data, gt, out = tmp_path / "data", tmp_path / "gt", tmp_path / "out"
    for scene, (h, w) in (("Alpha", (128, 192)), ("Beta", (128, 192))):
        os.makedirs(str(data / scene))
        os.makedirs(str(gt / scene))
        base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        networks.write_png(str(data / scene / "frame10.png"), base)
        networks.write_png(str(data / scene / "frame11.png"), np.roll(base, 2, axis=1))
        if scene == "Alpha":
            networks.write_png(str(gt / scene / "frame10i11.png"), np.roll(base, 1, axis=1))
    demo.main(["--data", str(data), "--gt", str(gt), "--output", str(out), "--model", "MEMC_Net", "--gpu-io", "--ssim"])
    text = capsys.readouterr().out
    line = [ln for ln in text.splitlines() if ln.startswith("Alpha")]
    assert len(line) == 1 and "interpolation error / PSNR / SSIM :" in line[0]
    err, psnr, ssim = (float(v) for v in line[0].split(":")[1].split("/"))
    assert np.isfinite([err, psnr, ssim]).all() and 0.0 <= err <= 255.0 and 0.0 <= psnr <= 100.0 and -1.0 <= ssim <= 1.0
    assert "Beta" in text and "no ground truth" in text and "for all 1 images" in text
    for scene in ("Alpha", "Beta"):
        rec = networks.read_png(str(out / scene / "frame10i11.png"))
        assert rec.shape == (128, 192, 3) and rec.dtype == np.uint8
    diffs = [f for f in os.listdir(str(out / "Alpha")) if f.startswith("frame10i11_diff")]
    assert len(diffs) == 1 and networks.read_png(str(out / "Alpha" / diffs[0])).shape == (128, 192, 3)
    assert "%.4f" % err in diffs[0]


def test_the_command_line_hands_its_switches_to_the_loop(tmp_path, monkeypatch):
    """the switches reach interpolate_png_tree by name; a default run passes none of them (the call it always made)"""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import importlib
    demo = importlib.import_module("demo_middlebury")
    import networks
    seen = []
    monkeypatch.setattr(networks, "interpolate_png_tree", lambda *a, **kw: (seen.append(kw), [])[1])
    base = ["--data", str(tmp_path), "--output", str(tmp_path / "out"), "--model", "MEMC_Net"]
    demo.main(base)
    demo.main(base + ["--gpu-io", "--scenes-per-step", "8", "--ssim", "--first", "im1.png", "--second", "im3.png",
                      "--middle", "im2.png", "--precision", "bf16"])
    assert seen[0] == dict(gt_dir=None, which=1)
    assert seen[1] == dict(gt_dir=None, which=1, gpu_io=True, scenes_per_step=8, ssim=True, first="im1.png", second="im3.png",
                           middle="im2.png", dtype=torch.bfloat16, autocast=None)
