"""The frame I/O kernels of libmemc_hip_video.so (include/memc_video.h) and the demo loop's gpu_io path against
networks/yuv_io.py on the host: decode over every (Y, U, V) triple and into padded slices of the network's input, the
quantiser on its ties, encode over every (R, G, B) triple, the integer luma sums, and the loop's file and scores.

Everything is compared byte for byte (torch.equal) but the encoder's Y plane at ORDER-SENSITIVE triples: the float64 sum
m0 r + m1 g + m2 b of the luma row truncates to another level under another summation order at 0.034 % of the RGB
triples (`luma_orders`: numpy's matmul, (a+b)+c, a+(b+c), (a+c)+b).  There the kernel's byte must lie within one level of
Yuv420Writer's; everywhere else it must equal it."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2), (6, 10), (34, 130), (128, 256), (130, 128), (720, 1280)]


@pytest.fixture(scope="module")
def V():
    import my_package._ext.my_lib_video as M
    M.lib()
    return M


@pytest.fixture(scope="module")
def Y():
    import networks.yuv_io as M
    return M


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def luma_orders(Y, rgb):
    """the truncated luma of uint8 [..., 3] under the four host evaluations: (matmul's bytes, order-sensitive mask)"""
    x = rgb / 255.0
    m = Y.YUV_FROM_RGB[0]
    p0, p1, p2 = m[0] * x[..., 0], m[1] * x[..., 1], m[2] * x[..., 2]
    first = (255.0 * Y.rgb_to_yuv(x)[..., 0]).astype(np.uint8)
    sensitive = np.zeros(first.shape, dtype=bool)
    for other in ((p0 + p1) + p2, p0 + (p1 + p2), (p0 + p2) + p1):
        other = (255.0 * other).astype(np.uint8)
        assert int(np.abs(other.astype(np.int16) - first).max()) <= 1
        sensitive |= other != first
    return first, sensitive


def host_decode(Y, path, buf, frames, h, w):
    with open(path, "wb") as f:
        f.write(buf.tobytes())
    rd = Y.Yuv420Reader(path, h, w, to_rgb=True)
    try:
        return np.stack([rd.read(k)[0] for k in range(frames)])
    finally:
        rd.close()


def host_encode(Y, path, rgb):
    wr = Y.Yuv420Writer(path, from_rgb=True)
    try:
        for frame in rgb:
            wr.write(frame)
    finally:
        wr.close()
    return np.fromfile(path, dtype=np.uint8).reshape(len(rgb), -1)


def split(i420, h, w):
    """[frames, h*w*3/2] -> Y [frames, h, w], U and V [frames, h/2, w/2]"""
    n, ny, nc = i420.shape[0], h * w, (h // 2) * (w // 2)
    return (i420[:, :ny].reshape(n, h, w), i420[:, ny:ny + nc].reshape(n, h // 2, w // 2),
            i420[:, ny + nc:].reshape(n, h // 2, w // 2))


def gpu_encode(V, dev, rgb):
    n, h, w, _ = rgb.shape
    out = torch.empty((n, V.frame_bytes(h, w)), dtype=torch.uint8, device=dev)
    assert V.i420_encode(torch.from_numpy(rgb).to(dev), n, h, w, out) == 0
    return out.cpu().numpy()


def check_encode(Y, got, want, rgb, h, w):
    """U and V equal; Y equal where the host's orders agree, within one level elsewhere.  Returns the sensitive count."""
    gy, gu, gv = split(got, h, w)
    wy, wu, wv = split(want, h, w)
    assert np.array_equal(gu, wu) and np.array_equal(gv, wv)
    first, sensitive = luma_orders(Y, rgb)
    assert np.array_equal(first, wy)                       # the writer's bytes are the matmul's
    assert np.array_equal(gy[~sensitive], wy[~sensitive])
    assert int(np.abs(gy.astype(np.int16) - wy)[sensitive].max(initial=0)) <= 1
    return int(sensitive.sum())


def test_decode_every_yuv_triple(V, Y, dev, tmp_path):
    """One 4096 x 4096 frame: block k = by * 2048 + bx has U = k >> 14, V = (k >> 6) & 255, its four Y 4 (k & 63) + {0..3}."""
    n = 4096
    k = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    yp = (4 * (k & 63)).repeat(2, axis=0).repeat(2, axis=1)
    yp[0::2, 1::2] += 1
    yp[1::2, 0::2] += 2
    yp[1::2, 1::2] += 3
    buf = np.concatenate([yp.ravel(), (k >> 14).ravel(), ((k >> 6) & 255).ravel()]).astype(np.uint8)
    triples = (yp.astype(np.int64) << 16) | ((k >> 14) << 8).repeat(2, 0).repeat(2, 1) | ((k >> 6) & 255).repeat(2, 0).repeat(2, 1)
    assert np.array_equal(np.sort(triples.ravel()), np.arange(1 << 24))          # every triple once
    want = host_decode(Y, str(tmp_path / "all.yuv"), buf, 1, n, n)
    rgb = torch.empty((1, n, n, 3), dtype=torch.uint8, device=dev)
    assert V.i420_decode(torch.from_numpy(buf).to(dev), 1, n, n, rgb=rgb) == 0
    assert torch.equal(rgb.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("h,w", SHAPES)
def test_decode_into_a_padded_slice(V, Y, dev, tmp_path, h, w, frames):
    """Both outputs at once, the planes into a slice (rows and planes longer than the extent) of a NaN-filled
    [2, B, 3, Hp + 1, Wp + 5]: every element of the slice is F.pad(float32(rgb) / 255, replicate), nothing else moves."""
    from networks.inference import pad_amounts
    rng = np.random.default_rng(h * 131 + w + frames)
    buf = rng.integers(0, 256, frames * Y.frame_bytes(h, w), dtype=np.uint8)
    want = host_decode(Y, str(tmp_path / "clip.yuv"), buf, frames, h, w)
    pads = pad_amounts(h, w)
    hp, wp = h + pads[2] + pads[3], w + pads[0] + pads[1]
    big = torch.full((2, frames, 3, hp + 1, wp + 5), float("nan"), device=dev)
    rgb = torch.full((frames, h, w, 3), 7, dtype=torch.uint8, device=dev)
    assert V.i420_decode(torch.from_numpy(buf).to(dev), frames, h, w, rgb=rgb, planes=big[1, :, :, :hp, :wp], pads=pads) == 0
    assert torch.equal(rgb.cpu(), torch.from_numpy(want))
    planes = torch.from_numpy(np.transpose(want, (0, 3, 1, 2)).astype(np.float32) / 255.0)
    exp = torch.full(big.shape, float("nan"))
    exp[1, :, :, :hp, :wp] = F.pad(planes, pads, mode="replicate")
    assert torch.equal(torch.nan_to_num(big.cpu(), nan=-7.0), torch.nan_to_num(exp, nan=-7.0))


def test_decode_planes_alone_and_rgb_alone(V, Y, dev, tmp_path):
    h, w, frames = 34, 130, 2
    buf = np.random.default_rng(3).integers(0, 256, frames * Y.frame_bytes(h, w), dtype=np.uint8)
    want = host_decode(Y, str(tmp_path / "clip.yuv"), buf, frames, h, w)
    src = torch.from_numpy(buf).to(dev)
    pads = (3, 0, 0, 5)
    planes = torch.full((frames, 3, h + 5, w + 3), float("nan"), device=dev)
    assert V.i420_decode(src, frames, h, w, planes=planes, pads=pads) == 0
    exp = F.pad(torch.from_numpy(np.transpose(want, (0, 3, 1, 2)).astype(np.float32) / 255.0), pads, mode="replicate")
    assert torch.equal(planes.cpu(), exp)
    rgb = torch.empty((frames, h, w, 3), dtype=torch.uint8, device=dev)
    assert V.i420_decode(src, frames, h, w, rgb=rgb) == 0
    assert torch.equal(rgb.cpu(), torch.from_numpy(want))
    assert V.i420_decode(src, frames, h, w) == -1                       # neither output


@pytest.mark.parametrize("h,w", [(6, 10), (34, 130), (130, 128)])
def test_quantise_a_crop_window(V, dev, h, w):
    """A random window of a larger tensor: ties (k + 0.5) / 255, values below 0 and above 1 -- numpy's round of the float32
    product, as the loop's host path computes it."""
    rng = np.random.default_rng(h + w)
    B, H, W = 2, h + 37, w + 71
    x = rng.uniform(-0.5, 1.5, (B, 3, H, W)).astype(np.float32)
    flat = x.reshape(-1)
    ties = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)
    flat[rng.choice(flat.size, 4 * ties.size, replace=False)] = np.tile(ties, 4)
    flat[rng.choice(flat.size, 64, replace=False)] = np.tile(np.float32([0.0, 1.0, -0.0, 1.0 + 2 ** -23, -2 ** -30, 0.5 / 255,
                                                                         254.5 / 255, 2.0]), 8)
    top, left = int(rng.integers(0, 38)), int(rng.integers(0, 72))
    crop = torch.from_numpy(x).to(dev)[:, :, top:top + h, left:left + w]
    want = np.round(255.0 * crop.clamp(0.0, 1.0).cpu().numpy()).astype(np.uint8)
    rgb = torch.empty((B, h, w, 3), dtype=torch.uint8, device=dev)
    assert V.rgb_quantise(crop, rgb) == 0
    assert torch.equal(rgb.cpu(), torch.from_numpy(np.transpose(want, (0, 2, 3, 1)).copy()))


def test_encode_every_rgb_triple(V, Y, dev, tmp_path):
    """All 2^24 triples as a 4096 x 4096 frame, four times: shifted by (0 | 1, 0 | 1) with wrap-around, so that every triple
    lands on an even row and an even column in one of them.  Frame 0 against Yuv420Writer's file; the shifted frames against
    the same per-triple bytes, shifted (the writer's rule is per pixel)."""
    n = 4096
    idx = np.arange(1 << 24, dtype=np.uint32).reshape(n, n)
    base = np.stack((idx >> 16, (idx >> 8) & 255, idx & 255), axis=-1).astype(np.uint8)
    want0 = host_encode(Y, str(tmp_path / "all.yuv"), base[None])
    yuv = Y.rgb_to_yuv(base / 255.0)
    full = [(255.0 * yuv[..., 0]).astype(np.uint8)] + [(255.0 * np.clip(yuv[..., c] + 0.5, 0.0, 1.0)).astype(np.uint8) for c in (1, 2)]
    del yuv
    first, sensitive = luma_orders(Y, base)
    count = int(sensitive.sum())
    print("order-sensitive RGB triples on this host: %d of 2^24" % count)
    assert count <= 16384
    assert np.array_equal(first, full[0])
    shifts = [(0, 0), (0, 1), (1, 0), (1, 1)]
    rgb = np.stack([np.roll(base, s, axis=(0, 1)) for s in shifts])
    got = gpu_encode(V, dev, rgb)
    gy, gu, gv = split(got, n, n)
    wy0, wu0, wv0 = split(want0, n, n)
    worst = 0
    for k, s in enumerate(shifts):
        wy, wu, wv = (np.roll(p, s, axis=(0, 1)) for p in full)
        sens = np.roll(sensitive, s, axis=(0, 1))
        if k == 0:
            assert np.array_equal(wy, wy0[0]) and np.array_equal(wu[::2, ::2], wu0[0]) and np.array_equal(wv[::2, ::2], wv0[0])
        assert np.array_equal(gu[k], wu[::2, ::2]) and np.array_equal(gv[k], wv[::2, ::2]), s
        assert np.array_equal(gy[k][~sens], wy[~sens]), s
        worst = max(worst, int(np.abs(gy[k].astype(np.int16) - wy)[sens].max(initial=0)))
        print("shift %s: Y bytes that differ from the writer's at order-sensitive triples: %d" % (s, int((gy[k] != wy).sum())))
    assert worst <= 1


@pytest.mark.parametrize("h,w", [(6, 10), (34, 130)])
def test_encode_three_frames(V, Y, dev, tmp_path, h, w):
    rgb = np.random.default_rng(h * w).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    check_encode(Y, gpu_encode(V, dev, rgb), host_encode(Y, str(tmp_path / "clip.yuv"), rgb), rgb, h, w)


def insensitive_frames(Y, rng, shape):
    """random uint8 RGB whose order-sensitive triples are replaced by black (which no order moves)"""
    rgb = rng.integers(0, 256, shape, dtype=np.uint8)
    rgb[luma_orders(Y, rgb)[1]] = 0
    assert not luma_orders(Y, rgb)[1].any()
    return rgb


def host_sums(Y, rec, gt):
    """luma_scores' planes, summed as integers"""
    ry = (Y.rgb_to_yuv(rec / 255.0)[..., 0] * 255.0).astype(np.uint8).astype(np.int64)
    gy = (Y.rgb_to_yuv(gt / 255.0)[..., 0] * 255.0).astype(np.uint8).astype(np.int64)
    d = (ry - gy).reshape(len(rec), -1)
    return np.stack((np.abs(d).sum(axis=1), (d * d).sum(axis=1)), axis=1)


def gpu_sums(V, dev, a, b):
    n, h, w, _ = a.shape
    sums = torch.full((n, 2), -1, dtype=torch.int64, device=dev)
    work = torch.empty(V.luma_score_workspace_bytes(n, h, w), dtype=torch.uint8, device=dev)
    assert V.luma_score(torch.as_tensor(a).to(dev), torch.as_tensor(b).to(dev), n, h, w, sums, work) == 0
    return sums.cpu().numpy()


@pytest.mark.parametrize("h,w", [(2, 2), (6, 10), (34, 130), (130, 128), (128, 256)])
def test_luma_sums(V, Y, dev, h, w):
    rng = np.random.default_rng(h + 7 * w)
    a, b = insensitive_frames(Y, rng, (3, h, w, 3)), insensitive_frames(Y, rng, (3, h, w, 3))
    b[1] = a[1]                                            # an identical pair among them
    want = host_sums(Y, a, b)
    got = gpu_sums(V, dev, a, b)
    assert np.array_equal(got, want)
    assert np.array_equal(gpu_sums(V, dev, a, b), got)     # a second run: the same bits
    assert tuple(got[1]) == (0, 0) and Y.scores_from_sums(got[1, 0], got[1, 1], h * w) == (0.0, 100.0)
    for k in (0, 2):                                       # the host's two numbers from the sums
        err, psnr = Y.luma_scores(a[k], b[k])
        got_err, got_psnr = Y.scores_from_sums(got[k, 0], got[k, 1], h * w)
        assert abs(got_err - err) <= 1e-12 and abs(got_psnr - psnr) <= 1e-12


def test_luma_sums_do_not_overflow(V, Y, dev):
    """all-0 against all-255 at 4096 x 4096: 2^24 * L and 2^24 * L^2 for white's luma level L, the second beyond 2^39.  White is
    an order-sensitive triple on the host (0.299 + 0.587 + 0.114 is 1 under one order and 1 - 2^-53 under another: L is 255 or 254), so L is luma_scores' level where the host's orders agree and one of their levels where they do not -- the
    same L in both sums, every pixel."""
    n = 4096
    white = np.full((1, 1, 1, 3), 255, dtype=np.uint8)
    first, sensitive = luma_orders(Y, white)
    level = int(first.ravel()[0])
    levels = [level] if not sensitive.any() else [level - 1, level, level + 1]
    assert not luma_orders(Y, np.zeros((1, 1, 1, 3), dtype=np.uint8))[1].any()
    a = torch.zeros((1, n, n, 3), dtype=torch.uint8)
    b = torch.full((1, n, n, 3), 255, dtype=torch.uint8)
    got = gpu_sums(V, dev, a, b)
    print("white: luma level %d under matmul, order-sensitive %s; sums %s" % (level, bool(sensitive.any()), got.tolist()))
    assert got.tolist() in [[[(1 << 24) * lv, (1 << 24) * lv * lv]] for lv in levels]
    assert got[0, 0] > 1 << 31 and got[0, 1] > 1 << 39             # neither fits 32 bits signed; the squares need 40
    assert np.array_equal(gpu_sums(V, dev, a, b), got)
    assert gpu_sums(V, dev, b, b).tolist() == [[0, 0]]


def stub_model(x):
    mid = (x[0] + x[1]) * 0.5
    return [mid, mid], None, None, None


def clean_clip(Y, path, h, w):
    """A five-frame clip of random bytes (the first seed) for which the host alone says that, of the two scored frames, one
    involves no order-sensitive byte (neither in the result nor in the frame it is scored against) and the other does.
    Returns (per written frame: its RGB bytes, per scored frame: the number of sensitive pixels involved)."""
    fb = Y.frame_bytes(h, w)
    for seed in range(400):
        buf = np.random.default_rng(seed).integers(0, 256, 5 * fb, dtype=np.uint8)
        rgb = host_decode(Y, path, buf, 5, h, w)
        planes = rgb.astype(np.float32) / np.float32(255.0)
        written, involved = [], []
        for i in (0, 2):
            rec = np.round(np.float32(255.0) * np.clip((planes[i] + planes[i + 2]) * np.float32(0.5), 0.0, 1.0)).astype(np.uint8)
            written += [rgb[i], rec]
            involved.append(int(luma_orders(Y, rec)[1].sum() + luma_orders(Y, rgb[i + 1])[1].sum()))
        if min(involved) == 0 and max(involved) > 0:
            return written, involved
    raise AssertionError("no seed below 400 gives such a clip")


def test_the_loop_both_ways(V, Y, dev, tmp_path):
    import networks
    h, w = 34, 130
    src = str(tmp_path / "in.yuv")
    written, involved = clean_clip(Y, src, h, w)
    outs, scores = {}, {}
    for name, kw in (("host", dict()), ("gpu", dict(gpu_io=True)), ("gpu2", dict(gpu_io=True, pairs_per_step=2))):
        dst = str(tmp_path / (name + ".yuv"))
        scores[name] = networks.interpolate_yuv_sequence(stub_model, src, dst, h, w, dev, **kw)
        outs[name] = np.fromfile(dst, dtype=np.uint8)
    assert outs["host"].size == 4 * Y.frame_bytes(h, w)                 # frame 0, result 1, frame 2, result 3
    assert np.array_equal(outs["gpu2"], outs["gpu"]) and scores["gpu2"] == scores["gpu"]
    rgb = np.stack(written)
    assert np.array_equal(outs["host"].reshape(4, -1), host_encode(Y, str(tmp_path / "again.yuv"), rgb))
    check_encode(Y, outs["gpu"].reshape(4, -1), outs["host"].reshape(4, -1), rgb, h, w)
    assert [s[0] for s in scores["gpu"]] == [s[0] for s in scores["host"]] == [1, 3]
    for got, want, n in zip(scores["gpu"], scores["host"], involved):
        print("frame %d: gpu %r host %r, order-sensitive pixels involved: %d" % (got[0], got[1:], want[1:], n))
        if n == 0:
            assert abs(got[1] - want[1]) <= 1e-12 and abs(got[2] - want[2]) <= 1e-12
        else:                                              # each such pixel moves |dY| by at most one level
            assert abs(got[1] - want[1]) <= n / float(h * w) + 1e-12


def test_gpu_io_needs_a_gpu_device(Y, tmp_path):
    src = str(tmp_path / "in.yuv")
    open(src, "wb").write(bytes(3 * Y.frame_bytes(2, 2)))
    with pytest.raises(ValueError):
        Y.interpolate_yuv_sequence(stub_model, src, str(tmp_path / "out.yuv"), 2, 2, "cpu", gpu_io=True)
