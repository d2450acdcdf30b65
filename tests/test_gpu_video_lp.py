"""The fp16 / bf16 frame I/O kernels of libmemc_hip_video_lp.so (include/memc_video_lp.h) and the demo loop's gpu_io path with a
half dtype, against torch's own casts and the host route of networks/yuv_io.py.

Everything is compared exactly (torch.equal, ==): decode is (rgb.float() / 255).to(T) of the float32 library's bytes,
replicate-padded; quantise is round-half-even of 255 * clamp(float32(x), 0, 1) over every bit pattern of T; the loop's two
routes write the same file and return the same scores on a clip that holds no order-sensitive RGB triple (memc_video.h: the
encoder's Y moves by one level between summation orders at 0.034 % of the triples; the clip avoids them, so that what is
compared is the half I/O and nothing else).  With ssim=True the files and the first three elements of every score tuple are
identical again; the fourth is libmemc_hip_ssim.so's float64 mean, which sums the window values in another order than numpy
and is held to that library's own bound (tests/test_gpu_ssim.py: (32 + windows) * 2^-53; observed here: 3 to 7 * 10^-18)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HALVES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
SHAPES = [(2, 2), (6, 10), (34, 130), (130, 128)]


@pytest.fixture(scope="module")
def V():
    import my_package._ext.my_lib_video as M
    M.lib()
    return M


@pytest.fixture(scope="module")
def VL():
    import my_package._ext.my_lib_video_lp as M
    M.lib()
    return M


@pytest.fixture(scope="module")
def Y():
    import networks.yuv_io as M
    return M


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


# ---- decode ------------------------------------------------------------------------------------------------------------

def reference_rgb(V, src, frames, h, w):
    """the float32 library's bytes for the same I420 bytes"""
    rgb = torch.empty((frames, h, w, 3), dtype=torch.uint8, device=src.device)
    assert V.i420_decode(src, frames, h, w, rgb=rgb) == 0
    return rgb


def reference_planes(rgb, pads, dtype):
    return F.pad((rgb.float() / 255).permute(0, 3, 1, 2), pads, mode="replicate").to(dtype)


def same_bits(a, b):
    """torch.equal on the 16-bit patterns: NaN equals NaN of the same bits"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
@pytest.mark.parametrize("odd_pads", [False, True], ids=["demo_pads", "pads_3_0_0_5"])
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("h,w", SHAPES)
def test_decode_into_a_padded_slice(V, VL, Y, dev, h, w, frames, odd_pads, dtype):
    """Both outputs at once, the planes into a slice of a NaN-filled [2, B, 3, Hp + 1, Wp + 5] that starts at column 1 (its
    rows start on an odd element: 2-byte alignment only): every element of the slice is the reference, nothing else moves."""
    from networks.inference import pad_amounts
    rng = np.random.default_rng(h * 131 + w + frames)
    src = torch.from_numpy(rng.integers(0, 256, frames * Y.frame_bytes(h, w), dtype=np.uint8)).to(dev)
    want_rgb = reference_rgb(V, src, frames, h, w)
    pads = (3, 0, 0, 5) if odd_pads else pad_amounts(h, w)
    hp, wp = h + pads[2] + pads[3], w + pads[0] + pads[1]
    big = torch.full((2, frames, 3, hp + 1, wp + 5), float("nan"), dtype=dtype, device=dev)
    view = big[1, :, :, :hp, 1:1 + wp]
    assert view.stride(3) == 1
    assert any((view.storage_offset() + r * view.stride(2)) % 2 for r in range(2))     # a row that starts on an odd element
    rgb = torch.full((frames, h, w, 3), 7, dtype=torch.uint8, device=dev)
    assert VL.i420_decode(src, frames, h, w, rgb=rgb, planes=view, pads=pads) == 0
    assert torch.equal(rgb, want_rgb)
    exp = torch.full_like(big, float("nan"))
    exp[1, :, :, :hp, 1:1 + wp] = reference_planes(want_rgb, pads, dtype)
    assert torch.equal(view, exp[1, :, :, :hp, 1:1 + wp])
    assert same_bits(big, exp)                                      # every element outside the slice is still NaN
    assert int(torch.isnan(big).sum()) == big.numel() - frames * 3 * hp * wp


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
def test_decode_planes_alone_and_rgb_alone(V, VL, Y, dev, dtype):
    h, w, frames = 34, 130, 2
    src = torch.from_numpy(np.random.default_rng(3).integers(0, 256, frames * Y.frame_bytes(h, w), dtype=np.uint8)).to(dev)
    want_rgb = reference_rgb(V, src, frames, h, w)
    pads = (3, 0, 0, 5)
    planes = torch.full((frames, 3, h + 5, w + 3), float("nan"), dtype=dtype, device=dev)
    assert VL.i420_decode(src, frames, h, w, planes=planes, pads=pads) == 0
    assert torch.equal(planes, reference_planes(want_rgb, pads, dtype))
    rgb = torch.empty((frames, h, w, 3), dtype=torch.uint8, device=dev)
    assert VL.i420_decode(src, frames, h, w, rgb=rgb) == 0
    assert torch.equal(rgb, want_rgb)
    assert VL.i420_decode(src, frames, h, w) == -1                      # neither output
    # this door is half only, the other float32 only; a w-stride other than 1 is refused
    f32 = torch.empty((frames, 3, h, w), dtype=torch.float32, device=dev)
    with pytest.raises(TypeError):
        VL.i420_decode(src, frames, h, w, planes=f32)
    with pytest.raises(TypeError):
        VL.rgb_quantise(f32, rgb)
    with pytest.raises(TypeError):
        V.i420_decode(src, frames, h, w, planes=f32.to(dtype))
    with pytest.raises(TypeError):
        VL.rgb_quantise(torch.empty((frames, 3, h, 2 * w), dtype=dtype, device=dev)[:, :, :, ::2], rgb)
    with pytest.raises(ValueError):
        VL.i420_decode(src, frames, h, w, planes=planes)                # the shape of another padding


def test_decode_every_yuv_triple_bf16(V, VL, dev):
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
    del triples, yp, k
    src = torch.from_numpy(buf).to(dev)
    want_rgb = reference_rgb(V, src, 1, n, n)
    rgb = torch.empty_like(want_rgb)
    planes = torch.empty((1, 3, n, n), dtype=torch.bfloat16, device=dev)
    assert VL.i420_decode(src, 1, n, n, rgb=rgb, planes=planes) == 0
    assert torch.equal(rgb, want_rgb)
    assert torch.equal(planes, reference_planes(want_rgb, (0, 0, 0, 0), torch.bfloat16))


# ---- quantise ----------------------------------------------------------------------------------------------------------

def host_quantise(x):
    """[B, 3, h, w] of T -> uint8 [B, h, w, 3]: numpy's round (ties to even) of the float32 product, NaN -> 0"""
    f = torch.nan_to_num(x.float().cpu(), nan=0.0).clamp(0.0, 1.0).numpy()
    return torch.from_numpy(np.transpose(np.round(np.float32(255.0) * f).astype(np.uint8), (0, 2, 3, 1)).copy())


def exact_ties(dtype):
    """the bit patterns of T whose widened value times 255 is exactly k + 0.5 (in float64: 24 x 8 bits, no rounding)"""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    p = bits.double() * 255.0
    return bits[(p > 0) & (p < 255) & (p - torch.floor(p) == 0.5)]


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
def test_quantise_every_bit_pattern(VL, dev, dtype):
    """All 65 536 patterns of T as a 256 x 256 plane, the three channels rotated by 0, 21 845 and 43 690 positions (a channel
    mix-up shows), a second frame with the pattern reversed."""
    base = torch.arange(65536, dtype=torch.int32)
    chans = torch.stack([torch.roll(base, -r) for r in (0, 21845, 43690)])
    both = torch.stack([chans, torch.flip(chans, dims=(1,))])                    # [2, 3, 65536]
    x = both.to(torch.int16).view(dtype).reshape(2, 3, 256, 256)
    # what the pattern holds by construction: NaN, both infinities, both zeros, values on either side of [0, 1], every
    # level, and the exact ties T can represent -- one per dtype: a tie k + 0.5 = 255 m 2^e needs 255 | 2k + 1, which
    # leaves k = 127 (x = 0.5) alone
    ties = exact_ties(dtype)
    assert ties.float().tolist() == [0.5]
    want = host_quantise(x)
    flat = x[0, 0].reshape(-1)
    assert int(torch.isnan(flat).sum()) > 0 and bool(torch.isinf(flat).any()) and bool((flat < 0).any()) and bool((flat > 1).any())
    assert len(torch.unique(want[0, :, :, 0])) == 256                            # all 256 levels are reached
    half = want[0, :, :, 0].reshape(-1)[flat == 0.5]
    assert half.tolist() == [128]                                                # 127.5 goes to the even level
    rgb = torch.full((2, 256, 256, 3), 9, dtype=torch.uint8, device=dev)
    assert VL.rgb_quantise(x.to(dev), rgb) == 0
    assert torch.equal(rgb.cpu(), want)
    nan = torch.isnan(x).permute(0, 2, 3, 1)
    assert int(rgb.cpu()[nan].max()) == 0                                        # NaN maps to 0


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
@pytest.mark.parametrize("h,w", [(6, 10), (34, 130), (130, 128)])
def test_quantise_a_crop_window(VL, dev, h, w, dtype):
    """A random window of a larger tensor (strides, 2-byte alignment): values below 0 and above 1, the tie, the ends."""
    rng = np.random.default_rng(h + w)
    B, H, W = 2, h + 37, w + 71
    x = torch.from_numpy(rng.uniform(-0.5, 1.5, (B, 3, H, W)).astype(np.float32)).to(dtype)
    flat = x.view(-1)
    special = torch.tensor([0.0, 1.0, -0.0, 0.5, 1.0 + 2.0 ** -7, -2.0 ** -14, 0.5 / 255, 254.5 / 255, 2.0, float("nan")]).to(dtype)
    flat[torch.from_numpy(rng.choice(flat.numel(), 8 * special.numel(), replace=False))] = special.repeat(8)
    top, left = int(rng.integers(0, 38)), 2 * int(rng.integers(0, 36)) + 1     # an odd column: rows start on an odd element
    crop = x.to(dev)[:, :, top:top + h, left:left + w]
    assert crop.stride(2) % 2 == 1 and crop.storage_offset() > 0
    want = host_quantise(crop)
    rgb = torch.empty((B, h, w, 3), dtype=torch.uint8, device=dev)
    assert VL.rgb_quantise(crop, rgb) == 0
    assert torch.equal(rgb.cpu(), want)


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
def test_round_trip(V, VL, Y, dev, dtype):
    """quantise(decode planes, cropped) gives the decoded bytes back"""
    from networks.inference import pad_amounts
    h, w, frames = 34, 130, 2
    src = torch.from_numpy(np.random.default_rng(5).integers(0, 256, frames * Y.frame_bytes(h, w), dtype=np.uint8)).to(dev)
    pads = pad_amounts(h, w)
    planes = torch.empty((frames, 3, h + pads[2] + pads[3], w + pads[0] + pads[1]), dtype=dtype, device=dev)
    rgb = torch.empty((frames, h, w, 3), dtype=torch.uint8, device=dev)
    assert VL.i420_decode(src, frames, h, w, rgb=rgb, planes=planes, pads=pads) == 0
    back = torch.full_like(rgb, 3)
    assert VL.rgb_quantise(planes[:, :, pads[2]:pads[2] + h, pads[0]:pads[0] + w], back) == 0
    assert torch.equal(back, rgb) and torch.equal(rgb, reference_rgb(V, src, frames, h, w))


# ---- the loop both ways ------------------------------------------------------------------------------------------------

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


def stub_model(x):
    """computes in the dtype it is given"""
    mid = 0.5 * x[0] + 0.5 * x[1]
    return [x[0], mid], None, None, None


def stub_model_float32(x):
    """answers in float32 whatever it is given"""
    mid = 0.5 * x[0].float() + 0.5 * x[1].float()
    return [x[0].float(), mid], None, None, None


def stub_bytes(rgb_a, rgb_b, fed, computes=None, answers=None):
    """the mean of two uint8 [h, w, 3] frames as bytes: planes of dtype `fed`, the arithmetic in `computes` and the answer in
    `answers` (both: as fed)"""
    a, b = (torch.from_numpy(f.astype(np.float32) / np.float32(255.0)).to(fed).to(computes or fed) for f in (rgb_a, rgb_b))
    mid = (0.5 * a + 0.5 * b).to(answers or computes or fed)
    return np.round(np.float32(255.0) * mid.float().clamp(0.0, 1.0).numpy()).astype(np.uint8)


# (fed, computes, answers) of every stub the tests below run
VARIANTS = [(torch.float32, None, None)] + [v for T in HALVES for v in ((T, None, None), (T, torch.float32, None),
                                                                        (torch.float32, None, T))]


H, W = 34, 130


@pytest.fixture(scope="module")
def clip(Y, tmp_path_factory):
    """tests/test_gpu_video_io.py's insensitive_frames idea, carried to where the loop's RGB bytes arise: five frames of
    random I420 bytes in which every RGB triple the loop encodes or scores -- the decoded frames and the stub's results in
    every precision the tests below run (VARIANTS) -- is one whose luma no summation order moves.  A pixel that is not gets
    a new Y byte."""
    path = str(tmp_path_factory.mktemp("lp_loop") / "in.yuv")
    rng = np.random.default_rng(1905)
    fb = Y.frame_bytes(H, W)
    buf = rng.integers(0, 256, (5, fb), dtype=np.uint8)
    for _ in range(64):
        rgb = host_decode(Y, path, buf, 5, H, W)
        bad = luma_orders(Y, rgb)[1]                                   # [5, H, W]
        for i in (0, 2):
            for variant in VARIANTS:
                bad[i] |= luma_orders(Y, stub_bytes(rgb[i], rgb[i + 2], *variant))[1]
        if not bad.any():
            return path
        for k in range(5):
            n = int(bad[k].sum())
            buf[k, :H * W][bad[k].ravel()] = rng.integers(0, 256, n, dtype=np.uint8)
    raise AssertionError("no clip without order-sensitive triples after 64 rounds")


def both_routes(Y, dev, model, src, tmp_path, tag, **kw):
    import networks
    out = {}
    for name, extra in (("host", dict()), ("gpu", dict(gpu_io=True))):
        dst = str(tmp_path / ("%s_%s.yuv" % (tag, name)))
        scores = networks.interpolate_yuv_sequence(model, src, dst, H, W, dev, first=0, last=3, **extra, **kw)
        out[name] = (np.fromfile(dst, dtype=np.uint8), scores)
    assert out["host"][0].size == 4 * Y.frame_bytes(H, W)
    assert np.array_equal(out["gpu"][0], out["host"][0]), tag
    assert [s[0] for s in out["gpu"][1]] == [1, 3]
    return out["host"], out["gpu"]


def ssim_tolerance(h, w):
    """tests/test_gpu_ssim.py's: the mean of (h - 6)(w - 6) window values in float64, summed in another order on the device"""
    return (32 + (h - 6) * (w - 6)) * 2.0 ** -53


@pytest.mark.parametrize("pairs_per_step", [1, 2])
@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
def test_the_loop_both_ways(Y, dev, clip, tmp_path, dtype, pairs_per_step):
    seen = []

    def model(x):
        seen.append(x.dtype)
        return stub_model(x)
    host, gpu = both_routes(Y, dev, model, clip, tmp_path, "plain", dtype=dtype, pairs_per_step=pairs_per_step)
    assert gpu[1] == host[1]                                           # identical score tuples
    assert seen and all(d == dtype for d in seen)
    # the file is the restatement: frame i's bytes, then the stub's bytes in T
    rd = Y.Yuv420Reader(clip, H, W, to_rgb=True)
    rgb = [rd.read(k)[0] for k in range(5)]
    rd.close()
    wr = Y.Yuv420Writer(str(tmp_path / "want.yuv"), from_rgb=True)
    for i in (0, 2):
        wr.write(rgb[i])
        wr.write(stub_bytes(rgb[i], rgb[i + 2], dtype))
    wr.close()
    assert np.array_equal(gpu[0], np.fromfile(str(tmp_path / "want.yuv"), dtype=np.uint8))
    # with ssim=True: the same file, the same first three elements; the fourth is libmemc_hip_ssim.so's
    host_s, gpu_s = both_routes(Y, dev, model, clip, tmp_path, "ssim", dtype=dtype, pairs_per_step=pairs_per_step, ssim=True)
    assert np.array_equal(gpu_s[0], gpu[0])
    assert [t[:3] for t in gpu_s[1]] == gpu[1] and [t[:3] for t in host_s[1]] == host[1]
    for g, h_ in zip(gpu_s[1], host_s[1]):
        print("frame %d: SSIM gpu %r host %r" % (g[0], g[3], h_[3]))
        assert abs(g[3] - h_[3]) <= ssim_tolerance(H, W)
    # which = 0: the first frame comes back as its own bytes on both routes
    host0, gpu0 = both_routes(Y, dev, model, clip, tmp_path, "first", dtype=dtype, pairs_per_step=pairs_per_step, which=0)
    frames = gpu0[0].reshape(4, -1)
    assert np.array_equal(frames[0], frames[1]) and np.array_equal(frames[2], frames[3]) and gpu0[1] == host0[1]


def test_the_loop_both_ways_under_autocast(Y, dev, clip, tmp_path):
    """autocast=bfloat16 with a stub that returns float32: float32 planes in, the float32 quantiser out, on both routes"""
    seen = []

    def model(x):
        seen.append((x.dtype, torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")))
        return stub_model_float32(x)
    host, gpu = both_routes(Y, dev, model, clip, tmp_path, "autocast", autocast=torch.bfloat16)
    assert gpu[1] == host[1]
    assert seen == [(torch.float32, True, torch.bfloat16)] * 4
    plain_host, plain_gpu = both_routes(Y, dev, stub_model_float32, clip, tmp_path, "plain")
    assert np.array_equal(gpu[0], plain_gpu[0]) and gpu[1] == plain_gpu[1]


@pytest.mark.parametrize("dtype", HALVES, ids=IDS)
def test_the_quantiser_follows_the_result_s_dtype(Y, dev, clip, tmp_path, dtype):
    """a model that returns another dtype than it was fed: half in, float32 out, and float32 in, half out"""
    host, gpu = both_routes(Y, dev, stub_model_float32, clip, tmp_path, "widened", dtype=dtype)
    assert gpu[1] == host[1]

    def narrowing(x):
        frames, *rest = stub_model(x)
        return [f.to(dtype) for f in frames], None, None, None
    host, gpu = both_routes(Y, dev, narrowing, clip, tmp_path, "narrowed")
    assert gpu[1] == host[1]
