"""The SSIM kernels of libmemc_hip_ssim.so (include/memc_ssim.h) and the demo loop's gpu_io path with ssim=True against the host
rule of networks/yuv_io.py (ssim_from_planes, luma_ssim), at the smallest shapes at which the tiling can go wrong: a tile of
ssim_tiles is 64 x 16 window centres and stages a 70 x 22 byte box.

Tolerance: (32 + N) * 2^-53 absolute, N = (h - 6)(w - 6) the number of windows.  Both sides evaluate S with about a dozen
roundings and |S| <= 1; any summation order of N terms of magnitude <= 1 moves the mean by at most N * 2^-53.  That is 5e-13
at the largest shape here, while a dropped, doubled or shifted window moves the mean by about 0.1 / N >= 1e-5.  Equal planes
must give exactly 1.0, and everything that should not matter (padding, base address, the workspace's content, the batch, a
second run) must leave the bits as they are."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# 7x7: one centre; 22x70: exactly one tile's box; 23x71: one centre past it each way; 38x134: 32 x 128 centres, exactly
# 2 x 2 full tiles; 40x136: 3 x 3 tiles, the last ones 2 centres wide and 2 high; 9x300: 3 rows of centres over five
# tiles, the last 38 wide
SHAPES = [(7, 7), (8, 10), (22, 70), (23, 71), (38, 134), (40, 136), (9, 300)]
KINDS = ["iid", "near", "checker", "equal", "corner"]


@pytest.fixture(scope="module")
def S():
    import my_package._ext.my_lib_ssim as M
    M.lib()
    return M


@pytest.fixture(scope="module")
def Y():
    import networks.yuv_io as M
    return M


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def tolerance(h, w):
    return (32 + (h - 6) * (w - 6)) * 2.0 ** -53


def make_planes(kind, seed, frames, h, w):
    """two uint8 [frames, h, w]: iid bytes; the second within +-3 of the first; a 0 / 255 checkerboard of period 7 against
    itself moved by (2 + f, 3) (whole windows of 255 in both: the largest integers); equal; equal but for one corner pixel
    (a different corner per frame), which only the corner's window sees"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (frames, h, w), dtype=np.uint8)
    if kind == "iid":
        return a, rng.integers(0, 256, (frames, h, w), dtype=np.uint8)
    if kind == "near":
        return a, np.clip(a.astype(np.int16) + rng.integers(-3, 4, (frames, h, w)), 0, 255).astype(np.uint8)
    if kind == "checker":
        ff, yy, xx = np.mgrid[0:frames, 0:h, 0:w]
        board = lambda y, x: ((((y // 7) + (x // 7)) & 1) * 255).astype(np.uint8)
        return board(yy, xx), board(yy + 2 + ff, xx + 3)
    if kind == "equal":
        return a, a.copy()
    b = a.copy()
    for f in range(frames):
        y, x = [(h - 1, w - 1), (0, 0), (0, w - 1), (h - 1, 0)][f % 4]
        b[f, y, x] ^= 0x80
    return a, b


_cases = {}


def case(Y, kind, frames, h, w):
    """the planes of a case and the host's numbers for them, computed once and shared (nothing modifies them)"""
    key = (kind, frames, h, w)
    if key not in _cases:
        a, b = make_planes(kind, 1000 * h + w + 7 * frames + KINDS.index(kind), frames, h, w)
        want = np.array([Y.ssim_from_planes(a[f], b[f]) for f in range(frames)])
        for arr in (a, b, want):
            arr.setflags(write=False)
        _cases[key] = (a, b, want)
    return _cases[key]


def run_u8(S, dev, a, b, fill=None):
    """ssim_u8 on two device tensors (any strides) -> the doubles, on the host"""
    frames, h, w = a.shape
    out = torch.full((frames,), float("nan"), dtype=torch.float64, device=dev)
    work = torch.empty(S.ssim_workspace_bytes(frames, h, w), dtype=torch.uint8, device=dev)
    if fill is not None:
        work.fill_(fill)
    assert S.ssim_u8(a, b, out, work) == 0
    return out.cpu()


def dense(dev, x):
    return torch.from_numpy(np.array(x)).to(dev)           # a copy: the shared cases are read-only


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("h,w", SHAPES)
def test_planes_against_the_host_rule(S, Y, dev, h, w, frames):
    for kind in KINDS:
        a, b, want = case(Y, kind, frames, h, w)
        got = run_u8(S, dev, dense(dev, a), dense(dev, b)).numpy()
        err = np.abs(got - want)
        print("%3d x %3d x %d %-7s gpu %s  |gpu - host| max %.3g (tolerance %.3g)" % (h, w, frames, kind, got.tolist(), err.max(),
                                                                                     tolerance(h, w)))
        assert np.all(np.isfinite(got)) and np.all(err <= tolerance(h, w)), (kind, got.tolist(), want.tolist())
        if kind == "equal":
            assert np.all(got == 1.0), got.tolist()
        else:
            assert np.all(got < 1.0), (kind, got.tolist())
        if kind == "corner":                               # one window of N moved, and was seen
            n = (h - 6) * (w - 6)
            assert np.all((1.0 - got) * n > 1e-3) and np.all((1.0 - got) * n <= 2.0), got.tolist()


@pytest.mark.parametrize("h,w", [(8, 10), (23, 71), (38, 134), (9, 300)])
def test_what_must_not_matter_leaves_the_bits(S, Y, dev, h, w):
    """Row-padded views (row stride w + 13, a gap between frames) at a base pointer one byte off, a second call, a workspace
    pre-filled with 0xFF and with 0x01, and the batch against single-frame calls: the dense call's bits."""
    frames = 3
    for kind in ("iid", "checker"):
        a, b, _want = case(Y, kind, frames, h, w)
        da, db = dense(dev, a), dense(dev, b)
        first = run_u8(S, dev, da, db)
        assert torch.equal(run_u8(S, dev, da, db), first)
        for fill in (0xFF, 0x01):
            assert torch.equal(run_u8(S, dev, da, db, fill=fill), first), fill
        sr, sf = w + 13, h * (w + 13) + 29
        views = []
        for x in (da, db):
            store = torch.full((1 + frames * sf,), 0x5A, dtype=torch.uint8, device=dev)
            v = store[1:].as_strided((frames, h, w), (sf, sr, 1))
            v.copy_(x)
            assert v.data_ptr() % 2 == 1 and v.stride() == (sf, sr, 1)
            views.append(v)
        assert torch.equal(run_u8(S, dev, views[0], views[1]), first)
        for f in range(frames):
            assert torch.equal(run_u8(S, dev, da[f:f + 1], db[f:f + 1]), first[f:f + 1]), f
            assert torch.equal(run_u8(S, dev, views[0][f:f + 1], views[1][f:f + 1]), first[f:f + 1]), f


def test_the_binding_checks_what_the_library_cannot_see(S, dev):
    a = torch.zeros((2, 8, 10), dtype=torch.uint8, device=dev)
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    work = torch.zeros(S.ssim_workspace_bytes(2, 8, 10), dtype=torch.uint8, device=dev)
    with pytest.raises(TypeError):
        S.ssim_u8(a, a.float(), out, work)
    with pytest.raises(TypeError):                         # two different row strides
        S.ssim_u8(a, torch.zeros((2, 8, 12), dtype=torch.uint8, device=dev)[:, :, :10], out, work)
    with pytest.raises(ValueError):
        S.ssim_u8(a, a[:, :7], out, work)
    with pytest.raises(ValueError):
        S.ssim_u8(a, a, out[:1], work)
    assert S.ssim_u8(a, a, out, work[:-1]) == -1           # a workspace one byte short
    assert S.ssim_u8(a[:, :6], a[:, :6], out, work) == -1  # h = 6
    assert out.cpu().tolist() == [0.0, 0.0]                # nothing was enqueued


def luma_orders(Y, rgb):
    """the truncated luma of uint8 [..., 3] under four host evaluations: (matmul's bytes, order-sensitive mask)"""
    x = rgb / 255.0
    m = Y.YUV_FROM_RGB[0]
    p0, p1, p2 = m[0] * x[..., 0], m[1] * x[..., 1], m[2] * x[..., 2]
    first = (255.0 * Y.rgb_to_yuv(x)[..., 0]).astype(np.uint8)
    sensitive = np.zeros(first.shape, dtype=bool)
    for other in ((p0 + p1) + p2, p0 + (p1 + p2), (p0 + p2) + p1):
        sensitive |= (255.0 * other).astype(np.uint8) != first
    return first, sensitive


def run_rgb(S, dev, a, b):
    frames, h, w, _ = a.shape
    out = torch.full((frames,), float("nan"), dtype=torch.float64, device=dev)
    work = torch.full((S.ssim_workspace_bytes(frames, h, w),), 0xFF, dtype=torch.uint8, device=dev)
    assert S.ssim_luma_rgb(dense(dev, a), dense(dev, b), frames, h, w, out, work) == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("h,w", [(8, 10), (34, 130)])
def test_rgb_frames_against_luma_ssim(S, Y, dev, h, w, frames):
    """iid RGB as it comes, and iid RGB whose order-sensitive triples (where the float64 luma sum truncates to another level
    under another summation order, 0.034 % of all triples) are replaced by black: on the latter tests/test_gpu_video_io.py
    already holds the device's Y to numpy's.  A luma level that differed would move the result by about 1e-7, far outside
    the tolerance: that would be a finding about the luma chain, not rounding."""
    rng = np.random.default_rng(h * 131 + w + frames)
    for label in ("insensitive", "as it comes"):
        a, b = (rng.integers(0, 256, (frames, h, w, 3), dtype=np.uint8) for _ in range(2))
        involved = int(luma_orders(Y, a)[1].sum() + luma_orders(Y, b)[1].sum())
        if label == "insensitive":
            a[luma_orders(Y, a)[1]] = 0
            b[luma_orders(Y, b)[1]] = 0
            assert not luma_orders(Y, a)[1].any() and not luma_orders(Y, b)[1].any()
        if frames == 3:
            b[1] = a[1]                                    # an identical pair among them
        want = np.array([Y.luma_ssim(a[f], b[f]) for f in range(frames)])
        got = run_rgb(S, dev, a, b)
        print("%3d x %3d x %d RGB %-12s order-sensitive pixels %d: gpu %s |gpu - host| max %.3g (tolerance %.3g)" % (
            h, w, frames, label, involved, got.tolist(), np.abs(got - want).max(), tolerance(h, w)))
        assert np.all(np.abs(got - want) <= tolerance(h, w)), (label, got.tolist(), want.tolist())
        if frames == 3:
            assert got[1] == 1.0
        assert np.array_equal(run_rgb(S, dev, a, b), got)   # a second run: the same bits


def stub_model(x):
    mid = (x[0] + x[1]) * 0.5
    return [mid, mid], None, None, None


def host_decode(Y, path, buf, frames, h, w):
    with open(path, "wb") as f:
        f.write(buf.tobytes())
    rd = Y.Yuv420Reader(path, h, w, to_rgb=True)
    try:
        return np.stack([rd.read(k)[0] for k in range(frames)])
    finally:
        rd.close()


def clean_clip(Y, path, h, w):
    """tests/test_gpu_video_io.py's clip: five frames of random bytes (the first seed) for which the host alone says that, of
    the two scored frames, one involves no order-sensitive byte and the other does.  Returns, per scored frame, the result
    and the real frame (RGB bytes of the host path) and the number of sensitive pixels involved."""
    fb = Y.frame_bytes(h, w)
    for seed in range(400):
        buf = np.random.default_rng(seed).integers(0, 256, 5 * fb, dtype=np.uint8)
        rgb = host_decode(Y, path, buf, 5, h, w)
        planes = rgb.astype(np.float32) / np.float32(255.0)
        pairs, involved = [], []
        for i in (0, 2):
            rec = np.round(np.float32(255.0) * np.clip((planes[i] + planes[i + 2]) * np.float32(0.5), 0.0, 1.0)).astype(np.uint8)
            pairs.append((rec, rgb[i + 1]))
            involved.append(int(luma_orders(Y, rec)[1].sum() + luma_orders(Y, rgb[i + 1])[1].sum()))
        if min(involved) == 0 and max(involved) > 0:
            return pairs, involved
    raise AssertionError("no seed below 400 gives such a clip")


def test_the_loop_with_the_third_score(S, Y, dev, tmp_path):
    """The model and clip of tests/test_gpu_video_io.py::test_the_loop_both_ways: with ssim=True the first three elements and
    the written file are those of ssim=False; the fourth is luma_ssim of the host path's frames within the tolerance where
    no order-sensitive pixel is involved (there that test finds the two paths' frames byte-equal), and equals the host
    loop's own fourth element there."""
    import networks
    h, w = 34, 130
    src = str(tmp_path / "in.yuv")
    pairs, involved = clean_clip(Y, src, h, w)
    outs, scores = {}, {}
    for name, kw in (("off", dict(gpu_io=True)), ("on", dict(gpu_io=True, ssim=True)),
                     ("on2", dict(gpu_io=True, ssim=True, pairs_per_step=2)), ("host", dict(ssim=True))):
        dst = str(tmp_path / (name + ".yuv"))
        scores[name] = networks.interpolate_yuv_sequence(stub_model, src, dst, h, w, dev, **kw)
        outs[name] = np.fromfile(dst, dtype=np.uint8)
    assert all(len(t) == 3 for t in scores["off"]) and all(len(t) == 4 for t in scores["on"])
    assert [t[:3] for t in scores["on"]] == scores["off"] and scores["on2"] == scores["on"]
    assert np.array_equal(outs["on"], outs["off"]) and np.array_equal(outs["on2"], outs["off"])
    assert [t[0] for t in scores["on"]] == [t[0] for t in scores["host"]] == [1, 3]
    checked = 0
    for got, host, (rec, gt), n in zip(scores["on"], scores["host"], pairs, involved):
        want = Y.luma_ssim(rec, gt)
        print("frame %d: gpu %r host %r luma_ssim %r, order-sensitive pixels involved: %d" % (got[0], got[3], host[3], want, n))
        assert host[3] == want
        if n == 0:
            assert abs(got[3] - want) <= tolerance(h, w)
            checked += 1
    assert checked == 1
