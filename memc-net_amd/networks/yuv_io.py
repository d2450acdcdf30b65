"""Planar YUV 4:2:0 frame files and the demo loop around a frame pair.

What the reference's HD demo does around the network (yuv_frame_io.py:31-200, demo_HD720p.py:60-170), restated on
numpy alone -- the reference needs scipy.misc.imresize and skimage.color for it, neither of which exists here:

  * a frame of an I420 file is h*w bytes of Y, then (h/2)*(w/2) of U, then of V (yuv_frame_io.py:38-41,50-52);
  * reading: chroma is upsampled by pixel repetition (imresize(..., interp='nearest') of an exact factor two picks
    source index i // 2), Y/255, U/255 - 0.5, V/255 - 0.5 go through the inverse of the analog-YUV matrix that
    skimage calls yuv2rgb, clipped to [0, 1], times 255, truncated to uint8 (:65-66,85-89);
  * writing: RGB/255 through the forward matrix, U + 0.5 and V + 0.5 clipped to [0, 1], every second chroma sample of
    every second row kept, times 255, truncated to uint8 (:129-148);
  * the demo reads frames i and i + 2, interpolates the middle one (pad to multiples of 128, crop: inference.py),
    writes frame i and the rounded result, and scores the result against the real frame i + 1 on the truncated luma
    planes: mean absolute error, PSNR (demo_HD720p.py:75-167) and, on request, SSIM (:150-190 calls skimage's
    compare_ssim at its defaults; luma_ssim restates that rule on integer window sums, in numpy alone).

interpolate_yuv_sequence(..., gpu_io=True) runs the same rule on the device (libmemc_hip_video.so, include/memc_video.h):
only raw I420 bytes cross the bus (with ssim=True the third score comes from libmemc_hip_ssim.so, include/memc_ssim.h).
Off by default; the numpy path is the definition the kernels are tested against.
dtype= / autocast= run the network in float16 / bfloat16 (a cast model, or torch.autocast around a float32 one) on either route;
with gpu_io=True a cast model's input is decoded by libmemc_hip_video_lp.so (include/memc_video_lp.h).  Off by default as well.
"""
import numpy as np

# skimage.color's yuv_from_rgb (the analog YUV of PAL: Y = 0.299 R + 0.587 G + 0.114 B, U = 0.492 (B - Y), V = 0.877 (R - Y))
YUV_FROM_RGB = np.array([[0.299, 0.587, 0.114],
                         [-0.14714119, -0.28886916, 0.43601035],
                         [0.61497538, -0.51496512, -0.10001026]], dtype=np.float64)
RGB_FROM_YUV = np.linalg.inv(YUV_FROM_RGB)


def rgb_to_yuv(rgb):
    """[..., 3] float RGB in [0, 1] -> analog YUV (what skimage.color.rgb2yuv computes)."""
    return np.asarray(rgb, dtype=np.float64) @ YUV_FROM_RGB.T


def yuv_to_rgb(yuv):
    return np.asarray(yuv, dtype=np.float64) @ RGB_FROM_YUV.T


def frame_bytes(h, w):
    return h * w + 2 * ((h // 2) * (w // 2))


class Yuv420Reader(object):
    """reader.read(k) -> (frame, True) or (None, False) past the end; frame is uint8 RGB [h, w, 3] (to_rgb) or the
    uint8 Y, U, V planes stacked at full resolution."""

    def __init__(self, path, h, w, to_rgb=True):
        if h % 2 or w % 2:
            raise ValueError("4:2:0 needs even dimensions, got %dx%d" % (w, h))
        self.h, self.w, self.to_rgb = h, w, to_rgb
        self.frame_length = frame_bytes(h, w)
        self.fp = open(path, "rb")

    def read(self, frame_index=None):
        h, w = self.h, self.w
        if frame_index is not None:
            self.fp.seek(frame_index * self.frame_length, 0)
        buf = self.fp.read(self.frame_length)
        if len(buf) < self.frame_length:
            return None, False
        a = np.frombuffer(buf, dtype=np.uint8)
        ny, nc = h * w, (h // 2) * (w // 2)
        y = a[:ny].reshape(h, w)
        u = a[ny:ny + nc].reshape(h // 2, w // 2).repeat(2, axis=0).repeat(2, axis=1)
        v = a[ny + nc:].reshape(h // 2, w // 2).repeat(2, axis=0).repeat(2, axis=1)
        if not self.to_rgb:
            return np.stack((y, u, v), axis=-1), True
        yuv = np.stack((y / 255.0, u / 255.0 - 0.5, v / 255.0 - 0.5), axis=-1)
        return (255.0 * np.clip(yuv_to_rgb(yuv), 0.0, 1.0)).astype(np.uint8), True

    def close(self):
        self.fp.close()


class Yuv420Writer(object):
    """writer.write(frame): uint8 RGB [h, w, 3] (from_rgb) or full-resolution Y, U, V planes stacked."""

    def __init__(self, path, from_rgb=True):
        self.fp = open(path, "wb")
        self.from_rgb = from_rgb

    def write(self, frame):
        frame = np.asarray(frame)
        if frame.ndim != 3 or frame.shape[2] != 3 or frame.shape[0] % 2 or frame.shape[1] % 2:
            raise ValueError("expected [h, w, 3] with even h and w, got %s" % (frame.shape,))
        if self.from_rgb:
            yuv = rgb_to_yuv(frame / 255.0)
            y = (255.0 * yuv[:, :, 0]).astype(np.uint8)
            u = (255.0 * np.clip(yuv[::2, ::2, 1] + 0.5, 0.0, 1.0)).astype(np.uint8)
            v = (255.0 * np.clip(yuv[::2, ::2, 2] + 0.5, 0.0, 1.0)).astype(np.uint8)
        else:
            y, u, v = frame[:, :, 0], frame[::2, ::2, 1], frame[::2, ::2, 2]
        for plane in (y, u, v):
            self.fp.write(np.ascontiguousarray(plane).tobytes())
        return True

    def close(self):
        self.fp.close()


def luma_scores(rec_rgb, gt_rgb):
    """The demo's two numbers for one interpolated frame: mean |dY| and PSNR on the truncated 8-bit luma planes
    (demo_HD720p.py:150-167; PSNR 100 for identical planes)."""
    gy = (rgb_to_yuv(gt_rgb / 255.0)[:, :, 0] * 255.0).astype(np.uint8).astype(np.float64)
    ry = (rgb_to_yuv(rec_rgb / 255.0)[:, :, 0] * 255.0).astype(np.uint8).astype(np.float64)
    diff = ry - gy
    mse = float(np.mean(diff ** 2))
    psnr = 100.0 if mse == 0 else float(20.0 * np.log10(255.0 / np.sqrt(mse)))
    return float(np.mean(np.abs(diff))), psnr


# skimage's compare_ssim at its defaults on 8-bit planes: 7 x 7 uniform window (49 samples), sample covariance,
# K1 = 0.01, K2 = 0.03, data range 255; numerator and denominator of its map scaled by 49^2 and 49 * 48 (memc_ssim.h)
SSIM_C1 = (0.01 * 255) ** 2 * 49 ** 2
SSIM_C2 = (0.03 * 255) ** 2 * 49 * 48


def _box7(p):
    """int64 [h, w] -> the sums over every 7 x 7 window that lies inside, [h - 6, w - 6], by 2-D cumulative sums"""
    c = np.zeros((p.shape[0] + 1, p.shape[1] + 1), dtype=np.int64)
    c[1:, 1:] = p.cumsum(axis=0).cumsum(axis=1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def ssim_from_planes(a, b):
    """SSIM of two uint8 planes [h, w] as skimage's compare_ssim computes it at its defaults: the mean of the SSIM map over
    the (h - 6)(w - 6) windows that lie inside the plane.  On bytes the five window sums are exact integers; per window
        S = ((2 sx sy + c1) (2 Vxy + c2)) / ((sx^2 + sy^2 + c1) (Vxx + Vyy + c2)),  V.. = 49 s.. - s. s.
    in float64 from the integers (no cancellation: equal planes give exactly 1.0)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.ndim != 2 or a.shape != b.shape:
        raise ValueError("expected two uint8 planes of one shape, got %s %s and %s %s" % (a.dtype, a.shape, b.dtype, b.shape))
    if min(a.shape) < 7:
        raise ValueError("SSIM's 7 x 7 window needs h and w of at least 7, got %dx%d" % (a.shape[1], a.shape[0]))
    x, y = a.astype(np.int64), b.astype(np.int64)
    sx, sy, sxx, syy, sxy = _box7(x), _box7(y), _box7(x * x), _box7(y * y), _box7(x * y)
    vxx, vyy, vxy = 49 * sxx - sx * sx, 49 * syy - sy * sy, 49 * sxy - sx * sy
    s = ((2 * sx * sy + SSIM_C1) * (2 * vxy + SSIM_C2)) / ((sx * sx + sy * sy + SSIM_C1) * (vxx + vyy + SSIM_C2))
    return float(np.mean(s))


def luma_ssim(rec_rgb, gt_rgb):
    """The demo's third number for one interpolated frame: SSIM of the truncated 8-bit luma planes, luma_scores' planes."""
    gy = (rgb_to_yuv(gt_rgb / 255.0)[:, :, 0] * 255.0).astype(np.uint8)
    ry = (rgb_to_yuv(rec_rgb / 255.0)[:, :, 0] * 255.0).astype(np.uint8)
    return ssim_from_planes(ry, gy)


def scores_from_sums(sum_abs, sum_sq, pixels):
    """luma_scores' two numbers from the integer sums of |dY| and dY^2 over a plane of `pixels` samples, in float64."""
    mse = float(int(sum_sq)) / pixels
    psnr = 100.0 if mse == 0 else float(20.0 * np.log10(255.0 / np.sqrt(mse)))
    return float(int(sum_abs)) / pixels, psnr


def _interpolate_yuv_sequence_gpu(model, in_path, out_path, h, w, device, first, last, pairs_per_step, which, ssim=False,
                                  half=None, autocast=None):
    """interpolate_yuv_sequence with the frame I/O on the device (my_package._ext.my_lib_video, include/memc_video.h): per
    step the raw bytes of frames i, i + 2 and i + 1 of every pair go up, two I420 frames per pair and the integer score
    sums come down.  Decode writes straight into the padded network input; frame i is encoded from its decoded RGB bytes
    (what Yuv420Writer does with the reader's frame), the result from the quantised crop of the network's output.
    ssim=True: one memc_ssim_luma_rgb call per step on the result and the real frame, both on the device already; its
    doubles share the integer sums' buffer and come down with them.
    half (torch.float16 / torch.bfloat16): the network's input is allocated in that dtype and decoded into by
    my_package._ext.my_lib_video_lp (include/memc_video_lp.h).  The quantiser follows the dtype of what the model returns:
    float32 (an autocast run, for one) goes to my_lib_video, a half result to my_lib_video_lp."""
    import torch
    import my_package._ext.my_lib_video as V
    import my_package._ext.my_lib_video_lp as VL            # loads its library on first use: never in a float32 run
    if ssim:
        import my_package._ext.my_lib_ssim as S
    from .inference import pad_amounts, run_model
    if h % 2 or w % 2:
        raise ValueError("4:2:0 needs even dimensions, got %dx%d" % (w, h))
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("gpu_io=True needs a CUDA (HIP) device, got %s" % (device,))

    def ok(code, what):
        if code != 0:
            raise RuntimeError("%s failed its checks (return code %d)" % (what, code))

    fb = frame_bytes(h, w)
    left, right, top, bottom = pads = pad_amounts(h, w)
    hp, wp = h + top + bottom, w + left + right
    scores = []
    with open(in_path, "rb") as fin, open(out_path, "wb") as fout:
        def read(k):
            fin.seek(k * fb, 0)
            buf = fin.read(fb)
            return buf if len(buf) == fb else None
        index = first
        while index < last:
            batch = []
            while len(batch) < pairs_per_step and index < last:
                a, b = read(index), read(index + 2)
                if a is None or b is None:
                    index = last
                    break
                batch.append((index, a, b, read(index + 1)))        # frame i + 1 lies before frame i + 2: it is there
                index += 2
            if not batch:
                break
            n = len(batch)
            # [frames i | frames i + 2 | frames i + 1], n of each
            raw = np.frombuffer(b"".join(t[j] for j in (1, 2, 3) for t in batch), dtype=np.uint8)
            raw = torch.from_numpy(raw.copy()).to(device).view(3, n, fb)
            x = torch.empty((2, n, 3, hp, wp), dtype=torch.float32 if half is None else half, device=device)
            D = V if half is None else VL
            rgb_a, rgb_gt, rec = (torch.empty((n, h, w, 3), dtype=torch.uint8, device=device) for _ in range(3))
            ok(D.i420_decode(raw[0], n, h, w, rgb=rgb_a, planes=x[0], pads=pads), "memc_i420_decode")
            ok(D.i420_decode(raw[1], n, h, w, planes=x[1], pads=pads), "memc_i420_decode")
            ok(V.i420_decode(raw[2], n, h, w, rgb=rgb_gt), "memc_i420_decode")
            frames, _flows, _filters, _occlusions = run_model(model, x, autocast)
            mid = frames[which][:, :, top:top + h, left:left + w]
            Q = VL if mid.dtype in (torch.float16, torch.bfloat16) else V
            ok(Q.rgb_quantise(mid, rec), "memc_rgb_quantise")
            out = torch.empty((n, 2, fb), dtype=torch.uint8, device=device)
            for k in range(n):                                      # the file's order: frame i, then the result
                ok(V.i420_encode(rgb_a[k], 1, h, w, out[k, 0]), "memc_i420_encode")
                ok(V.i420_encode(rec[k], 1, h, w, out[k, 1]), "memc_i420_encode")
            down = torch.empty(n * (3 if ssim else 2), dtype=torch.int64, device=device)   # [n, 2] sums | n doubles
            sums = down[:2 * n].view(n, 2)
            work = torch.empty(V.luma_score_workspace_bytes(n, h, w), dtype=torch.uint8, device=device)
            ok(V.luma_score(rec, rgb_gt, n, h, w, sums, work), "memc_luma_score")
            if ssim:
                work = torch.empty(S.ssim_workspace_bytes(n, h, w), dtype=torch.uint8, device=device)
                ok(S.ssim_luma_rgb(rec, rgb_gt, n, h, w, down[2 * n:].view(torch.float64), work), "memc_ssim_luma_rgb")
            fout.write(out.cpu().numpy().tobytes())
            down = down.cpu().numpy()
            sums = down[:2 * n].reshape(n, 2).view(np.uint64)
            for k, t in enumerate(batch):
                score = (t[0] + 1,) + scores_from_sums(sums[k, 0], sums[k, 1], h * w)
                scores.append(score + (float(down[2 * n + k:2 * n + k + 1].view(np.float64)[0]),) if ssim else score)
    return scores


def interpolate_yuv_sequence(model, in_path, out_path, h, w, device, first=0, last=100, pairs_per_step=1, which=1,
                             gpu_io=False, ssim=False, dtype=None, autocast=None):
    """The demo loop: for i = first, first + 2, ...: frames i and i + 2 in, the interpolated frame i + 1 out
    (out_path receives frame i, then the interpolated frame), scored against the file's own frame i + 1.
    pairs_per_step > 1 batches that many independent pairs through the network at once (same results: every operator
    of the path is per frame pair).  Returns the list of (index of the interpolated frame, mean |dY|, PSNR); with
    ssim=True every tuple gains a fourth element, the SSIM of the two luma planes (luma_ssim).
    gpu_io=True (a CUDA device) decodes, quantises, encodes and scores on the device instead of in numpy on the host:
    the same bytes, but for Y samples whose float64 sum depends on its order (one level at 0.034 % of the RGB triples).
    dtype=torch.float16 / torch.bfloat16: the planes handed to the model are (float32(byte) / 255).to(dtype), padded in that
    dtype (the caller has cast the model: model.to(dtype)); autocast=torch.float16 / torch.bfloat16: the model runs inside
    torch.autocast on float32 planes.  The two exclude each other (ValueError; any other dtype: TypeError -- both before a
    file is opened).  The result is widened to float32 before it is quantised, on either route."""
    from .inference import check_precision, interpolate_pairs
    half = check_precision(dtype, autocast)
    if gpu_io:
        return _interpolate_yuv_sequence_gpu(model, in_path, out_path, h, w, device, first, last, pairs_per_step, which,
                                             ssim, half, autocast)
    import torch
    reader, writer = Yuv420Reader(in_path, h, w, to_rgb=True), Yuv420Writer(out_path, from_rgb=True)
    scores = []
    try:
        index = first
        while index < last:
            batch = []
            while len(batch) < pairs_per_step and index < last:
                a, ok_a = reader.read(index)
                b, ok_b = reader.read(index + 2)
                if not (ok_a and ok_b):
                    index = last
                    break
                batch.append((index, a, b))
                index += 2
            if not batch:
                break

            def to_tensor(frames):
                x = np.stack([np.transpose(f, (2, 0, 1)) for f in frames]).astype(np.float32) / 255.0
                x = torch.from_numpy(x).to(device)
                return x if half is None else x.to(half)
            mid = interpolate_pairs(model, to_tensor([a for _, a, _ in batch]), to_tensor([b for _, _, b in batch]), which,
                                    dtype=half, autocast=autocast)
            if mid.dtype in (torch.float16, torch.bfloat16):
                mid = mid.float()                          # numpy has no bfloat16; the widening is exact
            mid = np.round(255.0 * mid.clamp(0.0, 1.0).cpu().numpy()).astype(np.uint8)
            for k, (i, a, _b) in enumerate(batch):
                rec = np.transpose(mid[k], (1, 2, 0))
                writer.write(a)
                writer.write(rec)
                gt, ok = reader.read(i + 1)
                if ok:
                    scores.append((i + 1,) + luma_scores(rec, gt) + ((luma_ssim(rec, gt),) if ssim else ()))
    finally:
        reader.close()
        writer.close()
    return scores
