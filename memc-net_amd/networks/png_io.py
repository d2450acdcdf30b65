"""8-bit PNG files and the demo loop over a Middlebury-style tree.

The reference's still-image demo (demo_MiddleBury.py:66-181) reads `<data>/<scene>/frame10.png` and `frame11.png` with
scipy.misc.imread, interpolates the middle frame (pad to multiples of 128, crop: inference.py), writes it with
scipy.misc.imsave and scores it against `<gt>/<scene>/frame10i11.png`: mean absolute RGB error and PSNR on the 8-bit
images, plus a difference picture 128 + rec - gt cast to uint8.  Neither scipy.misc nor an image library exists here,
so the codec is restated on zlib + numpy: the PNG subset those files use -- 8 bits per sample, grey / grey+alpha /
RGB / RGBA / palette, non-interlaced, all five scanline filters on reading; the writer emits RGB or grey with the
"up" filter, which such pictures compress well under.
"""
import os
import struct
import zlib

import numpy as np

_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}          # colour type -> samples per pixel


def _chunks(buf):
    pos = len(_SIGNATURE)
    while pos + 8 <= len(buf):
        n, kind = struct.unpack(">I4s", buf[pos:pos + 8])
        body = buf[pos + 8:pos + 8 + n]
        if len(body) < n:
            raise ValueError("truncated PNG chunk %r" % kind)
        (crc,) = struct.unpack(">I", buf[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(kind + body) & 0xFFFFFFFF != crc:
            raise ValueError("bad CRC in PNG chunk %r" % kind)
        yield kind, body
        pos += 12 + n


def _unfilter(raw, h, w, bpp):
    """Undo the per-scanline filters (PNG specification, section 9): raw is h rows of 1 + w * bpp bytes."""
    stride = w * bpp
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, stride + 1)
    out = np.zeros((h + 1, stride + bpp), dtype=np.uint8)     # a zero row above, bpp zero bytes to the left
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:]
        cur, up = out[y + 1], out[y]
        if ft == 0:
            cur[bpp:] = line
        elif ft == 2:
            cur[bpp:] = line + up[bpp:]
        elif ft == 1:                                         # left neighbour: a running sum per byte lane, mod 256
            lanes = line.reshape(w, bpp).astype(np.uint32)
            cur[bpp:] = (np.cumsum(lanes, axis=0) & 0xFF).astype(np.uint8).reshape(-1)
        elif ft in (3, 4):                                    # average / Paeth depend on the byte just produced:
            c, u, ln = [0] * (stride + bpp), up.tolist(), line.tolist()     # a plain loop, on Python ints
            if ft == 3:
                for i in range(stride):
                    c[i + bpp] = (ln[i] + ((c[i] + u[i + bpp]) >> 1)) & 0xFF
            else:
                for i in range(stride):
                    a, b, d = c[i], u[i + bpp], u[i]          # left, up, upper left (u carries bpp bytes of padding)
                    p = a + b - d
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - d)
                    c[i + bpp] = (ln[i] + (a if (pa <= pb and pa <= pc) else (b if pb <= pc else d))) & 0xFF
            cur[:] = np.array(c, dtype=np.uint8)
        else:
            raise ValueError("unknown PNG filter type %d" % ft)
    return out[1:, bpp:]


def read_png(path):
    """-> uint8 array [h, w] (grey) or [h, w, c] (c = 2, 3, 4); palette images come back as RGB."""
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:8] != _SIGNATURE:
        raise ValueError("%s is not a PNG file" % path)
    header, palette, data = None, None, []
    for kind, body in _chunks(buf):
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"PLTE":
            palette = np.frombuffer(body, dtype=np.uint8).reshape(-1, 3)
        elif kind == b"IDAT":
            data.append(body)
        elif kind == b"IEND":
            break
    if header is None:
        raise ValueError("PNG without IHDR")
    w, h, depth, ctype, _comp, _filt, interlace = header
    if depth != 8 or ctype not in _CHANNELS or interlace != 0:
        raise ValueError("unsupported PNG: bit depth %d, colour type %d, interlace %d" % (depth, ctype, interlace))
    bpp = _CHANNELS[ctype]
    raw = zlib.decompress(b"".join(data))
    if len(raw) != h * (w * bpp + 1):
        raise ValueError("PNG data size does not match its header")
    img = _unfilter(raw, h, w, bpp).reshape(h, w, bpp)
    if ctype == 3:
        if palette is None:
            raise ValueError("palette PNG without PLTE")
        return palette[img[:, :, 0]]
    return img[:, :, 0].copy() if bpp == 1 else img.copy()


def write_png(path, image):
    """image: uint8 [h, w] or [h, w, 1 | 3 | 4]."""
    a = np.asarray(image)
    if a.dtype != np.uint8:
        raise ValueError("write_png takes uint8, got %s" % a.dtype)
    if a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] not in (1, 3, 4):
        raise ValueError("expected [h, w] or [h, w, 1 | 3 | 4], got %s" % (a.shape,))
    h, w, c = a.shape
    ctype = {1: 0, 3: 2, 4: 6}[c]
    flat = a.reshape(h, w * c)
    up = np.zeros_like(flat)
    up[1:] = flat[:-1]
    rows = np.empty((h, w * c + 1), dtype=np.uint8)
    rows[:, 0] = 2                                            # filter type "up"
    rows[:, 1:] = flat - up                                   # uint8 arithmetic wraps modulo 256, as the filter asks

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(_SIGNATURE)
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        f.write(chunk(b"IEND", b""))


def rgb_scores(rec_rgb, gt_rgb):
    """The still-image demo's numbers (demo_MiddleBury.py:164-172): mean |rec - gt| over all samples and PSNR; also the
    difference picture it saves (128 + rec - gt, cast to uint8 the way numpy casts: modulo 256)."""
    diff = 128.0 + np.asarray(rec_rgb, dtype=np.float64) - np.asarray(gt_rgb, dtype=np.float64)
    err = float(np.mean(np.abs(diff - 128.0)))
    mse = float(np.mean((diff - 128.0) ** 2))
    psnr = 100.0 if mse == 0 else min(100.0, float(20.0 * np.log10(255.0 / np.sqrt(mse))))    # (capped like the luma scores:
                                                                                              #  an exact match must not make the scene average inf)
    return err, psnr, (diff.astype(np.int64) & 0xFF).astype(np.uint8)


def rgb_scores_from_sums(sum_abs, sum_sq, samples):
    """rgb_scores' two numbers (err, psnr) from the integer sums of |rec - gt| and (rec - gt)^2 over a picture of `samples`
    samples (3 h w), with its cap of 100.  The same floats as rgb_scores for the same pictures: both sums are integers below
    2^53 (at most 255^2 * 3 * 32768^2 < 2^48), so numpy's float64 sums of the integer-valued samples are exact whatever their
    order, and either way one division by the sample count rounds once."""
    err = float(int(sum_abs)) / samples
    mse = float(int(sum_sq)) / samples
    psnr = 100.0 if mse == 0 else min(100.0, float(20.0 * np.log10(255.0 / np.sqrt(mse))))
    return err, psnr


def rgb_ssim(rec_rgb, gt_rgb):
    """SSIM of two 8-bit RGB pictures [h, w, 3] the way the reference's other picture demo reports it (demo_Vimeo_VE.py:168,
    compare_ssim(..., multichannel=True) at its defaults): the mean over the three channels of the SSIM of the channel
    planes (yuv_io.ssim_from_planes).  ValueError for a picture with h or w below 7."""
    from .yuv_io import ssim_from_planes
    rec, gt = np.asarray(rec_rgb), np.asarray(gt_rgb)
    if rec.ndim != 3 or rec.shape[2] != 3 or rec.shape != gt.shape:
        raise ValueError("expected two [h, w, 3] pictures of one shape, got %s and %s" % (rec.shape, gt.shape))
    return float(np.mean([ssim_from_planes(rec[:, :, c], gt[:, :, c]) for c in range(3)]))


def _usable_scenes(data_dir, first, second):
    """(scene, first frame, second frame) of every scene directory that has both files and three channels, in sorted order"""
    for scene in sorted(os.listdir(data_dir)):
        a_path, b_path = os.path.join(data_dir, scene, first), os.path.join(data_dir, scene, second)
        if not (os.path.isfile(a_path) and os.path.isfile(b_path)):
            continue
        a, b = read_png(a_path), read_png(b_path)
        if a.shape != b.shape:
            raise ValueError("%s: the two frames differ in size (%s, %s)" % (scene, a.shape, b.shape))
        if a.ndim != 3 or a.shape[2] != 3:
            continue
        yield scene, a, b


def _scene_batches(scenes, scenes_per_step):
    """consecutive scenes of one (h, w), at most scenes_per_step of them, as lists"""
    batch = []
    for item in scenes:
        if batch and item[1].shape != batch[0][1].shape:
            yield batch
            batch = []
        batch.append(item)
        if len(batch) == scenes_per_step:                  # full: it runs before the next scene's files are read
            yield batch
            batch = []
    if batch:
        yield batch


def _read_gt(gt_dir, scene, middle):
    """the scene's ground truth (RGBA cut to RGB), or None where there is none"""
    gt_path = os.path.join(gt_dir, scene, middle) if gt_dir else None
    if not (gt_path and os.path.isfile(gt_path)):
        return None
    gt = read_png(gt_path)
    if gt.ndim == 3 and gt.shape[2] == 4:
        gt = gt[:, :, :3]
    return gt


def _diff_path(out_dir, scene, middle, err):
    stem = middle[:-4] if middle.lower().endswith(".png") else middle
    return os.path.join(out_dir, scene, "%s_diff%.4f.png" % (stem, err))


def _png_batch_host(model, batch, out_dir, device, gt_dir, middle, which, dtype, autocast, ssim):
    """one batch of interpolate_png_tree with the pixel work in numpy on the host"""
    import torch
    from .inference import interpolate_pairs

    def to_tensor(imgs):
        x = np.stack([np.transpose(img, (2, 0, 1)) for img in imgs])
        return torch.from_numpy(x.astype(np.float32) / 255.0).to(device)
    mid = interpolate_pairs(model, to_tensor([a for _, a, _ in batch]), to_tensor([b for _, _, b in batch]), which,
                            dtype=dtype, autocast=autocast)
    if mid.dtype in (torch.float16, torch.bfloat16):
        mid = mid.float()                                  # numpy has no bfloat16; the widening is exact
    recs = np.round(255.0 * mid.clamp(0.0, 1.0).cpu().numpy()).astype(np.uint8)
    results = []
    for k, (scene, _a, _b) in enumerate(batch):
        rec = np.ascontiguousarray(np.transpose(recs[k], (1, 2, 0)))
        os.makedirs(os.path.join(out_dir, scene), exist_ok=True)
        write_png(os.path.join(out_dir, scene, middle), rec)
        gt = _read_gt(gt_dir, scene, middle)
        if gt is not None:
            err, psnr, diff = rgb_scores(rec, gt)
            write_png(_diff_path(out_dir, scene, middle, err), diff)
            results.append((scene, err, psnr) + ((rgb_ssim(rec, gt),) if ssim else ()))
        else:
            results.append((scene, None, None) + ((None,) if ssim else ()))
    return results


def _png_batch_gpu(model, batch, out_dir, device, gt_dir, middle, which, half, autocast, ssim):
    """one batch of interpolate_png_tree with the pixel work on the device (my_package._ext.my_lib_still, include/
    memc_still.h): the raw bytes of both frames and of the ground truth go up; decode writes straight into the padded
    network input; the quantised crop of the result is scored against the ground truth of the scenes that have one; the
    result bytes, the difference pictures and the integer sums come down.  ssim=True: one memc_ssim_u8 call on the 3 m
    channel planes of the m scored scenes (my_package._ext.my_lib_ssim); its doubles share the sums' buffer."""
    import torch
    import my_package._ext.my_lib_still as S
    from .inference import pad_amounts, run_model

    def ok(code, what):
        if code != 0:
            raise RuntimeError("%s failed its checks (return code %d)" % (what, code))

    n, (h, w, _c) = len(batch), batch[0][1].shape
    gts = [_read_gt(gt_dir, scene, middle) for scene, _a, _b in batch]
    for (scene, _a, _b), gt in zip(batch, gts):
        if gt is not None and gt.shape != (h, w, 3):
            raise ValueError("%s: the ground truth's shape %s is not the frames' %s" % (scene, gt.shape, (h, w, 3)))
    scored = [k for k in range(n) if gts[k] is not None]
    m = len(scored)
    left, right, top, bottom = pads = pad_amounts(h, w)
    raw = np.stack([a for _, a, _ in batch] + [b for _, _, b in batch] + [gts[k] for k in scored])
    raw = torch.from_numpy(np.ascontiguousarray(raw)).to(device)          # [first | second | ground truth], uint8
    x = torch.empty((2, n, 3, h + top + bottom, w + left + right), dtype=torch.float32 if half is None else half,
                    device=device)
    ok(S.rgb8_decode(raw[:n], x[0], pads), "memc_rgb8_decode")
    ok(S.rgb8_decode(raw[n:2 * n], x[1], pads), "memc_rgb8_decode")
    frames, _flows, _filters, _occlusions = run_model(model, x, autocast)
    mid = frames[which][:, :, top:top + h, left:left + w]
    out = torch.empty((n + m, h, w, 3), dtype=torch.uint8, device=device)  # [results | difference pictures]
    ok(S.rgb8_quantise(mid, out[:n]), "memc_rgb8_quantise")
    down = None
    if m:
        rec = out[:n] if m == n else out[:n].index_select(0, torch.tensor(scored, device=device))
        down = torch.empty(m * (5 if ssim else 2), dtype=torch.int64, device=device)      # [m, 2] sums | 3 m doubles
        work = torch.empty(S.rgb8_score_workspace_bytes(m, h, w), dtype=torch.uint8, device=device)
        ok(S.rgb8_score(rec, raw[2 * n:], down[:2 * m].view(m, 2), work, diff=out[n:]), "memc_rgb8_score")
        if ssim:
            import my_package._ext.my_lib_ssim as SS
            pa, pb = (t.permute(0, 3, 1, 2).contiguous().view(3 * m, h, w) for t in (rec, raw[2 * n:]))
            work = torch.empty(SS.ssim_workspace_bytes(3 * m, h, w), dtype=torch.uint8, device=device)
            ok(SS.ssim_u8(pa, pb, down[2 * m:].view(torch.float64), work), "memc_ssim_u8")
        down = down.cpu().numpy()
    out = out.cpu().numpy()
    results = []
    for k, (scene, _a, _b) in enumerate(batch):
        os.makedirs(os.path.join(out_dir, scene), exist_ok=True)
        write_png(os.path.join(out_dir, scene, middle), out[k])
        if gts[k] is None:
            results.append((scene, None, None) + ((None,) if ssim else ()))
            continue
        j = scored.index(k)
        sums = down[2 * j:2 * j + 2].view(np.uint64)
        err, psnr = rgb_scores_from_sums(sums[0], sums[1], 3 * h * w)
        write_png(_diff_path(out_dir, scene, middle, err), out[n + j])
        score = (scene, err, psnr)
        results.append(score + (float(np.mean(down[2 * m + 3 * j:2 * m + 3 * j + 3].view(np.float64))),) if ssim else score)
    return results


def interpolate_png_tree(model, data_dir, out_dir, device, gt_dir=None, first="frame10.png", second="frame11.png",
                         middle="frame10i11.png", which=1, dtype=None, autocast=None, gpu_io=False, scenes_per_step=1,
                         ssim=False):
    """For every scene directory of data_dir: first + second in, the interpolated middle frame out (out_dir/<scene>/),
    scored against gt_dir/<scene>/<middle> where that exists.  Returns [(scene, mean abs error, PSNR)] (None, None
    without ground truth).  Scenes that are not three-channel are skipped, as the reference skips them.
    dtype / autocast: interpolate_pairs' (a cast model, or torch.autocast around a float32 one), checked before a file is read;
    a half result is widened to float32 before it is rounded.
    scenes_per_step=N: consecutive usable scenes (sorted order) of one (h, w) go through the network as one batch of at most
    N; a batch ends when it holds N scenes, when the next usable scene has another size, or at the end.  Skipped scenes
    neither enter nor end a batch.  The results keep the sorted order and are those of N = 1 (every operator of the path is
    per frame pair).  N < 1: ValueError, before a file is read.
    gpu_io=True (a CUDA device; otherwise ValueError, before a file is read): the float conversion, the padding, the
    quantisation, the error sums and the difference picture run on the device (libmemc_hip_still.so, include/memc_still.h)
    instead of in numpy on the host: the same bytes and the same floats.
    ssim=True: every tuple gains a fourth element, the RGB SSIM against the ground truth (rgb_ssim; None without ground
    truth); ValueError for a picture with h or w below 7."""
    import torch
    from .inference import check_precision
    half = check_precision(dtype, autocast)
    if scenes_per_step < 1:
        raise ValueError("scenes_per_step: expected at least 1, got %r" % (scenes_per_step,))
    if gpu_io and torch.device(device).type != "cuda":
        raise ValueError("gpu_io=True needs a CUDA (HIP) device, got %s" % (device,))
    results = []
    for batch in _scene_batches(_usable_scenes(data_dir, first, second), scenes_per_step):
        if ssim and min(batch[0][1].shape[:2]) < 7:
            raise ValueError("%s: SSIM's 7 x 7 window needs h and w of at least 7, got %dx%d" % (
                batch[0][0], batch[0][1].shape[1], batch[0][1].shape[0]))
        if gpu_io:
            results += _png_batch_gpu(model, batch, out_dir, torch.device(device), gt_dir, middle, which, half, autocast, ssim)
        else:
            results += _png_batch_host(model, batch, out_dir, device, gt_dir, middle, which, dtype, autocast, ssim)
    return results
