"""The video-enhancement demo loop over a Vimeo-90K septuplet tree.

The reference's third demo (demo_Vimeo_VE.py:100-182) reads `<input>/<sequence>/<clip>/im1.png .. im7.png` -- the degraded
(noisy, blocky or down-sampled) septuplet -- replicate-pads every frame (to multiples of 128, by 32 + 32 on a side that
already is one: inference.pad_amounts, so 256 x 448 becomes 320 x 512), runs MEMC_Net_VE, crops the enhanced centre frame,
writes it as `<out>/<sequence>/<clip>/im4.png` (clip to [0, 1], x 255, round) and scores it against
`<target>/<sequence>/<clip>/im4.png`: mean absolute RGB error, PSNR and SSIM on the 8-bit pictures, per clip and averaged
into `<out>/metrics.txt`.  The clips are those a list file names (`sep_testlist.txt`: one `<sequence>/<clip>` per line), or
every directory of the tree that holds the seven files.  PNG files are read and written by png_io.py.
"""
import os

import numpy as np

from .png_io import read_png, rgb_scores, rgb_scores_from_sums, rgb_ssim, write_png

FRAMES = tuple("im%d.png" % k for k in range(1, 8))
CENTRE = "im4.png"


def list_clips(input_dir, list_file=None):
    """`<sequence>/<clip>` of every clip: the non-empty lines of list_file, in its order, or else every two-level directory
    of input_dir that holds im1.png .. im7.png, sorted"""
    if list_file:
        with open(list_file) as f:
            return [line.strip().strip("/") for line in f if line.strip()]
    clips = []
    for seq in sorted(os.listdir(input_dir)):
        if not os.path.isdir(os.path.join(input_dir, seq)):
            continue
        for clip in sorted(os.listdir(os.path.join(input_dir, seq))):
            if all(os.path.isfile(os.path.join(input_dir, seq, clip, name)) for name in FRAMES):
                clips.append(seq + "/" + clip)
    return clips


def metrics_text(results, ssim=False):
    """the line the reference writes to metrics.txt (demo_Vimeo_VE.py:175-176), over the clips' averages; without SSIM the
    line ends after the PSNR"""
    mean = lambda k: round(sum(r[k] for r in results) / len(results), 4)      # noqa: E731
    text = "The average interpolation error / PSNR for all images are : " + str(mean(1)) + ",\t  psnr " + str(mean(2))
    return text + (",\t  ssim " + str(mean(3)) if ssim else "")


def _read_septuplet(input_dir, target_dir, clip):
    frames = [read_png(os.path.join(input_dir, clip, name)) for name in FRAMES]
    gt = read_png(os.path.join(target_dir, clip, CENTRE))
    if gt.ndim == 3 and gt.shape[2] == 4:
        gt = gt[:, :, :3]
    for name, img in zip(FRAMES + ("the target " + CENTRE,), frames + [gt]):
        if img.ndim != 3 or img.shape[2] != 3 or img.shape != frames[0].shape:
            raise ValueError("%s: %s is %s, expected three channels of the size of %s, %s" % (
                clip, name, img.shape, FRAMES[0], frames[0].shape))
    return frames, gt


def _enhance_host(model, frames, device, half=None, autocast=None):
    """the enhanced centre frame as uint8 [h, w, 3], the pixel work in numpy and torch on the host's side of the model; `half`:
    the frames are cast to it and padded in it (a cast model); a half result is widened before it is rounded (exact)"""
    import torch
    import torch.nn.functional as F
    from .inference import pad_amounts, run_model
    h, w, _c = frames[0].shape
    left, right, top, bottom = pad_amounts(h, w)
    xs = [torch.from_numpy(np.transpose(img, (2, 0, 1))[None].astype(np.float32) / 255.0).to(device) for img in frames]
    if half is not None:
        xs = [x.to(half) for x in xs]
    xs = [F.pad(x, (left, right, top, bottom), mode="replicate") for x in xs]
    y = run_model(model, xs, autocast)
    y = (y[0] if isinstance(y, (tuple, list)) else y)[0, :, top:top + h, left:left + w]
    return np.ascontiguousarray(np.transpose(np.round(255.0 * y.float().clamp(0.0, 1.0).cpu().numpy()), (1, 2, 0)).astype(np.uint8))


def _enhance_gpu(model, frames, gt, device, ssim, half=None, autocast=None):
    """the same with the pixel work on the device (my_package._ext.my_lib_still, include/memc_still.h): the raw bytes of the
    seven frames and the target go up, decode writes the padded network inputs, the quantised crop of the result is scored;
    the result's bytes and the integer sums (and the three channels' SSIM) come down.  `half`: decode writes the planes in
    that storage (a cast model); quantise takes the result in whatever dtype the model returns.  -> (uint8 [h, w, 3], scores)"""
    import torch
    import my_package._ext.my_lib_still as S
    from .inference import pad_amounts, run_model

    def ok(code, what):
        if code != 0:
            raise RuntimeError("%s failed its checks (return code %d)" % (what, code))

    h, w, _c = frames[0].shape
    left, right, top, bottom = pads = pad_amounts(h, w)
    raw = torch.from_numpy(np.ascontiguousarray(np.stack(frames + [gt]))).to(device)      # [seven frames | target], uint8
    x = torch.empty((7, 3, h + top + bottom, w + left + right), dtype=torch.float32 if half is None else half, device=device)
    ok(S.rgb8_decode(raw[:7], x, pads), "memc_rgb8_decode")
    y = run_model(model, [x[k:k + 1] for k in range(7)], autocast)
    y = (y[0] if isinstance(y, (tuple, list)) else y)[:, :, top:top + h, left:left + w]
    rec = torch.empty((1, h, w, 3), dtype=torch.uint8, device=device)
    ok(S.rgb8_quantise(y, rec), "memc_rgb8_quantise")
    down = torch.empty(5 if ssim else 2, dtype=torch.int64, device=device)                # [1, 2] sums | 3 doubles
    work = torch.empty(S.rgb8_score_workspace_bytes(1, h, w), dtype=torch.uint8, device=device)
    ok(S.rgb8_score(rec, raw[7:], down[:2].view(1, 2), work), "memc_rgb8_score")
    if ssim:
        import my_package._ext.my_lib_ssim as SS
        pa, pb = (t.permute(0, 3, 1, 2).contiguous().view(3, h, w) for t in (rec, raw[7:]))
        work = torch.empty(SS.ssim_workspace_bytes(3, h, w), dtype=torch.uint8, device=device)
        ok(SS.ssim_u8(pa, pb, down[2:].view(torch.float64), work), "memc_ssim_u8")
    down = down.cpu().numpy()
    sums = down[:2].view(np.uint64)
    scores = rgb_scores_from_sums(sums[0], sums[1], 3 * h * w)
    return rec[0].cpu().numpy(), scores + ((float(np.mean(down[2:].view(np.float64))),) if ssim else ())


def enhance_septuplet_tree(model, input_dir, target_dir, out_dir, device, list_file=None, gpu_io=False, ssim=False,
                           dtype=None, autocast=None):
    """For every clip (list_clips): im1.png .. im7.png of input_dir in, the enhanced centre frame out
    (out_dir/<sequence>/<clip>/im4.png), scored against target_dir/<sequence>/<clip>/im4.png; the averages go to
    out_dir/metrics.txt (metrics_text).  `model`: seven [1, 3, H, W] frames -> the enhanced centre (MEMC_Net_VE at inference;
    of a tuple, the first element).  Returns [(clip, mean abs error, PSNR)], with the RGB SSIM (rgb_ssim) as a fourth element
    under ssim=True (ValueError for a picture with h or w below 7).
    gpu_io=True (a CUDA device; otherwise ValueError, before a file is read): the float conversion, the padding, the
    quantisation, the error sums and the SSIM run on the device (libmemc_hip_still.so, libmemc_hip_ssim.so) instead of in
    numpy on the host: the same bytes and the same floats.
    dtype / autocast: interpolate_png_tree's (inference.check_precision: a model cast to float16 / bfloat16 is fed planes of
    `dtype`, or a float32 model runs inside torch.autocast on float32 planes), checked before a file is read; a half result
    is widened to float32 before it is rounded."""
    import torch
    from .inference import check_precision
    half = check_precision(dtype, autocast)
    if gpu_io and torch.device(device).type != "cuda":
        raise ValueError("gpu_io=True needs a CUDA (HIP) device, got %s" % (device,))
    results = []
    for clip in list_clips(input_dir, list_file):
        frames, gt = _read_septuplet(input_dir, target_dir, clip)
        if ssim and min(gt.shape[:2]) < 7:
            raise ValueError("%s: SSIM's 7 x 7 window needs h and w of at least 7, got %dx%d" % (clip, gt.shape[1], gt.shape[0]))
        if gpu_io:
            rec, scores = _enhance_gpu(model, frames, gt, torch.device(device), ssim, half, autocast)
        else:
            rec = _enhance_host(model, frames, device, half, autocast)
            scores = rgb_scores(rec, gt)[:2] + ((rgb_ssim(rec, gt),) if ssim else ())
        os.makedirs(os.path.join(out_dir, clip), exist_ok=True)
        write_png(os.path.join(out_dir, clip, CENTRE), rec)
        results.append((clip,) + tuple(scores))
    if results:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "metrics.txt"), "w") as f:
            f.write(metrics_text(results, ssim) + "\n")
    return results
