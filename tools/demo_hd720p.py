#!/usr/bin/env python
"""tools/demo_hd720p.py -- the reference's HD demo (demo_HD720p.py) on this repository's operators: interpolate the odd
frames of a planar YUV 4:2:0 file from its even ones and score them against the file's own odd frames.

    python tools/demo_hd720p.py --input clip_1280x720.yuv --output clip_interp.yuv [--height 720 --width 1280]
                                [--model MEMC_Net_star --weights best.pth --align-corners] [--first 0 --last 100]
                                [--pairs-per-step 4] [--gpu-io] [--ssim]
                                [--precision {fp32,bf16,fp16,autocast-bf16,autocast-fp16}]

Frames i and i + 2 go in (replicate-padded to multiples of 128 like demo_HD720p.py:88-113), the output file receives
frame i and the interpolated frame i + 1 (demo_HD720p.py:146-149); printed per frame: mean |dY| and PSNR on the 8-bit
luma planes (:150-167).  --ssim adds the SSIM of the two luma planes (:150-190: skimage's compare_ssim at its defaults) and
writes <output>_psnr_Y.txt and <output>_ssim_Y.txt, one value per line.  Without --weights the network runs on its random
initialisation (plumbing check only).  --precision runs the network in reduced precision: a cast model (bf16, fp16; with
--gpu-io the planes are decoded and quantised by libmemc_hip_video_lp.so) or a float32 model under torch.autocast.
Needs a GPU: the operators have no CPU path.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--input", required=True)
    ap.add_argument("--output", required=True)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--model", default="MEMC_Net_star", choices=["MEMC_Net_star", "MEMC_Net"])
    ap.add_argument("--weights", default="")
    ap.add_argument("--align-corners", action="store_true",
                    help="bilinear upsampling as PyTorch 0.2 did it: what the published checkpoints were trained with")
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--last", type=int, default=100)
    ap.add_argument("--pairs-per-step", type=int, default=1)
    ap.add_argument("--save-which", type=int, default=1, choices=[0, 1], help="0: blended, 1: rectified (the demos' save_which)")
    ap.add_argument("--gpu-io", action="store_true",
                    help="decode, quantise, encode and score on the GPU (libmemc_hip_video.so) instead of in numpy on the host")
    ap.add_argument("--ssim", action="store_true",
                    help="also score SSIM on the luma planes (with --gpu-io: libmemc_hip_ssim.so) and write <output>_psnr_Y.txt "
                         "and <output>_ssim_Y.txt")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "fp16", "autocast-bf16", "autocast-fp16"],
                    help="fp32 (default): as ever.  bf16 / fp16: the model is cast after its weights are loaded and fed planes of "
                         "that dtype -- bf16 is the cast mode to prefer, an fp16 cast can overflow in the dense layers.  "
                         "autocast-bf16 / autocast-fp16: the float32 model runs inside torch.autocast on float32 planes")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the HIP operators have no CPU fallback")
    import networks
    dev = torch.device("cuda", 0)
    net = getattr(networks, a.model)(channel=3, filter_size=4, training=False, align_corners=a.align_corners)
    if a.weights:
        state = torch.load(a.weights, map_location="cpu")
        net.load_state_dict(state.get("state_dict", state), strict=True)
    net = net.to(dev).eval()
    half = {"bf16": torch.bfloat16, "fp16": torch.float16}
    dtype = half.get(a.precision)
    autocast = half.get(a.precision[len("autocast-"):]) if a.precision.startswith("autocast-") else None
    if dtype is not None:
        net = net.to(dtype)
    scores = networks.interpolate_yuv_sequence(net, a.input, a.output, a.height, a.width, dev, first=a.first, last=a.last,
                                               pairs_per_step=a.pairs_per_step, which=a.save_which, gpu_io=a.gpu_io,
                                               **(dict(ssim=True) if a.ssim else {}),
                                               **(dict(dtype=dtype, autocast=autocast) if a.precision != "fp32" else {}))
    for s in scores:
        print("frame %4d  mean|dY| %.4f  PSNR %.3f dB" % s[:3] + ("  SSIM %.6f" % s[3] if a.ssim else ""))
    if scores:
        print("average over %d interpolated frames: mean|dY| %.4f  PSNR %.3f dB" % (
            len(scores), sum(s[1] for s in scores) / len(scores), sum(s[2] for s in scores) / len(scores))
            + ("  SSIM %.6f" % (sum(s[3] for s in scores) / len(scores)) if a.ssim else ""))
    if a.ssim:
        for suffix, column in (("_psnr_Y.txt", 2), ("_ssim_Y.txt", 3)):
            with open(a.output + suffix, "w") as f:
                f.write("".join("%r\n" % s[column] for s in scores))


if __name__ == "__main__":
    main()
