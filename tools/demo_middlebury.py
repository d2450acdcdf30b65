#!/usr/bin/env python
"""tools/demo_middlebury.py -- the reference's still-image demo (demo_MiddleBury.py) on this repository's operators: for every
scene directory, interpolate the frame between frame10.png and frame11.png and score it against the ground truth.

    python tools/demo_middlebury.py --data other-data --gt other-gt-interp --output results
                                    [--model {MEMC_Net_star,MEMC_Net,MEMC_Net_s} --weights best.pth --align-corners] [--save-which 1]
                                    [--precision {fp32,bf16,fp16,autocast-bf16,autocast-fp16}]
                                    [--gpu-io] [--scenes-per-step N] [--ssim] [--fused-half-level]
                                    [--first im1.png --second im3.png --middle im2.png]

Each pair is replicate-padded to multiples of 128 like demo_MiddleBury.py:98-117 and cropped back; results/<scene>/ receives
frame10i11.png and, where ground truth exists, the difference picture 128 + rec - gt (named after the scene's mean
absolute error, :179); printed per scene: mean absolute RGB error and PSNR on the 8-bit pictures (:164-172).  PNG files
are read and written by networks/png_io.py (8 bits per sample, non-interlaced).  Without --weights the network runs on
its random initialisation (plumbing check only).  --precision runs the network in reduced precision: a cast model (bf16,
fp16) or a float32 model under torch.autocast.  --gpu-io does the pixel work around the network (float conversion, padding,
quantisation, error sums, difference picture) on the device: the same bytes and numbers; --scenes-per-step N sends up to N
consecutive scenes of one size through the network at once; --ssim adds the RGB SSIM (the mean over the three channels, as
demo_Vimeo_VE.py:168 reports it) as a third column.  --first / --second / --middle name the files of a scene, so that a
Vimeo-90K tree (im1.png, im3.png, im2.png) runs as it is.  --fused-half-level (MEMC_Net_s under --precision bf16 / fp16): the
flow estimator's pyramid-level inputs by the half-precision kernel (libmemc_hip_spynet_lp.so) instead of the torch expression
on half tensors; off by default, since it changes the values a cast model computes.  Needs a GPU: the operators have no CPU path.
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
    ap.add_argument("--data", required=True, help="directory of scene directories holding frame10.png / frame11.png")
    ap.add_argument("--gt", default="", help="directory of scene directories holding frame10i11.png")
    ap.add_argument("--output", required=True)
    ap.add_argument("--model", default="MEMC_Net_star", choices=["MEMC_Net_star", "MEMC_Net", "MEMC_Net_s"],
                    help="MEMC_Net_s: the reference README's `demo_MiddleBury.py --netName MEMC_Net_s --pretrained MEMC-Net_s_best.pth`")
    ap.add_argument("--weights", default="")
    ap.add_argument("--align-corners", action="store_true",
                    help="bilinear upsampling as PyTorch 0.2 did it: what the published checkpoints were trained with")
    ap.add_argument("--save-which", type=int, default=1, choices=[0, 1], help="0: blended, 1: rectified (the demos' save_which)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16", "fp16", "autocast-bf16", "autocast-fp16"],
                    help="fp32 (default): as ever.  bf16 / fp16: the model is cast after its weights are loaded and fed planes of "
                         "that dtype -- bf16 is the cast mode to prefer, an fp16 cast can overflow in the dense layers.  "
                         "autocast-bf16 / autocast-fp16: the float32 model runs inside torch.autocast on float32 planes")
    ap.add_argument("--gpu-io", action="store_true",
                    help="frame I/O and scores on the device (libmemc_hip_still.so) instead of in numpy on the host")
    ap.add_argument("--scenes-per-step", type=int, default=1, metavar="N",
                    help="consecutive scenes of one size that go through the network as one batch (default 1)")
    ap.add_argument("--ssim", action="store_true", help="also report the RGB SSIM (mean over the three channels)")
    ap.add_argument("--fused-half-level", action="store_true",
                    help="MEMC_Net_s cast to bf16 / fp16: SPyNet's level inputs by the half-precision kernel (sets "
                         "flownets.fused_level_half; off by default: the kernel samples at float32 positions, the torch "
                         "expression at positions rounded to the half dtype)")
    ap.add_argument("--first", default="frame10.png", help="file name of a scene's first frame")
    ap.add_argument("--second", default="frame11.png", help="file name of a scene's second frame")
    ap.add_argument("--middle", default="frame10i11.png", help="file name of the frame in between (output and ground truth)")
    a = ap.parse_args(argv)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the HIP operators have no CPU fallback")
    import networks
    dev = torch.device("cuda", 0)
    net = getattr(networks, a.model)(channel=3, filter_size=4, training=False, align_corners=a.align_corners)
    if a.weights:
        # as the reference demo does (demo_MiddleBury.py:48-60): keep the checkpoint's entries that exist in the model, load
        # those, leave the rest of the model as constructed -- and say what was left out on either side
        state = torch.load(a.weights, map_location="cpu")
        state = state.get("state_dict", state)
        own = net.state_dict()
        kept = {k: v for k, v in state.items() if k in own}
        skipped, missing = sorted(set(state) - set(own)), sorted(set(own) - set(state))
        own.update(kept)
        net.load_state_dict(own, strict=True)
        if skipped or missing:
            print("checkpoint: %d entries loaded, %d not in the model (%s...), %d of the model not in the checkpoint (%s...)" % (
                len(kept), len(skipped), ", ".join(skipped[:3]), len(missing), ", ".join(missing[:3])))
    net = net.to(dev).eval()
    half = {"bf16": torch.bfloat16, "fp16": torch.float16}
    dtype = half.get(a.precision)
    autocast = half.get(a.precision[len("autocast-"):]) if a.precision.startswith("autocast-") else None
    if dtype is not None:
        net = net.to(dtype)
    if a.fused_half_level:
        if a.model != "MEMC_Net_s":
            raise SystemExit("--fused-half-level: only MEMC_Net_s has a SPyNet flow estimator")
        net.flownets.fused_level_half = True
    os.makedirs(a.output, exist_ok=True)
    kw = dict(dtype=dtype, autocast=autocast) if a.precision != "fp32" else {}
    for name, value, default in (("first", a.first, "frame10.png"), ("second", a.second, "frame11.png"),
                                 ("middle", a.middle, "frame10i11.png"), ("gpu_io", a.gpu_io, False),
                                 ("scenes_per_step", a.scenes_per_step, 1), ("ssim", a.ssim, False)):
        if value != default:                               # a default run makes the call it always made
            kw[name] = value
    results = networks.interpolate_png_tree(net, a.data, a.output, dev, gt_dir=a.gt or None, which=a.save_which, **kw)
    scored = [r for r in results if r[1] is not None]
    what = "interpolation error / PSNR / SSIM" if a.ssim else "interpolation error / PSNR"
    fmt = " / ".join(["%.4f"] * (3 if a.ssim else 2))
    for r in results:
        if r[1] is None:
            print("%-16s written (no ground truth)" % r[0])
        else:
            print(("%-16s " + what + " : " + fmt) % tuple(r))
    if scored:
        print(("The average " + what + " for all %d images are : " + fmt) % (
            (len(scored),) + tuple(sum(r[k] for r in scored) / len(scored) for k in range(1, len(scored[0])))))


if __name__ == "__main__":
    main()
