#!/usr/bin/env python
"""tools/demo_vimeo_ve.py -- the reference's video-enhancement demo (demo_Vimeo_VE.py) on this repository's operators: for
every septuplet of a Vimeo-90K tree, enhance (denoise, deblock or super-resolve) the centre frame and score it against the
target.

    python tools/demo_vimeo_ve.py --input vimeo/input --target vimeo/target --output results
                                  [--list vimeo/sep_testlist.txt] [--weights best.pth --align-corners]
                                  [--gpu-io] [--ssim] [--composed]
                                  [--precision {fp32,bf16,fp16,autocast-bf16,autocast-fp16}]

Reads <input>/<sequence>/<clip>/im1.png .. im7.png, replicate-pads every frame like demo_Vimeo_VE.py:115-135 (to multiples
of 128; a side that already is one gets 32 + 32, so 256 x 448 runs as 320 x 512), runs MEMC_Net_VE and crops; results/
<sequence>/<clip>/ receives im4.png; printed per clip: mean absolute RGB error and PSNR on the 8-bit pictures (:157-167),
with --ssim the RGB SSIM (:168); the averages go to results/metrics.txt in the reference's wording (:175-181).  The clips
are those --list names (one <sequence>/<clip> per line), or every clip of the tree.  PNG files are read and written by
networks/png_io.py (8 bits per sample, non-interlaced).  Without --weights the network runs on its random initialisation
(plumbing check only).  --gpu-io does the pixel work around the network (float conversion, padding, quantisation, error
sums, SSIM) on the device: the same bytes and numbers.  --composed fills the rectifier's input by twelve warps and
torch.cat, the reference's sequence, instead of two stacked warps (MEMC_Net_VE.fused_stack).  --precision runs the network
in reduced precision: a cast model (bf16, fp16) or a float32 model under torch.autocast.  Needs a GPU: the operators have
no CPU path.
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
    ap.add_argument("--input", required=True, help="directory of <sequence>/<clip>/im1.png .. im7.png (the degraded frames)")
    ap.add_argument("--target", required=True, help="directory of <sequence>/<clip>/im4.png (the clean centre frames)")
    ap.add_argument("--output", required=True)
    ap.add_argument("--list", default="", help="file naming one <sequence>/<clip> per line (sep_testlist.txt)")
    ap.add_argument("--weights", default="")
    ap.add_argument("--align-corners", action="store_true",
                    help="bilinear upsampling as PyTorch 0.2 did it: what the published checkpoints were trained with")
    ap.add_argument("--gpu-io", action="store_true",
                    help="frame I/O and scores on the device (libmemc_hip_still.so) instead of in numpy on the host")
    ap.add_argument("--ssim", action="store_true", help="also report the RGB SSIM (mean over the three channels)")
    ap.add_argument("--composed", action="store_true", help="twelve warps and torch.cat instead of two stacked warps")
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
    # the reference demo's constructor arguments (demo_Vimeo_VE.py:40-42)
    net = networks.MEMC_Net_VE(batch=1, channel=3, width=None, height=None, scale_num=1, scale_ratio=2, temporal=False,
                               filter_size=4, save_which=1, debug=False, offset_scale=None, cuda_available=True,
                               cuda_id=None, training=False, align_corners=a.align_corners)
    if a.weights:
        state = torch.load(a.weights, map_location="cpu")
        net.load_state_dict(state.get("state_dict", state), strict=True)
    if a.composed:
        net.fused_stack = False
    net = net.to(dev).eval()
    half = {"bf16": torch.bfloat16, "fp16": torch.float16}
    dtype = half.get(a.precision)
    autocast = half.get(a.precision[len("autocast-"):]) if a.precision.startswith("autocast-") else None
    if dtype is not None:
        net = net.to(dtype)
    kw = dict(dtype=dtype, autocast=autocast) if a.precision != "fp32" else {}      # a default run makes the call it always made
    os.makedirs(a.output, exist_ok=True)
    results = networks.enhance_septuplet_tree(net, a.input, a.target, a.output, dev, list_file=a.list or None,
                                              gpu_io=a.gpu_io, ssim=a.ssim, **kw)
    what = "interpolation error / PSNR / SSIM" if a.ssim else "interpolation error / PSNR"
    fmt = " / ".join(["%.4f"] * (3 if a.ssim else 2))
    for r in results:
        print(("%-16s " + what + " : " + fmt) % tuple(r))
    if results:
        print(open(os.path.join(a.output, "metrics.txt")).read().rstrip("\n"))


if __name__ == "__main__":
    main()
