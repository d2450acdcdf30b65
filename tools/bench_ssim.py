#!/usr/bin/env python
"""tools/bench_ssim.py -- what the HD demo loop's third score costs: the SSIM kernels of libmemc_hip_ssim.so against the host
rule (networks/yuv_io.py::luma_ssim), and the loop (interpolate_yuv_sequence(gpu_io=True)) with and without ssim=True.

    python tools/bench_ssim.py [--height 720 --width 1280] [--launches 200 --rounds 5] [--host-reps 3]
                               [--pairs 5 --loop-rounds 4] [--out profiles/r17_ssim.txt]

Part 1: memc_ssim_luma_rgb on 1, 4 and 32 frame pairs of random RGB bytes: HIP events around `--launches` calls on one
        stream (a warm-up call first), `--rounds` times; microseconds per call and per frame, median and spread.  Each
        result is first checked against the host rule on frame 0.
Part 2: luma_ssim on the same frames on the host, wall clock, `--host-reps` times.
Part 3: the loop on a synthetic clip with a stub model (the mean of the two frames; the time is the I/O and the scores), the
        two settings alternating, a host clock around the whole call ending in a device synchronise: ms per pair.
The host figures are figures of the CPU of the machine this runs on; the report names it.  Needs a GPU.
"""
import argparse
import os
import platform
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def stub_model(x):
    mid = (x[0] + x[1]) * 0.5
    return [mid, mid], None, None, None


def spread(values):
    return "median %.2f  min %.2f  max %.2f" % (statistics.median(values), min(values), max(values))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--loop-rounds", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the SSIM kernels have no CPU path")
    import my_package._ext.my_lib_ssim as S
    import networks
    from networks import yuv_io
    dev = torch.device("cuda", 0)
    h, w = a.height, a.width
    lines = ["SSIM of the luma planes (libmemc_hip_ssim.so) against the host rule, %dx%d, one process" % (w, h),
             "host CPU (the host figures are this CPU's): %s, %s logical CPUs visible" % (cpu_name(), os.cpu_count()),
             "GPU: %s; %s" % (torch.cuda.get_device_name(0), S.version()), ""]

    # ---- 1. the kernels, 2. the host rule on the same frames
    rng = np.random.default_rng(0)
    host_rgb = [rng.integers(0, 256, (32, h, w, 3), dtype=np.uint8) for _ in range(2)]
    host_rgb[1][:, ::2] = host_rgb[0][:, ::2]             # every second row equal: SSIM neither 0 nor 1
    lines.append("memc_ssim_luma_rgb: HIP events around %d calls on one stream, %d rounds; us per call" % (a.launches, a.rounds))
    for frames in (1, 4, 32):
        ta, tb = (torch.from_numpy(x[:frames]).to(dev) for x in host_rgb)
        out = torch.empty(frames, dtype=torch.float64, device=dev)
        work = torch.empty(S.ssim_workspace_bytes(frames, h, w), dtype=torch.uint8, device=dev)
        call = lambda: S.ssim_luma_rgb(ta, tb, frames, h, w, out, work)
        assert call() == 0
        torch.cuda.synchronize()
        want = yuv_io.luma_ssim(host_rgb[0][0], host_rgb[1][0])
        got = float(out[0].item())
        tol = (32 + (h - 6) * (w - 6)) * 2.0 ** -53
        lines.append("  frames %2d: frame 0: gpu %.17g host %.17g |diff| %.3g (tolerance %.3g)%s" % (
            frames, got, want, abs(got - want), tol, "" if abs(got - want) <= tol else "  BEYOND THE TOLERANCE"))
        us = []
        for _ in range(a.rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(a.launches):
                call()
            stop.record()
            stop.synchronize()
            us.append(1e3 * start.elapsed_time(stop) / a.launches)
        lines.append("  frames %2d: us per call: %s;  us per frame at the median: %.2f" % (
            frames, spread(us), statistics.median(us) / frames))
    lines.append("")
    ms = []
    for _ in range(a.host_reps):
        t = time.perf_counter()
        yuv_io.luma_ssim(host_rgb[0][0], host_rgb[1][0])
        ms.append(1e3 * (time.perf_counter() - t))
    lines.append("luma_ssim on the host (numpy; luma planes and 2-D cumulative sums), one frame pair: ms: %s" % spread(ms))
    y0, y1 = ((yuv_io.rgb_to_yuv(x[0] / 255.0)[:, :, 0] * 255.0).astype(np.uint8) for x in host_rgb)
    ms = []
    for _ in range(a.host_reps):
        t = time.perf_counter()
        yuv_io.ssim_from_planes(y0, y1)
        ms.append(1e3 * (time.perf_counter() - t))
    lines.append("ssim_from_planes on the host, the luma planes given: ms: %s" % spread(ms))
    lines.append("")

    # ---- 3. the loop with and without the third score
    tmp = tempfile.mkdtemp(prefix="memc_ssim_")
    src, dst = os.path.join(tmp, "in.yuv"), os.path.join(tmp, "out.yuv")
    with open(src, "wb") as f:
        for _ in range(2 * a.pairs + 1):
            f.write(rng.integers(0, 256, yuv_io.frame_bytes(h, w), dtype=np.uint8).tobytes())
    try:
        def run(ssim, n):
            kw = dict(ssim=True) if ssim else {}
            scores = networks.interpolate_yuv_sequence(stub_model, src, dst, h, w, dev, first=0, last=2 * n, gpu_io=True, **kw)
            assert len(scores) == n and len(scores[0]) == (4 if ssim else 3)
        for ssim in (False, True):
            run(ssim, 1)
        per_pair = {False: [], True: []}
        for _ in range(a.loop_rounds):
            for ssim in (False, True):
                torch.cuda.synchronize()
                t = time.perf_counter()
                run(ssim, a.pairs)
                torch.cuda.synchronize()
                per_pair[ssim].append(1e3 * (time.perf_counter() - t) / a.pairs)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    lines.append("interpolate_yuv_sequence(gpu_io=True), stub model, %d pairs per call, %d rounds, the settings alternating; host "
                 "clock (file I/O included) ending in a device synchronise; ms per pair" % (a.pairs, a.loop_rounds))
    lines.append("  without ssim: by round %s;  %s" % (" ".join("%.2f" % v for v in per_pair[False]), spread(per_pair[False])))
    lines.append("  ssim=True:    by round %s;  %s" % (" ".join("%.2f" % v for v in per_pair[True]), spread(per_pair[True])))
    lines.append("  added per pair at the medians: %.3f ms" % (statistics.median(per_pair[True]) - statistics.median(per_pair[False])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
