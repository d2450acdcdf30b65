#!/usr/bin/env python
"""tools/bench_video_io.py -- the HD demo loop (networks/yuv_io.py::interpolate_yuv_sequence) with its frame I/O in numpy on the
host against gpu_io=True (libmemc_hip_video.so), in ONE process, the two alternating.

    python tools/bench_video_io.py [--height 720 --width 1280] [--pairs 5 --rounds 4] [--net-pairs 4 --net-rounds 3]
                                   [--skip-network] [--out profiles/r15_video_io.txt]

Part 1: a stub model (the mean of the two frames), so that the time is the I/O around the network: per round `--pairs` frame
pairs through the numpy path, then as many through gpu_io; host clock around the whole call (file reads and writes included),
ending in a device synchronise; one warm-up pair each way first.  Reported: milliseconds per pair, per round and the median.
Part 2: the real MEMC_Net_star (random initialisation) both ways: pairs per second.
The clip is random bytes in a temporary file: the arithmetic does not depend on the content.
The numpy figure is a figure of the CPU of the machine this runs on; the report names it.
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


def timed(torch, fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def alternate(torch, networks, model, src, dst, h, w, dev, pairs, rounds, lines, label):
    """ms per pair of each path, per round; the paths alternate within a round"""
    def run(gpu_io, n):
        scores = networks.interpolate_yuv_sequence(model, src, dst, h, w, dev, first=0, last=2 * n, gpu_io=gpu_io)
        assert len(scores) == n, (len(scores), n)
    for gpu_io in (False, True):
        run(gpu_io, 1)                                     # warm-up: library load, allocator, solver choice
    ms = {False: [], True: []}
    for _ in range(rounds):
        for gpu_io in (False, True):
            ms[gpu_io].append(1e3 * timed(torch, lambda: run(gpu_io, pairs)) / pairs)
    for gpu_io, name in ((False, "numpy on the host"), (True, "gpu_io=True")):
        lines.append("%s, %-18s ms per pair by round: %s   median %.2f" % (
            label, name + ":", " ".join("%.2f" % v for v in ms[gpu_io]), statistics.median(ms[gpu_io])))
    return statistics.median(ms[False]), statistics.median(ms[True])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--net-pairs", type=int, default=4)
    ap.add_argument("--net-rounds", type=int, default=3)
    ap.add_argument("--skip-network", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the HIP operators have no CPU fallback")
    # MIOpen gets a private copy of the in-tree kernel database, as in bench.py
    cache_src = os.path.join(ROOT, "memc-net_amd", "networks", "miopen_cache")
    if "MIOPEN_USER_DB_PATH" not in os.environ and "MIOPEN_CUSTOM_CACHE_DIR" not in os.environ and os.path.isdir(cache_src):
        tmp = tempfile.mkdtemp(prefix="memc_miopen_")
        for name in os.listdir(cache_src):
            if not name.endswith(".md"):
                shutil.copy(os.path.join(cache_src, name), tmp)
        os.environ["MIOPEN_USER_DB_PATH"] = os.environ["MIOPEN_CUSTOM_CACHE_DIR"] = tmp
    import networks
    from networks import yuv_io
    dev = torch.device("cuda", 0)
    h, w = a.height, a.width
    work = tempfile.mkdtemp(prefix="memc_video_io_")
    src, dst = os.path.join(work, "in.yuv"), os.path.join(work, "out.yuv")
    n_frames = 2 * max(a.pairs, a.net_pairs) + 1
    rng = np.random.default_rng(0)
    with open(src, "wb") as f:
        for _ in range(n_frames):
            f.write(rng.integers(0, 256, yuv_io.frame_bytes(h, w), dtype=np.uint8).tobytes())

    lines = ["HD demo loop, frame I/O in numpy on the host against gpu_io=True, %dx%d, one process, the paths alternating" % (w, h),
             "host CPU (the numpy figures are this CPU's): %s, %s logical CPUs visible" % (cpu_name(), os.cpu_count()),
             "GPU: %s" % torch.cuda.get_device_name(0),
             "host clock around interpolate_yuv_sequence (file I/O included), ending in a device synchronise", ""]
    try:
        host, gpu = alternate(torch, networks, stub_model, src, dst, h, w, dev, a.pairs, a.rounds, lines, "stub model")
        lines.append("stub model: %d pairs each way; gpu_io takes x%.3f of the numpy path's time per pair" % (
            a.pairs * a.rounds, gpu / host))
        if not a.skip_network:
            with torch.device(dev):
                net = networks.MEMC_Net_star(channel=3, filter_size=4, training=False)
            net = net.to(dev).eval()
            lines.append("")
            host, gpu = alternate(torch, networks, net, src, dst, h, w, dev, a.net_pairs, a.net_rounds, lines, "MEMC_Net_star")
            lines.append("MEMC_Net_star (fp32, one pair per step), %d pairs each way: %.2f pairs/s with numpy I/O, %.2f pairs/s with "
                         "gpu_io: x%.2f end to end" % (a.net_pairs * a.net_rounds, 1e3 / host, 1e3 / gpu, host / gpu))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
