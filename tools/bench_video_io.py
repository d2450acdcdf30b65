#!/usr/bin/env python
"""tools/bench_video_io.py -- the HD demo loop (networks/yuv_io.py::interpolate_yuv_sequence) with its frame I/O in numpy on the
host against gpu_io=True (libmemc_hip_video.so), in ONE process, the two alternating.

    python tools/bench_video_io.py [--height 720 --width 1280] [--pairs 5 --rounds 4] [--net-pairs 4 --net-rounds 3]
                                   [--skip-network] [--out profiles/r15_video_io.txt] [--only {io,lp}]
                                   [--lp-frames 4 --lp-reps 20 --lp-rounds 7]

Part 1: a stub model (the mean of the two frames), so that the time is the I/O around the network: per round `--pairs` frame
pairs through the numpy path, then as many through gpu_io; host clock around the whole call (file reads and writes included),
ending in a device synchronise; one warm-up pair each way first.  Reported: milliseconds per pair, per round and the median.
Part 2: the real MEMC_Net_star (random initialisation) both ways: pairs per second.
--only lp: the frame I/O of a network in fp16 / bf16 (libmemc_hip_video_lp.so) instead, each row against its alternative, the
two alternating round by round in this one process, both dtypes:
    decode_lp     a step's two decode calls (`--lp-frames` pairs) into a half input   | the float32 decode, then .to(T)
    quantise_lp   the quantiser on the half crop of the network's output               | .float(), then the float32 quantiser
(device events around `--lp-reps` repetitions; allocations and casts count on the side that needs them), then the whole loop
with MEMC_Net_star and gpu_io=True in fp32, as a bf16 cast and under bf16 autocast: milliseconds per pair, the modes
alternating, the fp32 figure of the same process the baseline.
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


def spread(values):
    return "%s   median %.1f  min %.1f  max %.1f" % (" ".join("%.1f" % v for v in values), statistics.median(values),
                                                     min(values), max(values))


def lp_kernels(torch, h, w, dev, frames, reps, rounds, lines):
    """the two rows of the lp group, per dtype: microseconds per call (decode: per pair of calls), A and B alternating"""
    import numpy as np
    import my_package._ext.my_lib_video as V
    import my_package._ext.my_lib_video_lp as VL
    from networks.inference import pad_amounts
    left, right, top, bottom = pads = pad_amounts(h, w)
    hp, wp = h + top + bottom, w + left + right
    fb = V.frame_bytes(h, w)
    raw = torch.from_numpy(np.random.default_rng(1).integers(0, 256, 2 * frames * fb, dtype=np.uint8)).to(dev).view(2, frames, fb)
    rgb_a, rec = (torch.empty((frames, h, w, 3), dtype=torch.uint8, device=dev) for _ in range(2))

    def ok(code):
        assert code == 0, code

    def events(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        torch.cuda.synchronize()
        return 1e3 * start.elapsed_time(stop) / reps

    for T in (torch.bfloat16, torch.float16):
        def decode_lp():
            x = torch.empty((2, frames, 3, hp, wp), dtype=T, device=dev)
            ok(VL.i420_decode(raw[0], frames, h, w, rgb=rgb_a, planes=x[0], pads=pads))
            ok(VL.i420_decode(raw[1], frames, h, w, planes=x[1], pads=pads))
            return x

        def decode_f32_then_cast():
            x = torch.empty((2, frames, 3, hp, wp), dtype=torch.float32, device=dev)
            ok(V.i420_decode(raw[0], frames, h, w, rgb=rgb_a, planes=x[0], pads=pads))
            ok(V.i420_decode(raw[1], frames, h, w, planes=x[1], pads=pads))
            return x.to(T)
        assert torch.equal(decode_lp(), decode_f32_then_cast())
        crop = torch.rand((frames, 3, hp, wp), device=dev).to(T)[:, :, top:top + h, left:left + w]

        def quantise_lp():
            ok(VL.rgb_quantise(crop, rec))

        def float_then_quantise():
            ok(V.rgb_quantise(crop.float(), rec))
        quantise_lp()
        want = rec.clone()
        float_then_quantise()
        assert torch.equal(rec, want)
        for row, a, b, alt in (("decode_lp", decode_lp, decode_f32_then_cast, "float32 decode + .to(T)"),
                               ("quantise_lp", quantise_lp, float_then_quantise, ".float() + float32 quantise")):
            for fn in (a, b):
                events(fn)                                 # warm-up: code objects, the allocator's blocks
            us = {a: [], b: []}
            for _ in range(rounds):
                for fn in (a, b):
                    us[fn].append(events(fn))
            name = str(T).replace("torch.", "")
            lines.append("%-11s %-8s us by round: %s" % (row, name, spread(us[a])))
            lines.append("%-11s %-8s us by round: %s" % ("  against", name, spread(us[b])) + "   (%s)" % alt)
            lines.append("%-11s %-8s takes x%.3f of its alternative's time (medians)" % (
                row, name, statistics.median(us[a]) / statistics.median(us[b])))
        lines.append("")


def lp_loop(torch, networks, src, dst, h, w, dev, pairs, rounds, lines):
    """the whole loop, gpu_io=True, MEMC_Net_star: ms per pair in fp32, as a bf16 cast and under bf16 autocast, alternating"""
    import copy
    with torch.device(dev):
        net = networks.MEMC_Net_star(channel=3, filter_size=4, training=False)
    net = net.to(dev).eval()
    modes = (("fp32", net, dict()), ("bf16 cast", copy.deepcopy(net).to(torch.bfloat16), dict(dtype=torch.bfloat16)),
             ("bf16 autocast", net, dict(autocast=torch.bfloat16)))

    def run(model, kw, n):
        scores = networks.interpolate_yuv_sequence(model, src, dst, h, w, dev, first=0, last=2 * n, gpu_io=True, **kw)
        assert len(scores) == n, (len(scores), n)
    for name, model, kw in modes:
        t = timed(torch, lambda: run(model, kw, 1))        # warm-up: library load, allocator, solver choice
        print("warm-up %s: %.1f s" % (name, t), flush=True)
    ms = {name: [] for name, _m, _k in modes}
    for r in range(rounds):
        for name, model, kw in modes:
            ms[name].append(1e3 * timed(torch, lambda: run(model, kw, pairs)) / pairs)
        print("round %d done" % r, flush=True)
    base = statistics.median(ms["fp32"])
    for name, _m, _k in modes:
        lines.append("MEMC_Net_star %dx%d gpu_io=True, %-14s ms per pair by round: %s   x%.3f of fp32's median" % (
            w, h, name + ":", spread(ms[name]), statistics.median(ms[name]) / base))


def io_group(torch, networks, a, src, dst, h, w, dev):
    """numpy I/O against gpu_io=True: the stub model, then MEMC_Net_star"""
    lines = ["HD demo loop, frame I/O in numpy on the host against gpu_io=True, %dx%d, one process, the paths alternating" % (w, h),
             "host CPU (the numpy figures are this CPU's): %s, %s logical CPUs visible" % (cpu_name(), os.cpu_count()),
             "GPU: %s" % torch.cuda.get_device_name(0),
             "host clock around interpolate_yuv_sequence (file I/O included), ending in a device synchronise", ""]
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
    return lines


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
    ap.add_argument("--only", default="io", choices=["io", "lp"],
                    help="io (default): numpy I/O against gpu_io=True; lp: the fp16 / bf16 frame I/O against its alternatives and "
                         "the loop in fp32, bf16 cast and bf16 autocast")
    ap.add_argument("--lp-frames", type=int, default=4)
    ap.add_argument("--lp-reps", type=int, default=20)
    ap.add_argument("--lp-rounds", type=int, default=7)
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

    try:
        if a.only == "lp":
            lines = ["HD demo loop in fp16 / bf16: the half frame I/O (libmemc_hip_video_lp.so) against its alternatives, %dx%d, "
                     "%d pairs per step, one process, A and B alternating" % (w, h, a.lp_frames),
                     "GPU: %s" % torch.cuda.get_device_name(0),
                     "device events around %d repetitions per figure; %d rounds" % (a.lp_reps, a.lp_rounds), ""]
            lp_kernels(torch, h, w, dev, a.lp_frames, a.lp_reps, a.lp_rounds, lines)
            if not a.skip_network:
                lines.append("host clock around interpolate_yuv_sequence (file I/O included), ending in a device synchronise; "
                             "%d pairs per figure, one pair per step" % a.net_pairs)
                lp_loop(torch, networks, src, dst, h, w, dev, a.net_pairs, a.net_rounds, lines)
        else:
            lines = io_group(torch, networks, a, src, dst, h, w, dev)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
