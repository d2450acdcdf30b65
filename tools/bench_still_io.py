#!/usr/bin/env python
"""tools/bench_still_io.py -- the still-image demo loop (networks/png_io.py::interpolate_png_tree): its pixel work in numpy on
the host against gpu_io=True (libmemc_hip_still.so), and scenes_per_step 1 against 8, in ONE process, A and B alternating.

    python tools/bench_still_io.py [--rounds 7 --reps 5] [--scenes 32 --batch 8 --net-rounds 7] [--skip-network]
                                   [--out profiles/r20_still_io.txt]

Part (a): the I/O of one step without the model call, for n scenes of h x w with ground truth -- 16 x 448 x 256 (w x h) and
1 x 640 x 480, float32 and bfloat16 planes:
    A  what the host route does around the model call: float conversion of both frames and upload, the cast, two F.pad and a
       stack; on a stand-in for the model's output: crop, widen, clamp, scale, download, round, transpose; rgb_scores per scene
    B  the GPU route's calls for the same bytes: upload of the bytes, two rgb8_decode into one input, rgb8_quantise of the
       crop, rgb8_score with the difference picture, download of bytes and sums, rgb_scores_from_sums per scene
Host clock around `--reps` repetitions, ending in a device synchronise; milliseconds per step by round.  Both sides are held to
the same bytes and floats before anything is timed.
Part (b): MEMC_Net_star (random initialisation) as a bfloat16 cast through interpolate_png_tree(gpu_io=True) on a generated
tree of `--scenes` scenes of 448 x 256 with ground truth, scenes_per_step 1 against `--batch`: seconds per scene by round,
PNG reading and writing included.
The pictures are random bytes: the arithmetic does not depend on the content (zlib's time does: random bytes are its worst
case).  The numpy figures are figures of the CPU of the machine this runs on; the report names it.
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


def timed(torch, fn, reps=1):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def spread(values, fmt="%.3f"):
    return "%s   median %s  min %s  max %s" % (" ".join(fmt % v for v in values), fmt % statistics.median(values),
                                               fmt % min(values), fmt % max(values))


def io_of_one_step(torch, np, png_io, dev, n, h, w, T, rounds, reps, lines):
    import torch.nn.functional as F
    import my_package._ext.my_lib_still as S
    from networks.inference import pad_amounts
    left, right, top, bottom = pads = pad_amounts(h, w)
    hp, wp = h + top + bottom, w + left + right
    rng = np.random.default_rng(n * h + w)
    a, b, gt = (rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8) for _ in range(3))
    half = T if T != torch.float32 else None
    y = torch.rand((n, 3, hp, wp), device=dev).mul_(1.2).sub_(0.1).to(T)      # a stand-in for what the model returns

    def ok(code):
        assert code == 0, code

    def host():
        def to_tensor(imgs):
            x = np.stack([np.transpose(img, (2, 0, 1)) for img in imgs])
            return torch.from_numpy(x.astype(np.float32) / 255.0).to(dev)
        f0, f2 = to_tensor(a), to_tensor(b)
        if half is not None:
            f0, f2 = f0.to(half), f2.to(half)
        x = torch.stack([F.pad(f, (left, right, top, bottom), mode="replicate") for f in (f0, f2)])
        mid = y[:, :, top:top + h, left:left + w]
        if half is not None:
            mid = mid.float()
        recs = np.round(255.0 * mid.clamp(0.0, 1.0).cpu().numpy()).astype(np.uint8)
        out = []
        for k in range(n):
            rec = np.ascontiguousarray(np.transpose(recs[k], (1, 2, 0)))
            out.append((rec,) + png_io.rgb_scores(rec, gt[k]))
        return x, out

    def gpu():
        raw = torch.from_numpy(np.stack([a, b, gt])).to(dev)
        x = torch.empty((2, n, 3, hp, wp), dtype=T, device=dev)
        ok(S.rgb8_decode(raw[0], x[0], pads))
        ok(S.rgb8_decode(raw[1], x[1], pads))
        res = torch.empty((2 * n, h, w, 3), dtype=torch.uint8, device=dev)
        ok(S.rgb8_quantise(y[:, :, top:top + h, left:left + w], res[:n]))
        sums = torch.empty((n, 2), dtype=torch.int64, device=dev)
        work = torch.empty(S.rgb8_score_workspace_bytes(n, h, w), dtype=torch.uint8, device=dev)
        ok(S.rgb8_score(res[:n], raw[2], sums, work, diff=res[n:]))
        res, sums = res.cpu().numpy(), sums.cpu().numpy().view(np.uint64)
        return x, [(res[k],) + png_io.rgb_scores_from_sums(sums[k, 0], sums[k, 1], 3 * h * w) + (res[n + k],) for k in range(n)]

    (xa, oa), (xb, ob) = host(), gpu()                     # warm-up, and: the same input, bytes and floats
    assert torch.equal(xa, xb)
    for ra, rb in zip(oa, ob):
        assert np.array_equal(ra[0], rb[0]) and ra[1:3] == rb[1:3] and np.array_equal(ra[3], rb[3])
    ms = {host: [], gpu: []}
    for _ in range(rounds):
        for fn in (host, gpu):
            ms[fn].append(1e3 * timed(torch, fn, reps))
    name = "%2d x %dx%d %-8s" % (n, w, h, str(T).replace("torch.", ""))
    lines.append("%s A numpy on the host, ms per step by round: %s" % (name, spread(ms[host])))
    lines.append("%s B gpu_io=True,       ms per step by round: %s" % (name, spread(ms[gpu])))
    lines.append("%s B takes x%.3f of A's time (medians)" % (name, statistics.median(ms[gpu]) / statistics.median(ms[host])))
    lines.append("")


def batches(torch, np, networks, dev, scenes, batch, rounds, lines):
    h, w = 256, 448
    work = tempfile.mkdtemp(prefix="memc_still_io_")
    try:
        rng = np.random.default_rng(0)
        data, gt, out = (os.path.join(work, d) for d in ("data", "gt", "out"))
        for k in range(scenes):
            for root, names in ((data, ("im1.png", "im3.png")), (gt, ("im2.png",))):
                os.makedirs(os.path.join(root, "%05d" % k))
                for name in names:
                    networks.write_png(os.path.join(root, "%05d" % k, name), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        with torch.device(dev):
            net = networks.MEMC_Net_star(channel=3, filter_size=4, training=False)
        net = net.to(dev).eval().to(torch.bfloat16)

        def run(n):
            res = networks.interpolate_png_tree(net, data, out, dev, gt_dir=gt, first="im1.png", second="im3.png",
                                                middle="im2.png", dtype=torch.bfloat16, gpu_io=True, scenes_per_step=n)
            assert len(res) == scenes and all(r[1] is not None for r in res)
            shutil.rmtree(out, ignore_errors=True)
        for n in (1, batch):
            t = timed(torch, lambda: run(n))               # warm-up: library load, allocator, solver choice
            print("warm-up scenes_per_step=%d: %.1f s" % (n, t), flush=True)
        s = {1: [], batch: []}
        for r in range(rounds):
            for n in (1, batch):
                s[n].append(timed(torch, lambda: run(n)) / scenes)
            print("round %d done" % r, flush=True)
        for n in (1, batch):
            lines.append("MEMC_Net_star bf16 cast, gpu_io=True, %d scenes of %dx%d, scenes_per_step=%d, seconds per scene by "
                         "round: %s" % (scenes, w, h, n, spread(s[n], "%.4f")))
        lines.append("scenes_per_step=%d takes x%.3f of scenes_per_step=1's time per scene (medians)" % (
            batch, statistics.median(s[batch]) / statistics.median(s[1])))
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--net-rounds", type=int, default=7)
    ap.add_argument("--skip-network", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the HIP kernels have no CPU fallback")
    # MIOpen gets a private copy of the in-tree kernel database, as in bench.py
    cache_src = os.path.join(ROOT, "memc-net_amd", "networks", "miopen_cache")
    if "MIOPEN_USER_DB_PATH" not in os.environ and "MIOPEN_CUSTOM_CACHE_DIR" not in os.environ and os.path.isdir(cache_src):
        tmp = tempfile.mkdtemp(prefix="memc_miopen_")
        for name in os.listdir(cache_src):
            if not name.endswith(".md"):
                shutil.copy(os.path.join(cache_src, name), tmp)
        os.environ["MIOPEN_USER_DB_PATH"] = os.environ["MIOPEN_CUSTOM_CACHE_DIR"] = tmp
    import networks
    from networks import png_io
    dev = torch.device("cuda", 0)
    lines = ["still-image demo loop: pixel work in numpy on the host (A) against gpu_io=True (B, libmemc_hip_still.so), one "
             "process, A and B alternating over %d rounds" % a.rounds,
             "host CPU (the numpy figures are this CPU's): %s, %s logical CPUs visible" % (cpu_name(), os.cpu_count()),
             "GPU: %s" % torch.cuda.get_device_name(0),
             "(a) the I/O of one step without the model call; host clock around %d repetitions, ending in a device "
             "synchronise; n x width x height, storage of the planes" % a.reps, ""]
    for n, h, w in ((16, 256, 448), (1, 480, 640)):
        for T in (torch.float32, torch.bfloat16):
            io_of_one_step(torch, np, png_io, dev, n, h, w, T, a.rounds, a.reps, lines)
            print("\n".join(lines[-4:]), flush=True)
    if not a.skip_network:
        lines.append("(b) the whole loop, PNG reading and writing included; host clock around interpolate_png_tree, ending in a "
                     "device synchronise; %d rounds, the two alternating" % a.net_rounds)
        batches(torch, np, networks, dev, a.scenes, a.batch, a.net_rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
