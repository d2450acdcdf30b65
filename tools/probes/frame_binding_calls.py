#!/usr/bin/env python
"""tools/probes/frame_binding_calls.py -- what a call of the plane bindings costs on the host: the enqueue time of i420_decode
and rgb_quantise (my_lib_video and my_lib_video_lp), rgb8_decode (my_lib_still) and ssim_u8 (my_lib_ssim) on 2 frames of
64x48, the device far from busy, so that the figure is the binding's Python and the launch, not the kernel.

    python tools/probes/frame_binding_calls.py run <tree>/memc-net_amd <label> <out.json>   # one process per run
    python tools/probes/frame_binding_calls.py compare <out.txt> <parent run>.json ... -- <new run>.json ...

run: per function 200 calls unmeasured, then 20 windows of 200 calls, a device synchronise between the windows and none
inside; the run's figure is the median window, in microseconds per call.  compare: per function the parent's runs (median,
lowest, highest), the new tree's, and whether the new median lies within the parent's lowest .. highest."""
import json
import statistics
import sys
import time

F, H, W, CALLS, WINDOWS = 2, 48, 64, 200, 20


def run(package_dir, label, out):
    sys.path.insert(0, package_dir)
    import torch
    import my_package._ext.my_lib_ssim as SS
    import my_package._ext.my_lib_still as S
    import my_package._ext.my_lib_video as V
    import my_package._ext.my_lib_video_lp as VL
    dev = torch.device("cuda", 0)
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)      # noqa: E731
    i420, rgb = z((F * V.frame_bytes(H, W),), torch.uint8), z((F, H, W, 3), torch.uint8)
    f32, f16 = z((F, 3, H, W), torch.float32), z((F, 3, H, W), torch.float16)
    a, b, ssim = z((F, H, W), torch.uint8), z((F, H, W), torch.uint8), z((F,), torch.float64)
    work = z((SS.ssim_workspace_bytes(F, H, W),), torch.uint8)
    calls = {"my_lib_video.i420_decode": lambda: V.i420_decode(i420, F, H, W, rgb=rgb, planes=f32),
             "my_lib_video.rgb_quantise": lambda: V.rgb_quantise(f32, rgb),
             "my_lib_video_lp.i420_decode": lambda: VL.i420_decode(i420, F, H, W, rgb=rgb, planes=f16),
             "my_lib_video_lp.rgb_quantise": lambda: VL.rgb_quantise(f16, rgb),
             "my_lib_still.rgb8_decode": lambda: S.rgb8_decode(rgb, f16),
             "my_lib_ssim.ssim_u8": lambda: SS.ssim_u8(a, b, ssim, work)}
    res = {}
    for name, f in calls.items():
        assert f() == 0, name
        for _i in range(CALLS):
            f()
        torch.cuda.synchronize()
        windows = []
        for _w in range(WINDOWS):
            t0 = time.perf_counter()
            for _i in range(CALLS):
                f()
            windows.append((time.perf_counter() - t0) / CALLS * 1e6)
            torch.cuda.synchronize()
        res[name] = {"median_us": statistics.median(windows), "windows_us": windows}
        print("%-8s %-30s %.3f us/call" % (label, name, res[name]["median_us"]), flush=True)
    json.dump(res, open(out, "w"), indent=1)


def compare(out, parent, new):
    load = lambda paths: [json.load(open(p)) for p in paths]      # noqa: E731
    parent, new = load(parent), load(new)
    lines = ["enqueue time per call, microseconds: median of the runs (lowest .. highest); %d parent runs, %d new runs,"
             % (len(parent), len(new)),
             "alternating, one process per run, %d windows of %d calls per run, 2 frames of %dx%d" % (WINDOWS, CALLS, W, H), ""]
    for name in parent[0]:
        p, n = ([r[name]["median_us"] for r in runs] for runs in (parent, new))
        inside = min(p) <= statistics.median(n) <= max(p)
        lines.append("%-30s parent %7.3f (%7.3f .. %7.3f)   new %7.3f (%7.3f .. %7.3f)   new median %s the parent's spread"
                     % (name, statistics.median(p), min(p), max(p), statistics.median(n), min(n), max(n),
                        "within" if inside else "below" if statistics.median(n) < min(p) else "ABOVE"))
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "run":
        run(*sys.argv[2:])
    elif len(sys.argv) > 4 and sys.argv[1] == "compare" and "--" in sys.argv:
        cut = sys.argv.index("--")
        compare(sys.argv[2], sys.argv[3:cut], sys.argv[cut + 1:])
    else:
        sys.exit(__doc__)
