"""tools/probes/satellite_calls.py MODE PKGDIR [LABEL OUT]: every satellite entry point through the ctypes bindings of PKGDIR.
geometry: one 2x3x24x72 call per entry point and dtype combination, the backwards with and without gradinput1 (run under
rocprofv3 --kernel-trace).  hostcost: wall time per call, 10 000 calls, median of five repeats, of a batch-0 call and of
one covered 2x3x24x72 call of each entry point."""
import json
import statistics
import sys
import time

mode, pkg = sys.argv[1], sys.argv[2]
sys.path.insert(0, pkg)
import torch  # noqa: E402
import my_package._ext.my_lib_lp as LP  # noqa: E402
import my_package._ext.my_lib_lp_grad as LPG  # noqa: E402
import my_package._ext.my_lib_blend_grad as BG  # noqa: E402
import my_package._ext.my_lib_mx as MX  # noqa: E402
import my_package._ext.my_lib_mx_grad as MXG  # noqa: E402

dev = torch.device("cuda:0")
H, W = 24, 72
f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16


def tensors(n, dt_img, dt_flow, dt_taps, dt_gout):
    g = torch.Generator(device="cpu").manual_seed(5)
    r = lambda c, dt, s=1.0: (torch.rand((n, c, H, W), generator=g) * s).to(dt).to(dev)      # noqa: E731
    t = dict(img=r(3, dt_img), img2=r(3, dt_img), flow=r(2, dt_flow, 3.0), flow2=r(2, dt_flow, 3.0), taps=r(16, dt_taps),
             taps2=r(16, dt_taps), occ=r(1, dt_taps), occ2=r(1, dt_taps), gout=r(3, dt_gout))
    t["out"] = torch.empty_like(t["img"])
    t["g1"] = torch.zeros((n, 3, H, W), dtype=f32, device=dev)
    t["g2"], t["g3"], t["gocc"] = torch.empty_like(t["flow"]), torch.empty_like(t["taps"]), torch.empty_like(t["occ"])
    return t


def calls(n, p, fl, go, with_g1):
    """(label, function, last_kernel_path) of the entry points for payload p, flow fl, gradoutput go"""
    lp, mx, bw = tensors(n, p, fl, p, go), tensors(n, f32, fl, p, f32), tensors(n, f32, f32, f32, f32)
    g1 = (lambda t: t["g1"] if with_g1 else None)
    return [
        ("lp.fwd", lambda t=lp: LP.FilterInterpolationLayer_gpu_forward_lp(t["img"], t["flow"], t["taps"], t["out"]), LP),
        ("lp.blend", lambda t=lp: LP.FilterInterpolationBlendLayer_gpu_forward_lp(
            t["img"], t["img2"], t["flow"], t["flow2"], t["taps"], t["taps2"], t["occ"], t["occ2"], t["out"]), LP),
        ("lp_grad.bwd", lambda t=lp: LPG.FilterInterpolationLayer_gpu_backward_lp(
            t["img"], t["flow"], t["taps"], t["gout"], g1(t), t["g2"], t["g3"]), LPG),
        ("mx.fwd", lambda t=mx: MX.FilterInterpolationLayer_gpu_forward_mx(t["img"], t["flow"], t["taps"], t["out"]), MX),
        ("mx.blend", lambda t=mx: MX.FilterInterpolationBlendLayer_gpu_forward_mx(
            t["img"], t["img2"], t["flow"], t["flow2"], t["taps"], t["taps2"], t["occ"], t["occ2"], t["out"]), MX),
        ("mx_grad.bwd", lambda t=mx: MXG.FilterInterpolationLayer_gpu_backward_mx(
            t["img"], t["flow"], t["taps"], t["gout"], g1(t), t["g2"], t["g3"]), MXG),
        ("blend_grad.bwd", lambda t=bw: BG.FilterInterpolationBlendLayer_gpu_backward(
            t["img"], t["flow"], t["taps"], t["occ"], t["gout"], t["g2"], t["g3"], t["gocc"]), BG),
    ]


name = {f32: "f32", f16: "f16", bf16: "bf16"}
if mode == "geometry":
    seen = set()
    for p in (f16, bf16):
        for fl in (f32, p):
            for go in (f32, p):
                for with_g1 in (True, False):
                    for label, f, mod in calls(2, p, fl, go, with_g1):
                        key = (label, p if label != "blend_grad.bwd" else None, fl if label != "blend_grad.bwd" else None,
                               go if label == "lp_grad.bwd" else None, with_g1 if label.endswith("bwd") and label != "blend_grad.bwd" else None)
                        if key in seen:
                            continue
                        seen.add(key)
                        torch.cuda.synchronize()
                        rc = f()
                        torch.cuda.synchronize()
                        print("CASE %-15s taps %-4s flow %-4s gout %-4s g1 %-5s rc %d path %s" % (
                            label, name[p], name[fl], name[go], with_g1, rc, mod.last_kernel_path()), flush=True)
else:
    label_run, out = sys.argv[3], sys.argv[4]
    res = {}
    for kind, n in (("batch0", 0), ("covered", 2)):
        for label, f, _mod in calls(n, f16, f32, f32, False):
            assert f() == 0, (kind, label)
            torch.cuda.synchronize()
            reps = []
            for _ in range(5):
                t0 = time.perf_counter()
                for _i in range(10000):
                    f()
                reps.append((time.perf_counter() - t0) / 10000 * 1e6)
                torch.cuda.synchronize()
            res["%s %s" % (kind, label)] = {"median_us": statistics.median(reps), "reps_us": reps}
            print("%-8s %-8s %-15s median %.3f us/call  (%s)" % (label_run, kind, label, statistics.median(reps),
                                                                " ".join("%.3f" % r for r in reps)), flush=True)
    json.dump(res, open(out, "w"), indent=1)
