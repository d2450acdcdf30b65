"""tools/probes/tiled_backward_calls.py TREE -- one covered 2x3x24x72 call of each of the five tiled RGB backward entry
points (the warp's on half and mixed storage, the blend direction's on float32, mixed and half storage) per dtype
combination, the warp's with and without gradinput1, through the ctypes bindings of TREE: 37 kernels.  Run under
`rocprofv3 --kernel-trace --output-format csv` once per tree to compare kernel names, grids, workgroup sizes and LDS."""
import sys
sys.path.insert(0, sys.argv[1] + "/memc-net_amd")
import torch
import my_package._ext.my_lib_blend_grad as BG
import my_package._ext.my_lib_lp_blend_grad as LPBG
import my_package._ext.my_lib_lp_grad as LPG
import my_package._ext.my_lib_mx_blend_grad as MXBG
import my_package._ext.my_lib_mx_grad as MXG

dev, f32 = torch.device("cuda:0"), torch.float32
g = torch.Generator(device="cpu").manual_seed(5)


def r(c, dt, s=1.0):
    return (torch.rand((2, c, 24, 72), generator=g) * s).to(dt).to(dev)


def run(name, f, lib):
    code = f()
    torch.cuda.synchronize()
    print(name, code, lib.last_kernel_path(), flush=True)
    assert code == 0


x = [r(3, f32), r(2, f32, 3.0), r(16, f32), r(1, f32), r(3, f32)]
run("blend_grad", lambda: BG.FilterInterpolationBlendLayer_gpu_backward(*x, *(torch.empty_like(t) for t in x[1:4])), BG)
for t in (torch.float16, torch.bfloat16):
    for fl in (f32, t):
        x = [r(3, f32), r(2, fl, 3.0), r(16, t), r(1, t), r(3, f32)]
        run("mx_blend_grad %s %s" % (t, fl), lambda: MXBG.FilterInterpolationBlendLayer_gpu_backward_mx(
            *x, *(torch.empty_like(u) for u in x[1:4])), MXBG)
        for g1 in (True, False):
            y = [r(3, f32), r(2, fl, 3.0), r(16, t), r(3, f32)]
            run("mx_grad %s %s %s" % (t, fl, g1), lambda: MXG.FilterInterpolationLayer_gpu_backward_mx(
                *y, torch.zeros_like(y[0]) if g1 else None, torch.empty_like(y[1]), torch.empty_like(y[2])), MXG)
        for go in (f32, t):
            x = [r(3, t), r(2, fl, 3.0), r(16, t), r(1, t), r(3, go)]
            run("lp_blend_grad %s %s %s" % (t, fl, go), lambda: LPBG.FilterInterpolationBlendLayer_gpu_backward_lp(
                *x, *(torch.empty_like(u) for u in x[1:4])), LPBG)
            for g1 in (True, False):
                y = [r(3, t), r(2, fl, 3.0), r(16, t), r(3, go)]
                run("lp_grad %s %s %s %s" % (t, fl, go, g1), lambda: LPG.FilterInterpolationLayer_gpu_backward_lp(
                    *y, torch.zeros((2, 3, 24, 72), device=dev) if g1 else None, torch.empty_like(y[1]),
                    torch.empty_like(y[2])), LPG)
