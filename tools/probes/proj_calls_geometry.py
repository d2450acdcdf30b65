#!/usr/bin/env python
"""tools/probes/proj_calls_geometry.py -- which kernels, on which grid, a call of the projection and of the many-channel
backward launchers queues: one call per case through the MEASUREMENT build of a tree, for a rocprofv3 kernel trace, and
the comparison of two such traces (a host-side change must leave every case as it was).

    rocprofv3 --kernel-trace -f csv -d <dir> -o a -- python tools/probes/proj_calls_geometry.py <tree>/memc-net_amd <a_cases.txt>
    python tools/probes/proj_calls_geometry.py --compare <a_kernel_trace.csv> <a_cases.txt> <b_kernel_trace.csv> <b_cases.txt>

Cases: (Depth)FlowProjection forward, fillhole 0 / 1, on 2x100x196, 2x70x198 (ragged width) and 2x20x6 (scalar kernels)
under every projection variant the parity tests force and the timing / trace arms; their backward under bl_cap x walk;
the FilterInterpolation / InterpolationCh backward on 2x5x40x72 and 2x4x40x70, the bilinear one with and without
bl_bwd_direct, and bl_cap 5 at C = 3.  The arms are launched for their trace only: several return wrong results by
design, no output is looked at.  One ATen kernel is queued in front of every case; the comparison cuts the trace there.
The trace's LDS column is what it is (static, or static + dynamic: the tool's version decides); per case the kernel names
in order, grid, workgroup size and that column must be equal."""
import csv
import ctypes
import os
import re
import sys

VARIANTS = sorted({-1, -43, 1, 0, 100, 104, 110, 112, -40, 400, 404, 412, 130, 142, 154, 160, 164, -10,       # test_gpu_parity.py,
                   -9, 114, 414, 134, 140,                                                                    # its pans
                   -5, -8, -20, -21, -22, -23, -24, -25, -26, -29, -30, -31, -41, -42,
                   -46, -47, -48, -49, -50, -51, -52, -53, -54, 2, 3, 200, 251})
SHAPES = [(2, 100, 196), (2, 70, 198), (2, 20, 6)]


def run(pkg_dir, cases_path):
    tree = os.path.dirname(os.path.abspath(pkg_dir))
    sys.path[:0] = [tree, os.path.abspath(pkg_dir)]
    import torch
    from tools import measure as M

    dev = torch.device("cuda:0")
    ML, labels = M.bound(), []
    torch.manual_seed(5)
    trace = torch.zeros(1 << 16, dtype=torch.int64, device=dev)     # the trace arms' slots: 16 per workgroup, < 4096 workgroups here
    setter = M.lib().memc_debug_set_trace_buffer_proj
    setter.argtypes = [ctypes.c_void_p]
    assert setter(ctypes.c_void_p(trace.data_ptr())) == 0
    sentinel = torch.zeros(64, device=dev)

    def case(label, fn):
        labels.append(label)
        sentinel.add_(1)
        assert fn() in (0, -1), label                 # (-1: an arm that does not exist at this geometry -- on both trees)

    proj = []
    for b, h, w in SHAPES:
        f = (torch.randn(b, 2, h, w, device=dev) * 3).contiguous()
        d = torch.rand(b, 1, h, w, device=dev) + 0.5
        proj.append((f, d, torch.zeros_like(d), torch.zeros_like(f), torch.rand_like(f), torch.zeros_like(f), torch.zeros_like(d)))
    many = []
    for b, c, h, w in ((2, 5, 40, 72), (2, 4, 40, 70), (2, 3, 40, 72)):
        x, fl = torch.rand(b, c, h, w, device=dev), (torch.randn(b, 2, h, w, device=dev) * 3).contiguous()
        k, g = torch.rand(b, 16, h, w, device=dev), torch.rand(b, c, h, w, device=dev)
        many.append((x, fl, k, g, torch.zeros_like(x), torch.zeros_like(fl), torch.zeros_like(k)))
    torch.cuda.synchronize()
    try:
        for f, d, cnt, out, go, g1, g2 in proj:
            shape = "x".join(map(str, f.shape[:1] + f.shape[2:]))
            for v in VARIANTS:
                M.set_variant("projection", v)
                for fh in (0, 1):
                    case("proj_fwd %s variant %d fill %d" % (shape, v, fh),
                         lambda: ML.FlowProjectionLayer_gpu_forward(f, cnt, out, fh))
                    case("dproj_fwd %s variant %d fill %d" % (shape, v, fh),
                         lambda: ML.DepthFlowProjectionLayer_gpu_forward(f, d, cnt, out, fh))
            M.set_variant("projection", -1)
        for f, d, cnt, out, go, g1, g2 in proj[:2]:
            shape = "x".join(map(str, f.shape[:1] + f.shape[2:]))
            ML.DepthFlowProjectionLayer_gpu_forward(f, d, cnt, out, 1)       # (count and output for the backward; no case)
            for cap in (-1, 0, 2):
                for walk in (-1, 4):
                    M.set_variant("bl_cap", cap)
                    M.set_variant("walk", walk)
                    case("proj_bwd %s bl_cap %d walk %d" % (shape, cap, walk),
                         lambda: ML.FlowProjectionLayer_gpu_backward(f, cnt, go, g1))
                    case("dproj_bwd %s bl_cap %d walk %d" % (shape, cap, walk),
                         lambda: ML.DepthFlowProjectionLayer_gpu_backward(f, d, cnt, out, go, g1, g2))
            M.set_variant("bl_cap", -1)
            M.set_variant("walk", -1)
        for x, fl, k, g, g1, g2, g3 in many[:2]:
            shape = "x".join(map(str, x.shape))
            case("fi_bwd %s" % shape, lambda: ML.FilterInterpolationLayer_gpu_backward(x, fl, k, g, g1, g2, g3))
            for direct in (0, 1):
                M.set_variant("bl_bwd_direct", direct)
                case("bl_bwd %s direct %d" % (shape, direct), lambda: ML.InterpolationChLayer_gpu_backward(x, fl, g, g1, g2))
            M.set_variant("bl_bwd_direct", 0)
        x, fl, k, g, g1, g2, g3 = many[2]
        M.set_variant("bl_cap", 5)
        case("bl_bwd %s bl_cap 5" % "x".join(map(str, x.shape)), lambda: ML.InterpolationLayer_gpu_backward(x, fl, g, g1, g2))
    finally:
        M.reset()
    torch.cuda.synchronize()
    with open(cases_path, "w") as fh_:
        fh_.write("\n".join(labels) + "\n")
    print("%d cases through %s" % (len(labels), M.MEASURE_LIB))


def segments(trace_csv, cases_path):
    """[(label, [(kernel, grid, workgroup, lds)])]: the trace in dispatch order, cut at the ATen kernels"""
    labels = open(cases_path).read().split("\n")[:-1]
    rows = list(csv.DictReader(open(trace_csv)))
    col = lambda *alts: next(c for c in rows[0] if c.lower() in alts)
    name, lds, disp = col("kernel_name"), col("lds_block_size", "group_segment_size", "lds_block_size_v"), col("dispatch_id")
    rows.sort(key=lambda r: int(r[disp]))
    dims = lambda r, what: "x".join(r["%s_%s" % (what, a)] for a in "XYZ")
    short = lambda n: re.sub(r"\(.*$", "", n.replace("void ", "").replace("memc::", "").replace(" [clone .kd]", ""))
    segs = [[]]
    for r in rows:
        if "at::native" in r[name]:
            segs.append([])
        else:
            segs[-1].append((short(r[name]), dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), r[lds]))
    assert len(segs) > len(labels), (len(segs), len(labels))
    return list(zip(labels, segs[-len(labels):]))


def compare(a_csv, a_cases, b_csv, b_cases):
    a, b = segments(a_csv, a_cases), segments(b_csv, b_cases)
    assert [l for l, _ in a] == [l for l, _ in b], "the two runs made different cases"
    differ = 0
    for (label, ka), (_l, kb) in zip(a, b):
        differ += ka != kb
        print("%-44s %-9s %s" % (label, "same" if ka == kb else "DIFFERENT", "  ".join("%s [%s / %s / %s]" % k for k in ka)))
        if ka != kb:
            print("%-44s %-9s %s" % ("", "  new:", "  ".join("%s [%s / %s / %s]" % k for k in kb)))
    print("%d cases, %d kernels; kernel names in order, grid, workgroup size and LDS column: %s" % (
        len(a), sum(len(k) for _l, k in a), "all equal" if not differ else "%d cases DIFFER" % differ))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:]))
    assert len(sys.argv) == 3, __doc__
    run(sys.argv[1], sys.argv[2])
