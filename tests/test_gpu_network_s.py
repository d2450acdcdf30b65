"""`networks.MEMC_Net_s` on the device, on the HIP operators: 64 x 64, batch 2, weights derived from the parameter names.

At each pyramid level the same (first, second, coarse) goes to `SPyNet.level_input` with `fused_level` True and False and
both 8-channel tensors are held to the operator rule of tests/test_gpu_spynet_level.py (tests/_spynet_spec.check_level).
Whole pyramids by the two routes are NOT compared bit for bit: MIOpen's convolutions need not repeat bits, and a level's
difference feeds the next.  Whole inferences by both routes are checked for shape and finiteness, their difference printed;
then one training step, and the still-image demo's command line with --model MEMC_Net_s.
"""
import os
import sys

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd"), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _netutil                            # noqa: E402
import _spynet_spec as S                   # noqa: E402

pytestmark = pytest.mark.gpu
B, H, W = 2, 64, 64

_MODEL = {}


def model():
    """one model for the module (its weights are never changed: the training step only accumulates gradients)"""
    if not _MODEL:
        import networks
        assert "memc-net_amd" in networks.__file__
        net = networks.MEMC_Net_s(channel=3, filter_size=4, training=False).eval()
        net.load_state_dict(_netutil.named_weights(net.state_dict()), strict=True, warn_align_corners=False)
        _MODEL["net"] = net.cuda()
    return _MODEL["net"]


def LIB():
    import my_package._ext.my_lib_spynet as M
    return M


def test_every_level_input_by_both_routes():
    net = model()
    spy = net.flownets
    x = _netutil.frames(31, B, H, W).cuda()
    flags = (int(spy.align_upsample), int(spy.align_sample))
    from networks._spynet import level_input_composed
    with torch.no_grad():
        first, second = spy.pyramid(x[0], x[1])
        assert [tuple(t.shape[2:]) for t in first] == [(32, 32), (64, 64)]
        flow = first[0].new_zeros((B, 2, 16, 16))
        for level in range(len(first)):
            case = tuple(t.cpu().numpy() for t in (first[level], second[level], flow))
            spy.fused_level = True
            fused = spy.level_input(first[level], second[level], flow)
            assert LIB().last_kernel_path() == "spynet_level:quad"
            spy.fused_level = False
            composed = spy.level_input(first[level], second[level], flow)
            assert fused.shape == composed.shape == (B, 8) + tuple(first[level].shape[2:])
            # with `fused_level` off the layer ran its own torch expression; the network's copy of it (reached only on a
            # my_package without the extension) is the same rule
            assert torch.equal(composed, level_input_composed(first[level], second[level], flow, *(bool(f) for f in flags)))
            for name, t in (("fused", fused), ("composed", composed)):
                e = S.check_level(t.cpu().numpy(), case, flags, "MEMC_Net_s level %d, %s" % (level, name))
                print("level", level, name, "worst error: up %.3g, warp %.3g" % e)
            print("level", level, "max |fused - composed| = %.3g" % float((fused - composed).abs().max()))
            flow = spy.moduleBasic[level](fused) + fused[:, 6:8]
            assert float(flow.abs().max()) > 0             # the next level gets a flow that moves things


def test_whole_inference_by_both_routes():
    net = model()
    x = _netutil.frames(32, B, H, W).cuda()
    outs = {}
    with torch.no_grad():
        for fused in (True, False):
            net.flownets.fused_level = fused
            frames_out, flows, filters, occl = net(x)
            assert len(frames_out) == 2 and all(t.shape == (B, 3, H, W) for t in frames_out)
            assert all(t.shape == (B, 2, H, W) for t in flows) and all(t.shape == (B, 16, H, W) for t in filters)
            assert all(t.shape == (B, 1, H, W) for t in occl)
            for t in tuple(frames_out) + tuple(flows) + tuple(filters):
                assert bool(torch.isfinite(t).all())
            outs[fused] = (frames_out[1], flows[0])
    print("rectified: max |fused - composed| = %.3g; flow: %.3g" % (
        float((outs[True][0] - outs[False][0]).abs().max()), float((outs[True][1] - outs[False][1]).abs().max())))


def test_one_training_step(monkeypatch):
    """There is no backward kernel, so a level with an input that wants a gradient keeps torch's autograd.  The coarsest
    level has none -- its frames are data, its coarse flow is zeros -- so it, and it alone, still takes the kernel (its
    output is constant with respect to the parameters); the next level's coarse flow comes out of moduleBasic[0] and wants
    one.  Every call that reaches the binding is recorded, and both levels' convolutions must carry a gradient."""
    net = model()
    net.zero_grad()
    net.flownets.fused_level = True
    x3 = _netutil.training_frames(33, B, H, W).cuda()
    with torch.no_grad():                                  # leave the OTHER family's name behind, whatever ran before
        net.flownets.level_input(*(torch.from_numpy(a).cuda() for a in S.ordinary_case((2, 26, 42))))
    assert LIB().last_kernel_path() == "spynet_level:direct"
    reached, entry = [], LIB().SpyNetLevelLayer_gpu_forward

    def recording(first, second, coarse, out, *flags):
        reached.append((tuple(first.shape[2:]), any(t.requires_grad for t in (first, second, coarse)),
                        float(coarse.abs().max())))
        return entry(first, second, coarse, out, *flags)
    monkeypatch.setattr(LIB(), "SpyNetLevelLayer_gpu_forward", recording)
    net.training = True                                    # the class's own flag; the sub-modules stay in eval mode
    try:
        losses, flows, filters, occl = net(x3)
        total = sum(l.abs().mean() for l in losses)
        total.backward()
    finally:
        net.training = False
    # two directions, each with one 32 x 32 level whose inputs want no gradient and whose coarse flow is zero; the 64 x 64
    # levels did not reach the library
    assert reached == [((32, 32), False, 0.0)] * 2, reached
    assert LIB().last_kernel_path() == "spynet_level:quad"
    assert len(losses) == 2 and bool(torch.isfinite(total))
    got = _netutil.grad_l1_by_module(net)
    assert sorted(got) == ["flownets", "initScaleNets_filter", "initScaleNets_filter1", "initScaleNets_filter2", "rectifyNet"]
    assert all(np.isfinite(v) and v > 0 for v in got.values()), got
    # per level: both used stacks carry a gradient on every parameter, the four unused ones none
    for level, stack in enumerate(net.flownets.moduleBasic):
        for name, p in stack.named_parameters():
            if level < 2:
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, (level, name)
            else:
                assert p.grad is None, (level, name)
    net.zero_grad()


def test_still_image_demo_command_line(tmp_path, capsys):
    """tools/demo_middlebury.py --model MEMC_Net_s on the scene tree of tests/test_gpu_network.py's command-line test"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import importlib
    demo = importlib.import_module("demo_middlebury")
    import networks
    rng = np.random.default_rng(9)
    data, gt, out = tmp_path / "data", tmp_path / "gt", tmp_path / "out"
    for scene, (h, w) in (("Alpha", (128, 192)), ("Beta", (128, 192))):
        os.makedirs(str(data / scene))
        os.makedirs(str(gt / scene))
        base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        networks.write_png(str(data / scene / "frame10.png"), base)
        networks.write_png(str(data / scene / "frame11.png"), np.roll(base, 2, axis=1))
        if scene == "Alpha":
            networks.write_png(str(gt / scene / "frame10i11.png"), np.roll(base, 1, axis=1))
    demo.main(["--data", str(data), "--gt", str(gt), "--output", str(out), "--model", "MEMC_Net_s"])
    text = capsys.readouterr().out
    assert "Alpha" in text and "interpolation error / PSNR" in text and "Beta" in text and "no ground truth" in text
    assert "for all 1 images" in text
    rec = networks.read_png(str(out / "Alpha" / "frame10i11.png"))
    assert rec.shape == (128, 192, 3) and rec.dtype == np.uint8
    assert networks.read_png(str(out / "Beta" / "frame10i11.png")).shape == (128, 192, 3)
