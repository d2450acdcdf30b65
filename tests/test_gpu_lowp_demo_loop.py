"""The HD demo loop (networks/yuv_io.py, gpu_io=True) around the real MEMC_Net in reduced precision: a model cast to bfloat16
fed by libmemc_hip_video_lp.so, and the float32 model inside torch.autocast (bfloat16, float16) fed by libmemc_hip_video.so;
and tools/demo_hd720p.py --precision.

What is asserted is the plumbing: the planes' dtype and the autocast state the model saw, that the blend really ran in the
half (cast) or the mixed (autocast) library, the file's size and its two pass-through frames, byte for byte those of a
float32 run.  The interpolated frames are NOT held to the float32 run's under a bound: MIOpen's layers are not
reproducible between precisions, the weights are the untrained initial ones, and the operators' values are pinned call by
call in tests/test_gpu_lowp_network_calls.py.  The mean absolute luma difference to the float32 run is printed.
(A float16 cast is left to the stub models of tests/test_gpu_video_lp.py: with untrained weights its dense layers may
overflow, which would test MIOpen.)"""
import gc
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _netutil      # noqa: E402

pytestmark = pytest.mark.gpu

H = W = 64           # pads to 128 x 128
FRAMES, LAST = 5, 3


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """(networks, the float32 MEMC_Net at its initial weights, the clip's path, the float32 run's file and scores).
    The module leaves the process as it found it, as far as it can: the generators' states are restored after the model is
    built, and the model and the blocks the caching allocator holds for it are given back when the module is done.  (The
    suite's exact comparisons of two runs of one kernel whose sum order depends on wave timing, such as
    tests/test_gpu_lowp_parity.py's many-channel image gradient, passed or failed with what this module left behind.)"""
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    _netutil.purge_networks()
    import networks
    assert "memc-net_amd" in networks.__file__
    assert networks.pad_amounts(H, W) == (32, 32, 32, 32)
    with torch.random.fork_rng():
        torch.manual_seed(19)
        net = networks.MEMC_Net(channel=3, filter_size=4, training=False).cuda().eval()
    tmp = tmp_path_factory.mktemp("lowp_loop")
    src = str(tmp / "clip.yuv")
    rng = np.random.default_rng(19)
    wr = networks.Yuv420Writer(src)
    for _ in range(FRAMES):
        wr.write(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    wr.close()
    dst = str(tmp / "fp32.yuv")
    scores = networks.interpolate_yuv_sequence(net, src, dst, H, W, torch.device("cuda", 0), last=LAST, gpu_io=True)
    state = [networks, net, src, np.fromfile(dst, dtype=np.uint8).reshape(4, -1), scores]
    yield state
    state.clear()
    del net
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def run_mode(world, tmp_path, model, expect_dtype, expect_autocast, **kw):
    networks, _net, src, base, base_scores = world
    seen = []

    def hook(_module, args):
        seen.append((args[0].dtype, tuple(args[0].shape), torch.is_autocast_enabled("cuda"),
                     torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else None))
    handle = model.register_forward_pre_hook(hook)
    dst = str(tmp_path / "out.yuv")
    try:
        scores = networks.interpolate_yuv_sequence(model, src, dst, H, W, torch.device("cuda", 0), last=LAST, gpu_io=True, **kw)
    finally:
        handle.remove()
    torch.cuda.synchronize()
    assert [s[0] for s in scores] == [s[0] for s in base_scores] == [1, 3]
    assert os.path.getsize(dst) == 4 * (H * W * 3 // 2)
    out = np.fromfile(dst, dtype=np.uint8).reshape(4, -1)
    assert np.array_equal(out[0], base[0]) and np.array_equal(out[2], base[2])      # frames 0 and 2 pass through
    assert seen == [(expect_dtype, (2, 1, 3, 128, 128), expect_autocast is not None, expect_autocast)] * 2
    assert all(np.isfinite(s[1]) and np.isfinite(s[2]) for s in scores)
    luma = np.abs(out[1::2, :H * W].astype(np.int16) - base[1::2, :H * W]).mean(axis=1)
    print("%s: mean |dY| of the two interpolated frames to the float32 run's: %s; scores %s, float32 scores %s" % (
        kw, ["%.4f" % v for v in luma], scores, base_scores))
    return scores


def test_bf16_cast(world, tmp_path):
    import copy
    import my_package._ext.my_lib_lp as lp
    model = copy.deepcopy(world[1]).to(torch.bfloat16)
    run_mode(world, tmp_path, model, torch.bfloat16, None, dtype=torch.bfloat16)
    assert lp.last_kernel_path() == "fi_blend_lp:tiled_c3"
    del model


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_autocast(world, tmp_path, dtype):
    import my_package._ext.my_lib_mx as mx
    run_mode(world, tmp_path, world[1], torch.float32, dtype, autocast=dtype)
    assert mx.last_kernel_path() == "fi_blend_mx:tiled_c3"
    assert all(p.dtype == torch.float32 for p in world[1].parameters())           # the model itself stays float32


def test_hd_demo_command_line_in_bf16(world, tmp_path, capsys):
    """tools/demo_hd720p.py --precision bf16 --gpu-io on the same clip: it prints its scores and writes the file"""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import importlib
    demo = importlib.import_module("demo_hd720p")
    src, dst = world[2], str(tmp_path / "out.yuv")
    demo.main(["--input", src, "--output", dst, "--height", str(H), "--width", str(W), "--model", "MEMC_Net",
               "--last", str(LAST), "--precision", "bf16", "--gpu-io"])
    out = capsys.readouterr().out
    assert "frame    1" in out and "frame    3" in out and "average over 2 interpolated frames" in out
    assert os.path.getsize(dst) == 4 * (H * W * 3 // 2)
    got = np.fromfile(dst, dtype=np.uint8).reshape(4, -1)
    assert np.array_equal(got[0], world[3][0]) and np.array_equal(got[2], world[3][2])
    with pytest.raises(SystemExit):                                # argparse refuses what is not a mode
        demo.main(["--input", src, "--output", dst, "--precision", "fp8"])
