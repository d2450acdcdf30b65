"""MEMC_Net_star in reduced precision, unmodified: cast to bfloat16, and in float32 under torch.autocast(float16).  Both
run inference end to end with finite outputs, and the adaptive warps inside go through libmemc_hip_lp.so (calls counted
through a wrapper on the binding)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _netutil      # noqa: E402

pytestmark = pytest.mark.gpu
SIZE = 128           # the smallest MEMC_Net_star shape of tests/test_gpu_network.py


@pytest.fixture(scope="module")
def star():
    _netutil.purge_networks()
    import networks
    m = networks.MEMC_Net_star(channel=3, filter_size=4, training=False)
    m.load_state_dict(_netutil.named_weights(m.state_dict()), strict=True)
    return m.cuda().eval()


@pytest.fixture
def lp_calls(monkeypatch):
    import my_package._ext.my_lib_lp as L
    calls = {}
    for name in ("FilterInterpolationLayer_gpu_forward_lp", "FilterInterpolationBlendLayer_gpu_forward_lp"):
        real = getattr(L, name)

        def counted(*args, _real=real, _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*args)

        monkeypatch.setattr(L, name, counted)
    return calls


def _finite(outs):
    return all(bool(torch.isfinite(t.float()).all()) for t in outs)


def test_bfloat16_model_runs_end_to_end(star, lp_calls):
    import copy
    m = copy.deepcopy(star).to(torch.bfloat16)
    x = _netutil.frames(7, 1, SIZE, SIZE).cuda().to(torch.bfloat16)
    with torch.no_grad():
        frames_out, flows, filters, occlusions = m(x)
    torch.cuda.synchronize()
    assert [t.dtype for t in frames_out] == [torch.bfloat16, torch.bfloat16]
    assert frames_out[1].shape == (1, 3, SIZE, SIZE) and _finite(frames_out)
    assert flows[0].dtype == torch.bfloat16 and filters[0].dtype == torch.bfloat16
    # the fused blend of the frames and the two context warps
    assert lp_calls.get("FilterInterpolationBlendLayer_gpu_forward_lp", 0) >= 1, lp_calls
    assert lp_calls.get("FilterInterpolationLayer_gpu_forward_lp", 0) >= 2, lp_calls


def test_autocast_float16_runs_end_to_end(star, lp_calls):
    x = _netutil.frames(7, 1, SIZE, SIZE).cuda()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        frames_out, flows, filters, occlusions = star(x)
    torch.cuda.synchronize()
    # the U-Nets return float16 under autocast; the frames themselves stay float32, so the blended frame (promoted payload)
    # is float32 and the context warps (float16 features and taps) run in float16
    assert all(t.dtype in (torch.float16, torch.float32) for t in frames_out)
    assert frames_out[1].shape == (1, 3, SIZE, SIZE) and _finite(frames_out)
    assert filters[0].dtype == torch.float16
    assert lp_calls.get("FilterInterpolationLayer_gpu_forward_lp", 0) >= 2, lp_calls
