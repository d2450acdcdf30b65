"""the build-owned `networks.MEMC_Net_star` (memc-net_amd/networks) against the
reference class.

CPU tests (this file, not gpu): the custom operators are provided by the oracle (tests/_oracle_ops.py) for BOTH
models, so what is compared is the network wiring, the state-dict layout and the dense layers.
  * against the committed vectors tests/golden/network_star_128.npz (made by make_golden_network.py from the
    reference class) -- always runs;
  * against the reference classes' state-dict layout, outputs and training-step gradients, recorded in
    tests/golden/reference_star_64.npz / reference_base_64.npz by make_golden_reference_class.py -- always runs.
The GPU test of the same model on the HIP operators is tests/test_gpu_network.py.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _netutil      # noqa: E402
import _oracle_ops   # noqa: E402

GOLD = os.path.join(HERE, "golden", "network_star_128.npz")


@pytest.fixture(autouse=True)
def _oracle_backed_ops():
    """`my_package` resolves to the oracle-backed stand-ins inside these tests only."""
    _oracle_ops.install()
    yield
    _oracle_ops.uninstall()


def _outputs(net, x):
    with torch.no_grad():
        frames_out, flows, filters, occl = net(x)
    return {"blended": frames_out[0], "rectified": frames_out[1], "flow0": flows[0], "flow1": flows[1],
            "occlusion0": occl[0], "occlusion1": occl[1],
            "filter0_mean": filters[0].mean(dim=1), "filter1_mean": filters[1].mean(dim=1)}


def _own_model(name="MEMC_Net_star"):
    _netutil.purge_networks()
    import networks                                        # memc-net_amd/networks (conftest puts it on the path)
    assert "memc-net_amd" in networks.__file__
    return getattr(networks, name)(channel=3, filter_size=4, training=False).eval()


def test_own_model_matches_reference_vectors():
    gold = np.load(GOLD)
    net = _own_model()
    assert sum(p.numel() for p in net.parameters()) == int(gold["n_params"]) == 70312501
    net.load_state_dict(_netutil.named_weights(net.state_dict()), strict=True)
    got = _outputs(net, _netutil.frames(7, 1, 128, 128))
    for k, v in got.items():
        ref = gold[k]
        tol = 2e-5 * max(1.0, float(np.abs(ref).max()))
        assert np.abs(v.numpy() - ref).max() <= tol, k


def test_own_base_model_matches_reference_vectors():
    gold = np.load(os.path.join(HERE, "golden", "network_base_64.npz"))
    net = _own_model("MEMC_Net")
    assert sum(p.numel() for p in net.parameters()) == int(gold["n_params"])
    net.load_state_dict(_netutil.named_weights(net.state_dict()), strict=True)
    got = _outputs(net, _netutil.frames(7, 1, 64, 64))
    for k, v in got.items():
        ref = gold[k]
        assert np.abs(v.numpy() - ref).max() <= 2e-5 * max(1.0, float(np.abs(ref).max())), k


def test_own_model_training_step_matches_reference_fingerprint():
    gold = np.load(GOLD)
    net = _own_model()
    net.load_state_dict(_netutil.named_weights(net.state_dict()), strict=True)
    net.train()
    losses, _f, _k, _o = net(_netutil.training_frames(5, 1, 128, 128))
    total = sum(l.abs().mean() for l in losses)
    total.backward()
    assert abs(float(total) - float(gold["train_loss"])) <= 1e-5 * float(gold["train_loss"])
    got = _netutil.grad_l1_by_module(net)
    want = {k[len("grad_l1/"):]: float(gold[k]) for k in gold.files if k.startswith("grad_l1/")}
    assert sorted(got) == sorted(want)                    # ctxNet gets no gradient in either (detached warps)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-4 * want[k], k


_GOLD = {}


def _gold(cls):
    """tests/golden/reference_<cls>_64.npz (made by make_golden_reference_class.py from the reference class), as a dict."""
    if cls not in _GOLD:
        with np.load(os.path.join(HERE, "golden", "reference_%s_64.npz" % cls)) as f:
            _GOLD[cls] = {k: f[k] for k in f.files}
    return _GOLD[cls]


def _ref(key):
    return _gold(key.split("/")[0])[key]


def _assert_outputs_match_reference(prefix, got):
    """Every output within 2e-5 * max(1, max |want|) of the reference class's.  The fixture holds each output as integer
    multiples of a step of at most a quarter of that tolerance (|recorded - exact| <= step / 2), so the comparison with the
    recorded values allows tol - step / 2: a pass bounds the distance to the exact output by the full tolerance."""
    gold = _gold(prefix.rstrip("/"))
    assert sorted(got) == sorted(k[len(prefix + "out/"):] for k in gold if k.startswith(prefix + "out/"))
    for k, v in got.items():
        tol, step = float(gold[prefix + "out_tol/" + k]), float(gold[prefix + "out_step/" + k])
        assert step <= tol / 4
        want = _netutil.dequantize(_netutil.from_byte_planes(gold[prefix + "out/" + k]), step)
        have = v.double().numpy().reshape(-1)
        assert have.shape == want.shape, k
        assert float(np.abs(have - want).max()) <= tol - step / 2, k


# Float32 gradients of a 70M-parameter network recomputed on another CPU (other SIMD kernels, other thread counts: other
# reduction orders in the dense layers) differ from the recorded ones by up to ~2.5e-4 of a tensor's largest |g| (element,
# max) and ~1.6e-4 of a module's sum |g|; in one process (the same CPU for both classes) by ~1e-7.  The gradient checks
# allow for the former; a 0.1 % error in one tensor's gradient still fails them.
GRAD_RTOL = 1e-3


def _assert_reference_state_layout(prefix, own_sd):
    """Same names in the same order and the same shapes as the reference class's state dict: a reference checkpoint loads
    as is."""
    assert list(own_sd.keys()) == [str(k) for k in _ref(prefix + "state_names")]
    assert [list(t.shape) for t in own_sd.values()] == json.loads(str(_ref(prefix + "state_shapes")))


def test_state_dict_and_outputs_match_reference_class():
    net = _own_model()
    own_sd = net.state_dict()
    _assert_reference_state_layout("star/", own_sd)
    net.load_state_dict(_netutil.named_weights(own_sd), strict=True)
    _assert_outputs_match_reference("star/", _outputs(net, _netutil.frames(11, 2, 64, 64)))


def test_training_mode_returns_reference_structure():
    net = _own_model()
    net.train()
    with torch.no_grad():
        net.load_state_dict(_netutil.named_weights(net.state_dict()))
        two = _netutil.frames(3, 1, 64, 64)
        x = torch.stack((two[0], 0.5 * (two[0] + two[1]), two[1]))            # (frame0, ground truth, frame2)
        losses, flows, filters, occl = net(x)
        with pytest.raises(AssertionError):
            net(two)                                                           # training wants three frames
    # reference MEMC_Net_star.py:163-170: residuals against the middle frame, and singly nested lists
    assert len(losses) == 2 and losses[0].shape == (1, 3, 64, 64)
    assert len(flows) == 1 and len(flows[0]) == 2 and flows[0][0].shape == (1, 2, 64, 64)
    assert len(filters) == 1 and filters[0][0].shape == (1, 16, 64, 64)
    assert len(occl) == 1 and occl[0][1].shape == (1, 1, 64, 64)


def test_training_step_gradients_match_reference_class():
    """One training step (Charbonnier-free: plain L1 of the two residuals) against the reference class's: the same loss
    and the same parameter gradients, i.e. the backward wiring (detached context warps, un-filled projection when
    gradients flow) is the reference's.  Per parameter tensor: the same set of tensors with a gradient, each gradient's
    max |g| and sum |g|, and its values at the recorded positions (a seeded sample plus the arg-max |g|; GRAD_RTOL)."""
    two = _netutil.frames(5, 1, 64, 64)
    x = torch.stack((two[0], 0.5 * (two[0] + two[1]), two[1]))
    net = _own_model()
    net.load_state_dict(_netutil.named_weights(net.state_dict()), strict=True)
    net.train()
    losses, _flows, _filters, _occl = net(x)
    total = sum(l.abs().mean() for l in losses)
    total.backward()
    got = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}

    want_loss = float(_ref("star/train_loss"))
    assert abs(float(total) - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    names = [str(k) for k in _ref("star/grad_names")]
    assert sorted(got) == sorted(names)
    values, used = _ref("star/grad_values"), 0
    for i, k in enumerate(names):
        g = got[k].detach().reshape(-1)
        want_max, step = float(_ref("star/grad_max")[i]), float(_ref("star/grad_step")[i])
        scale = max(1e-3, want_max)
        assert step <= GRAD_RTOL * scale / 4
        # the recorded positions (regenerated from the name and the reference's arg-max) and their values, recorded as
        # integer multiples of `step` (|recorded - exact| <= step / 2: allowed for below, so a pass bounds the distance to
        # the exact gradient by GRAD_RTOL * scale)
        idx = _netutil.grad_sample_positions(k, g.numel(), int(_ref("star/grad_argmax")[i]))
        want = _netutil.dequantize(values[used:used + len(idx)], step)
        used += len(idx)
        assert float(np.abs(g.double().numpy()[idx] - want).max()) <= GRAD_RTOL * scale - step / 2, k
        assert abs(float(g.abs().max()) - want_max) <= GRAD_RTOL * scale, k
        want_l1 = float(_ref("star/grad_l1")[i])
        assert abs(float(g.double().abs().sum()) - want_l1) <= GRAD_RTOL * max(want_l1, scale), k
    assert used == len(values)


def test_base_model_matches_reference_class():
    """MEMC_Net (no context branch, plain conv rectifier): state dict, inference outputs and one training
    step's gradients against the reference class."""
    _netutil.purge_networks()
    import networks
    net = networks.MEMC_Net(channel=3, filter_size=4, training=False).eval()
    own_sd = net.state_dict()
    _assert_reference_state_layout("base/", own_sd)
    net.load_state_dict(_netutil.named_weights(own_sd), strict=True)
    _assert_outputs_match_reference("base/", _outputs(net, _netutil.frames(13, 1, 64, 64)))
    net.train()
    losses, _f, _k, _o = net(_netutil.training_frames(5, 1, 64, 64))
    total = sum(l.abs().mean() for l in losses)
    total.backward()
    got_loss, got_g = float(total.detach()), _netutil.grad_l1_by_module(net)
    want_loss = float(_ref("base/train_loss"))
    want_g = {k[len("base/grad_l1_module/"):]: float(v) for k, v in _gold("base").items()
              if k.startswith("base/grad_l1_module/")}
    assert abs(got_loss - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
    assert sorted(got_g) == sorted(want_g)
    for k in want_g:
        assert abs(got_g[k] - want_g[k]) <= GRAD_RTOL * max(1e-6, want_g[k]), k


def test_demo_padding_rule():
    """demo_HD720p.py:88-106: pad up to the next multiple of 128, split floor / rest; 32 per side when already a
    multiple (values worked out from that arithmetic)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "inference", os.path.join(os.path.dirname(HERE), "memc-net_amd", "networks", "inference.py"))
    inf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inf)
    assert inf.pad_amounts(720, 1280) == (32, 32, 24, 24)          # 1280 = 10 * 128 -> 32 + 32; 720 -> 768
    assert inf.pad_amounts(1080, 1920) == (32, 32, 36, 36)         # 1080 -> 1152
    assert inf.pad_amounts(256, 448) == (32, 32, 32, 32)           # 448 -> 512; 256 is a multiple
    assert inf.pad_amounts(480, 640) == (32, 32, 16, 16)           # 640 = 5 * 128; 480 -> 512
    assert inf.pad_amounts(101, 203) == (26, 27, 13, 14)           # odd totals: floor first

    class Probe(torch.nn.Module):                                   # returns its padded first frame
        def forward(self, x):
            assert x.shape[-2] % 128 == 0 or x.shape[-2] - 64 > 0
            return [x[0], x[0] + 1.0], None, None, None
    f0 = torch.rand(2, 3, 101, 203)
    out = inf.interpolate_pairs(Probe(), f0, torch.rand(2, 3, 101, 203), which=0)
    assert torch.equal(out, f0)                                     # the crop undoes the padding exactly
