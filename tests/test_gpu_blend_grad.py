"""The fused backward of the dual warp + occlusion blend for frames that are data (libmemc_hip_blend_grad.so,
include/memc_warp_blend_grad.h) and its use by FilterInterpolationBlendLayer.

Expected values are the CPU oracle's, as in test_gpu_parity.py::test_filter_interpolation_blend: the warp's backward on
gradoutput * occlusion for the flow and tap gradients, (gradoutput * warp forward) summed over the channels for the
occlusion gradient; the closeness rule is tests/_parity.py's, nothing else."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "memc-net_amd"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _lowp_paths as P                      # noqa: E402
import _netutil                              # noqa: E402
from _parity import RTOL, close              # noqa: E402
from tools import synth                      # noqa: E402

pytestmark = pytest.mark.gpu
PATH = "fi_blend_bwd:tiled_c3"
# the census table (bands in both directions, capped tiles, slow sites, split and mixed lanes, empty tiles, 4-column edge
# tiles, a ragged last tile row), the minimum width, and a wide row of mostly invalid sites
EXTRA = [(2, 37, 8, "smooth", 4.0, 31), (1, 20, 1280, "iid", 0.6 * 1280, 32)]
ABI_CASES = P.CASES + EXTRA
ABI_IDS = P.CASE_IDS + ["2x37x8-min-width", "1x20x1280-far"]


def G():
    import my_package._ext.my_lib_blend_grad as M
    return M


def BL():
    from my_package.functions import FilterInterpolationBlendLayer as M
    return M


def T(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def N(t):
    return t.detach().cpu().numpy()


def np_occlusion(rng, B, H, W):
    """uniform in [0, 1) with a block of exact zeros and a block of negative values"""
    o = rng.random((B, 1, H, W), dtype=np.float32)
    o[:, :, H // 4:H // 2, W // 4:W // 2] = 0.0
    o[:, :, H // 2:3 * H // 4, W // 2:3 * W // 4] *= -1.0
    return o


def direction(case):
    """(x, flow, taps, occ, gout) of one direction, numpy: signed gradoutput"""
    x, flow, filt, gout = P.case_inputs(case, 3)
    B, H, W = case[:3]
    return x, flow, filt, np_occlusion(np.random.default_rng(case[5] + 7), B, H, W), gout


def expected(oracle, x, flow, filt, occ, gout):
    """(flow, tap, occlusion) gradients of one direction from the oracle"""
    _g1, g2, g3 = oracle.filter_interpolation_backward(x, flow, filt, (gout * occ).astype(np.float32))
    g_occ = (gout * oracle.filter_interpolation_forward(x, flow, filt)).sum(axis=1, keepdims=True)
    return g2, g3, g_occ


def nan_like(t):
    return torch.full_like(t, float("nan"))


def fused(x, flow, filt, occ, gout, outs=None):
    """the C entry point into NaN-filled outputs: (status, gflow, gtaps, gocc)"""
    g2, g3, g4 = outs if outs is not None else (nan_like(flow), nan_like(filt), nan_like(occ))
    status = G().FilterInterpolationBlendLayer_gpu_backward(x, flow, filt, occ, gout, g2, g3, g4)
    torch.cuda.synchronize()
    return status, g2, g3, g4


def check_direction(oracle, got, host, label):
    for g, w, what in zip(got, expected(oracle, *host), ("grad flow", "grad taps", "grad occlusion")):
        assert not torch.isnan(g).any(), (label, what, "an element was not assigned")
        close(N(g), w, "%s %s" % (label, what), RTOL)


@pytest.mark.parametrize("case", ABI_CASES, ids=ABI_IDS)
def test_c_entry_point_on_every_in_kernel_path(oracle, case):
    host = direction(case)
    status, g2, g3, g4 = fused(*(T(a) for a in host))
    assert status == 0 and G().last_kernel_path() == PATH
    check_direction(oracle, (g2, g3, g4), host, "fused")


def test_census_of_the_added_cases():
    """what the two cases beyond the census table reach (counted on the CPU: tests/_lowp_paths.py)"""
    far = P.census(P.case_flow(EXTRA[1]))
    assert far["valid"] < 0.5 * far["sites"] and far["mixed_lanes"] > 0 and far["slow"] + far["split_lanes"] > 0, far
    narrow = P.census(P.case_flow(EXTRA[0]))
    assert narrow["tiles"] == 2 * 3 and narrow["ragged_cols"] == 8 and narrow["ragged_rows"] == 5, narrow


def test_strided_views_and_run_to_run(oracle):
    """Row-padded tensors (row stride W + 64) and an occlusion that is channel 1 of a [B, 2, H, W] tensor give the
    contiguous call's values bit for bit; so does a second identical call (no atomics)."""
    host = direction(P.CASES[1])
    dense = [T(a) for a in host]
    status, g2, g3, g4 = fused(*dense)
    assert status == 0
    check_direction(oracle, (g2, g3, g4), host, "dense")
    status, h2, h3, h4 = fused(*dense)
    assert status == 0
    assert torch.equal(g2, h2) and torch.equal(g3, h3) and torch.equal(g4, h4)
    # every tensor row-padded, outputs included (a gradient has its input's layout)
    pad = [synth.padded_planes(t) for t in dense]
    assert pad[0].stride(2) == host[0].shape[3] + 64 and not pad[0].is_contiguous()
    outs = tuple(synth.padded_planes(nan_like(t)) for t in (dense[1], dense[2], dense[3]))
    status, p2, p3, p4 = fused(*pad, outs=outs)
    assert status == 0 and G().last_kernel_path() == PATH
    assert torch.equal(g2, p2) and torch.equal(g3, p3) and torch.equal(g4, p4)
    # the occlusion (and its gradient) as channel 1 of a two-channel tensor
    two = torch.stack((torch.full_like(dense[3][:, 0], 9.0), dense[3][:, 0]), dim=1)
    gtwo = nan_like(two)
    status, v2, v3, v4 = fused(dense[0], dense[1], dense[2], two[:, 1:2], dense[4],
                               outs=(nan_like(dense[1]), nan_like(dense[2]), gtwo[:, 1:2]))
    assert status == 0
    assert torch.equal(g2, v2) and torch.equal(g3, v3) and torch.equal(g4, v4)
    assert torch.isnan(gtwo[:, 0]).all()                     # the neighbouring channel was not touched


class Spy:
    """replaces `owner.name` by a recorder that forwards to it"""

    def __init__(self, monkeypatch, owner, name):
        self.calls, self.returns = 0, []
        real = getattr(owner, name)

        def wrapped(*a, **k):
            self.calls += 1
            r = real(*a, **k)
            self.returns.append(r)
            return r
        monkeypatch.setattr(owner, name, wrapped)


def spies(monkeypatch):
    import my_package._ext.my_lib as my_lib
    return (Spy(monkeypatch, my_lib, "FilterInterpolationLayer_gpu_forward"),
            Spy(monkeypatch, my_lib, "FilterInterpolationLayer_gpu_backward"),
            Spy(monkeypatch, G(), "FilterInterpolationBlendLayer_gpu_backward"))


def blend_inputs(shape, seed, kind="smooth", sigma=None):
    """host dict of the blend's eight inputs + gradoutput"""
    B, C, H, W = shape
    h = {}
    for d, (x, f, k, o) in enumerate((("x0", "f0", "k0", "o0"), ("x2", "f1", "k1", "o1"))):
        rng = np.random.default_rng(seed + 100 * d)
        h[f] = synth.np_flow(rng, B, H, W, kind, sigma)
        h[x], h[k] = synth.np_image(rng, B, C, H, W), synth.np_filter(rng, B, H, W)
        h[o] = np_occlusion(rng, B, H, W)
    h["gout"] = np.random.default_rng(seed + 7).standard_normal((B, C, H, W)).astype(np.float32)
    return h


NAMES = ("x0", "x2", "f0", "f1", "k0", "k1", "o0", "o1")


def run_module(h, with_grad):
    from my_package.modules.FilterInterpolationBlendModule import FilterInterpolationBlendModule
    t = {n: T(h[n], n in with_grad) for n in NAMES}
    out = FilterInterpolationBlendModule()(*[t[n] for n in NAMES])
    return t, out


def check_module_grads(oracle, t, h, images=()):
    for x, f, k, o in (("x0", "f0", "k0", "o0"), ("x2", "f1", "k1", "o1")):
        g1, g2, g3 = oracle.filter_interpolation_backward(h[x], h[f], h[k], (h["gout"] * h[o]).astype(np.float32))
        w = oracle.filter_interpolation_forward(h[x], h[f], h[k])
        if x in images:
            close(N(t[x].grad), g1, "grad " + x, RTOL)
        else:
            assert t[x].grad is None
        close(N(t[f].grad), g2, "grad " + f, RTOL)
        close(N(t[k].grad), g3, "grad " + k, RTOL)
        close(N(t[o].grad), (h["gout"] * w).sum(axis=1, keepdims=True), "grad " + o, RTOL)


@pytest.mark.parametrize("shape", [(2, 3, 40, 64), (1, 3, 96, 256)], ids=["2x3x40x64", "1x3x96x256"])
def test_the_layer_takes_the_fused_route(oracle, monkeypatch, shape):
    h = blend_inputs(shape, 41)
    t, out = run_module(h, NAMES[2:])
    fwd, bwd, new = spies(monkeypatch)
    out.backward(T(h["gout"]))
    torch.cuda.synchronize()
    assert fwd.calls == 0 and bwd.calls == 0, (fwd.calls, bwd.calls)
    assert new.calls == 2 and new.returns == [0, 0], (new.calls, new.returns)
    check_module_grads(oracle, t, h)


def test_a_direction_whose_image_needs_a_gradient_keeps_the_composition(oracle, monkeypatch):
    h = blend_inputs((2, 3, 40, 64), 43)
    t, out = run_module(h, ("x0",) + NAMES[2:])
    fwd, bwd, new = spies(monkeypatch)
    out.backward(T(h["gout"]))
    torch.cuda.synchronize()
    assert fwd.calls == 1 and bwd.calls == 1, (fwd.calls, bwd.calls)          # direction 0: composed
    assert new.calls == 1 and new.returns == [0], (new.calls, new.returns)     # direction 1: fused
    check_module_grads(oracle, t, h, images=("x0",))


@pytest.mark.parametrize("shape", [(2, 3, 24, 23), (2, 5, 24, 32), (2, 3, 24, 4)], ids=["W23", "C5", "W4"])
def test_uncovered_calls_keep_the_old_route(oracle, monkeypatch, shape):
    """A ragged width, five channels, a width below 8: the new entry point is not called or returns 1, and the gradients
    are the per-direction composition's, bit for bit (the image gradient apart: it takes atomics)."""
    h = blend_inputs(shape, 47)
    t, out = run_module(h, NAMES[2:])
    fwd, bwd, new = spies(monkeypatch)
    out.backward(T(h["gout"]))
    torch.cuda.synchronize()
    assert all(r == 1 for r in new.returns), new.returns
    assert bwd.calls == 2
    # the backward function itself, asked for no image gradient: declines, composes
    saved = tuple(T(h[n]) for n in NAMES)
    gout = T(h["gout"])
    got = BL()._blend_backward(saved, gout, needs_image_grad=(False, False))
    assert new.returns and all(r == 1 for r in new.returns), new.returns
    for d in (0, 1):
        x, f, k, o = (saved[d], saved[2 + d], saved[4 + d], saved[6 + d])
        _gx, gf, gk, go = BL()._direction_backward(x, f, k, o, gout)
        assert torch.equal(got[2 + d], gf) and torch.equal(got[4 + d], gk) and torch.equal(got[6 + d], go)
        if shape[1] == 3 and shape[3] % 4 == 0:                  # the layer's own backward reached the same composition
            assert torch.equal(t[NAMES[2 + d]].grad, gf) and torch.equal(t[NAMES[4 + d]].grad, gk)
            assert torch.equal(t[NAMES[6 + d]].grad, go)
    check_module_grads(oracle, t, h)


def test_fused_against_composed():
    """The fused kernel and the per-direction composition on the GPU agree under the closeness rule.  They are NOT bit
    for bit: the composition rounds gradoutput * occlusion to fp32 before the warp's backward multiplies it with the
    pixels, the fused kernel multiplies by the occlusion last; the occlusion gradient is summed per tap there and per
    channel here."""
    h = blend_inputs((2, 3, 64, 256), 53, "iid", 20.0)
    x, f, k, o, gout = (T(h[n]) for n in ("x0", "f0", "k0", "o0", "gout"))
    status, g2, g3, g4 = fused(x, f, k, o, gout)
    assert status == 0
    _gx, c2, c3, c4 = BL()._direction_backward(x, f, k, o, gout)
    torch.cuda.synchronize()
    close(N(g2), N(c2), "fused vs composed grad flow", RTOL)
    close(N(g3), N(c3), "fused vs composed grad taps", RTOL)
    close(N(g4), N(c4), "fused vs composed grad occlusion", RTOL)


def test_a_training_step_runs_on_the_fused_backward(monkeypatch):
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    _netutil.purge_networks()
    import networks
    assert "memc-net_amd" in networks.__file__
    net = networks.MEMC_Net_star(channel=3, filter_size=4, training=True)
    net.load_state_dict(_netutil.named_weights(net.state_dict()), strict=True)
    net = net.cuda().train()
    losses, _f, _k, _o = net(_netutil.training_frames(5, 1, 128, 128).cuda())
    total = sum(l.abs().mean() for l in losses)
    new = Spy(monkeypatch, G(), "FilterInterpolationBlendLayer_gpu_backward")
    composed = Spy(monkeypatch, BL(), "_direction_backward")
    total.backward()
    torch.cuda.synchronize()
    assert new.calls >= 1 and all(r == 0 for r in new.returns), (new.calls, new.returns)
    assert composed.calls == 0
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
