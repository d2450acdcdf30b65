"""Generates tests/golden/reference_ve_64.npz, the fixture that stands for the REFERENCE class `networks.MEMC_Net_VE` in
tests/test_network_ve.py, so that the test runs wherever the repository does.  The class is imported from the reference
tree, unmodified, its custom operators provided by the CPU oracle (tests/_oracle_ops.py), its weights derived from the
parameter names (tests/_netutil.py).  Constructed as the reference's Vimeo demo does (demo_Vimeo_VE.py:40-42), with
training=False: the training constructor wants a weights file.  Recorded at 64 x 64, for batch 1 and batch 2 (at batch 1 a
swap of neighbour and batch element in the stacked rows n * B + b is invisible):

  ve/state_names, ve/state_shapes         the state dict's names and shapes, in order
  ve/b<B>/out/{rectified, flow, filter_mean}   the inference outputs `debug` returns, quantised as in
                                          make_golden_reference_class.py (integer multiples of a quarter of the tolerance)
  ve/b<B>/train_loss, ve/b<B>/grad_l1_module/<top-level module>
                                          one training step (the sum of the seven residuals' mean |.|) after
                                          `net.training = True` on the model in eval mode

Only names and quantised results are stored: no weights, and the reference source never enters the repository.
Run in the build container:  python tests/golden/make_golden_reference_ve.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _netutil      # noqa: E402
import _oracle_ops   # noqa: E402
from make_golden_reference_class import OUT_TOL_REL, state_layout   # noqa: E402

BATCHES = (1, 2)


def septuplet(seed, batch, h, w):
    """seven frames and a ground truth: (list of seven [B, 3, h, w], [B, 3, h, w]), a pure function of the arguments"""
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((batch, 3, h, w), generator=g) for _ in range(7)], torch.rand((batch, 3, h, w), generator=g)


def construct(cls):
    return cls(batch=1, channel=3, width=None, height=None, scale_num=1, scale_ratio=2, temporal=False, filter_size=4,
               save_which=1, debug=False, offset_scale=None, cuda_available=False, cuda_id=None, training=False)


def outputs(net, xs):
    """the reference's forward and, by its own methods, the flow and filter that forward returns under `debug` (whose
    prints index 0-dim tensors and fail under a current PyTorch)"""
    with torch.no_grad():
        rectified = net(xs)
        pairs = torch.cat([torch.cat((xs[3], xs[i]), dim=1) for i in range(7) if i != 3], dim=0)
        flow = net.forward_flownets(net.flownets, pairs)
        filt = net.forward_singlePath(net.initScaleNets_filter1,
                                      net.forward_singlePath(net.initScaleNets_filter, pairs, "filter"), name=None)
    return {"rectified": rectified, "flow": flow, "filter_mean": filt.mean(dim=1)}


def training_step(net, xs, y):
    """loss of one step with the sub-modules in eval mode (batch-norm statistics as loaded) and the class's own flag set"""
    net.zero_grad()
    net.training = True
    try:
        total = sum(l.abs().mean() for l in net(xs, y))
        total.backward()
    finally:
        net.training = False
    return float(total.detach())


def main():
    _oracle_ops.install()
    import torch.utils.model_zoo as model_zoo
    model_zoo.load_url = lambda *a, **k: {}            # the context network's ImageNet download: every weight is replaced
    ref = _netutil.import_reference_networks()
    torch.manual_seed(0)
    net = construct(ref.MEMC_Net_VE).eval()
    sd = net.state_dict()
    net.load_state_dict(_netutil.named_weights(sd))
    out = state_layout("ve/", sd)
    out["ve/n_params"] = np.int64(sum(p.numel() for p in net.parameters()))
    for batch in BATCHES:
        prefix = "ve/b%d/" % batch
        xs, y = septuplet(20 + batch, batch, 64, 64)
        for k, v in outputs(net, xs).items():
            v = v.numpy()
            tol = OUT_TOL_REL * max(1.0, float(np.abs(v).max()))
            out[prefix + "out_tol/" + k] = np.float64(tol)
            out[prefix + "out_step/" + k] = np.float64(tol / 4)
            out[prefix + "out/" + k] = _netutil.to_byte_planes(_netutil.quantize(v, tol / 4))
        out[prefix + "train_loss"] = np.float64(training_step(net, xs, y))
        out.update({prefix + "grad_l1_module/" + k: np.float64(v) for k, v in _netutil.grad_l1_by_module(net).items()})
    out["torch_version"] = np.array(torch.__version__)
    path = os.path.join(HERE, "reference_ve_64.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (os.path.basename(path), len(out), os.path.getsize(path)))
    print({k: float(v) for k, v in out.items() if "grad_l1_module" in k or "train_loss" in k})


if __name__ == "__main__":
    main()
