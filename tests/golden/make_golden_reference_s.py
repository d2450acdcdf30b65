"""Generates tests/golden/reference_s.npz, the fixture that stands for the REFERENCE class `networks.MEMC_Net_s` in
tests/test_network_s.py, so that the test runs wherever the repository does.  The class is imported from the reference
tree, unmodified, its custom operators provided by the CPU oracle (tests/_oracle_ops.py), its weights derived from the
parameter names (tests/_netutil.py).  Constructed with training=False: the training constructor wants SPyNet's `.t7`
weights through torch.utils.serialization, which a current PyTorch no longer has.  Two stand-ins are installed here and
nowhere else: an empty `torch.utils.serialization` module (Network.py imports it at module scope) and `torch.Tensor.cuda`
as the identity (Network.py:125, :157 move the grid and the zero flow to the GPU unconditionally).

Recorded at two sizes, each for batch 1 and batch 2:
    64 x 64     two pyramid levels (32 x 32, 64 x 64)
    96 x 160    four levels (12 x 20, 24 x 40, 48 x 80, 96 x 160)

  s/state_names, s/state_shapes, s/n_params        the state dict's names and shapes, in order; the parameter count
  s/<H>x<W>/b<B>/out/{blended, rectified, flow0, flow1, occlusion0, occlusion1, filter0_mean, filter1_mean}
                                          the inference outputs, quantised as in make_golden_reference_class.py (integer
                                          multiples of a quarter of the tolerance).  An output of more than FULL elements is
                                          recorded at SAMPLE seeded positions and every plane's last row and column (sample_positions) instead of everywhere: with
                                          every output whole the fixture is 1.5 MB, beyond what a committed file may have
  s/<H>x<W>/b<B>/train_loss, .../grad_l1_module/<top-level module>
                                          one training step (the sum of the two residuals' mean |.|) after
                                          `net.training = True` on the model in eval mode

Only names and quantised results are stored: no weights, and the reference source never enters the repository.
Run in the build container:  python tests/golden/make_golden_reference_s.py
"""
import os
import sys
import types
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _netutil      # noqa: E402
import _oracle_ops   # noqa: E402

OUT_TOL_REL = 2e-5          # tests/test_network_s.py: outputs within 2e-5 * max(1, max |want|)
SIZES = ((64, 64), (96, 160))
BATCHES = (1, 2)
FULL, SAMPLE = 1 << 14, 1 << 13


def seed_of(h, w, batch):
    return 1000 * batch + h + w


def sample_positions(key, shape):
    """flat positions of the output `key` ([..., H, W]) that the fixture records: all of them up to FULL elements, else SAMPLE
    drawn with a seed derived from the key and, of every plane, the whole last row and last column (where an error of an
    odd level's padding or of an edge would sit); sorted, unique"""
    numel = int(np.prod(shape))
    if numel <= FULL:
        return np.arange(numel, dtype=np.int64)
    rng = np.random.default_rng(zlib.crc32(key.encode()))
    h, w = shape[-2:]
    flat = np.arange(numel, dtype=np.int64).reshape(-1, h, w)
    edges = np.concatenate([flat[:, h - 1, :].reshape(-1), flat[:, :, w - 1].reshape(-1)])
    return np.unique(np.concatenate([rng.integers(0, numel, SAMPLE, dtype=np.int64), edges]))


def outputs(net, x):
    with torch.no_grad():
        frames_out, flows, filters, occl = net(x)
    return {"blended": frames_out[0], "rectified": frames_out[1], "flow0": flows[0], "flow1": flows[1],
            "occlusion0": occl[0], "occlusion1": occl[1],
            "filter0_mean": filters[0].mean(dim=1), "filter1_mean": filters[1].mean(dim=1)}


def training_step(net, x3):
    """loss of one step with the sub-modules in eval mode (batch-norm statistics as loaded) and the class's own flag set"""
    net.zero_grad()
    net.training = True
    try:
        losses, _f, _k, _o = net(x3)
        total = sum(l.abs().mean() for l in losses)
        total.backward()
    finally:
        net.training = False
    return float(total.detach())


def install_shims():
    sys.modules.setdefault("torch.utils.serialization", types.ModuleType("torch.utils.serialization"))
    torch.utils.serialization = sys.modules["torch.utils.serialization"]
    torch.Tensor.cuda = lambda self, *a, **k: self


def main():
    import json
    _oracle_ops.install()
    install_shims()
    ref = _netutil.import_reference_networks()
    torch.manual_seed(0)
    net = ref.MEMC_Net_s(channel=3, filter_size=4, training=False).eval()
    sd = net.state_dict()
    net.load_state_dict(_netutil.named_weights(sd))
    out = {"s/state_names": np.array(list(sd.keys())),
           "s/state_shapes": np.array(json.dumps([list(t.shape) for t in sd.values()])),
           "s/n_params": np.int64(sum(p.numel() for p in net.parameters()))}
    for h, w in SIZES:
        for batch in BATCHES:
            prefix = "s/%dx%d/b%d/" % (h, w, batch)
            for k, v in outputs(net, _netutil.frames(seed_of(h, w, batch), batch, h, w)).items():
                shape, v = tuple(v.shape), v.numpy().reshape(-1)
                tol = OUT_TOL_REL * max(1.0, float(np.abs(v).max()))
                out[prefix + "out_tol/" + k] = np.float64(tol)
                out[prefix + "out_step/" + k] = np.float64(tol / 4)
                out[prefix + "out_numel/" + k] = np.int64(v.size)
                out[prefix + "out/" + k] = _netutil.to_byte_planes(
                    _netutil.quantize(v[sample_positions(prefix + k, shape)], tol / 4))
            out[prefix + "train_loss"] = np.float64(training_step(net, _netutil.training_frames(seed_of(h, w, batch), batch, h, w)))
            out.update({prefix + "grad_l1_module/" + k: np.float64(v) for k, v in _netutil.grad_l1_by_module(net).items()})
    out["torch_version"] = np.array(torch.__version__)
    path = os.path.join(HERE, "reference_s.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes; %d state entries, %d parameters" % (
        os.path.basename(path), len(out), os.path.getsize(path), len(sd), int(out["s/n_params"])))
    print({k: float(v) for k, v in out.items() if "grad_l1_module" in k or "train_loss" in k})


if __name__ == "__main__":
    main()
