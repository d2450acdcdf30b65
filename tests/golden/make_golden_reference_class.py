"""Generates the fixtures that stand for the REFERENCE classes in the CPU network tests (tests/test_network_star.py,
tests/test_reference_dropin_import.py), so that those tests run wherever the repository does:

  reference_star_64.npz,   `networks.MEMC_Net_star` / `networks.MEMC_Net` (imported from the reference tree, unmodified;
  reference_base_64.npz    custom operators provided by the CPU oracle, tests/_oracle_ops.py) with name-derived weights:
                           the state dict's names and shapes in order, inference outputs on fixed 64 x 64 inputs, and one
                           training step -- its loss, per-submodule gradient L1 norms, and per parameter tensor the
                           gradient's max |g|, sum |g| and its values at a seeded sample of positions (the arg-max among them;
                           _netutil.grad_sample_positions regenerates the positions, only the arg-max is stored)
  reference_imports.json   what the reference's `networks` modules import from `my_package` (module, names), recorded by
                           an import hook while the package is imported

Only vectors and names are stored; the reference source never enters the repository.  Run in the build container:
    python tests/golden/make_golden_reference_class.py
"""
import builtins
import json
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

# Stored form (lossless where it matters, ~40 % of the float32 size): every output and sampled gradient value as an integer
# multiple of a step, |value - q * step| <= step / 2, the step a quarter of the tolerance the test holds that value to; the
# test subtracts step / 2 from its tolerance, so a pass still bounds the distance to the EXACT value by the full tolerance.
OUT_TOL_REL = 2e-5          # tests/test_network_star.py: outputs within 2e-5 * max(1, max |want|)
GRAD_STEP_REL = 2.5e-4      # a quarter of the gradient tolerance (test_network_star.GRAD_RTOL = 1e-3) of the tensor's scale


def outputs(net, x):
    with torch.no_grad():
        frames_out, flows, filters, occl = net(x)
    return {"blended": frames_out[0], "rectified": frames_out[1], "flow0": flows[0], "flow1": flows[1],
            "occlusion0": occl[0], "occlusion1": occl[1],
            "filter0_mean": filters[0].mean(dim=1), "filter1_mean": filters[1].mean(dim=1)}


def state_layout(prefix, sd):
    return {prefix + "state_names": np.array(list(sd.keys())),
            prefix + "state_shapes": np.array(json.dumps([list(t.shape) for t in sd.values()]))}


def training_step(net, x3):
    net.train()
    losses, _f, _k, _o = net(x3)
    total = sum(l.abs().mean() for l in losses)
    total.backward()
    return float(total.detach())


def quantized_outputs(prefix, net, x):
    out = {}
    for k, v in outputs(net, x).items():
        v = v.numpy()
        tol = OUT_TOL_REL * max(1.0, float(np.abs(v).max()))
        out[prefix + "out_tol/" + k] = np.float64(tol)
        out[prefix + "out_step/" + k] = np.float64(tol / 4)
        out[prefix + "out/" + k] = _netutil.to_byte_planes(_netutil.quantize(v, tol / 4))
    return out


def star_vectors(ref):
    net = ref.MEMC_Net_star(channel=3, filter_size=4, training=False).eval()
    sd = net.state_dict()
    net.load_state_dict(_netutil.named_weights(sd))
    out = state_layout("star/", sd)
    out.update(quantized_outputs("star/", net, _netutil.frames(11, 2, 64, 64)))
    two = _netutil.frames(5, 1, 64, 64)
    out["star/train_loss"] = np.float64(training_step(net, torch.stack((two[0], 0.5 * (two[0] + two[1]), two[1]))))
    # one entry per quantity, one element per parameter tensor with a gradient (in star/grad_names order); the sampled values
    # of all tensors concatenated in that order (their counts follow from the regenerated positions)
    rec = {"names": [], "max": [], "l1": [], "argmax": [], "step": [], "values": []}
    for name, p in net.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.detach().reshape(-1)
        argmax = int(g.abs().argmax())
        idx = _netutil.grad_sample_positions(name, g.numel(), argmax)
        step = GRAD_STEP_REL * max(1e-3, float(g.abs().max()))
        q = _netutil.quantize(g[torch.from_numpy(idx)].numpy(), step)
        assert np.abs(q).max() < 2 ** 15
        rec["names"].append(name)
        rec["max"].append(float(g.abs().max()))
        rec["l1"].append(float(g.double().abs().sum()))
        rec["argmax"].append(argmax)
        rec["step"].append(step)
        rec["values"].append(q.astype(np.int16))
    out["star/grad_names"] = np.array(rec["names"])
    out["star/grad_max"] = np.array(rec["max"], dtype=np.float64)
    out["star/grad_l1"] = np.array(rec["l1"], dtype=np.float64)
    out["star/grad_argmax"] = np.array(rec["argmax"], dtype=np.int64)
    out["star/grad_step"] = np.array(rec["step"], dtype=np.float64)
    out["star/grad_values"] = np.concatenate(rec["values"])
    return out


def base_vectors(ref):
    net = ref.MEMC_Net(channel=3, filter_size=4, training=False).eval()
    sd = net.state_dict()
    net.load_state_dict(_netutil.named_weights(sd))
    out = state_layout("base/", sd)
    out.update(quantized_outputs("base/", net, _netutil.frames(13, 1, 64, 64)))
    out["base/train_loss"] = np.float64(training_step(net, _netutil.training_frames(5, 1, 64, 64)))
    out.update({"base/grad_l1_module/" + k: np.float64(v) for k, v in _netutil.grad_l1_by_module(net).items()})
    return out


def record_imports():
    """Imports the reference's `networks` package with the REAL my_package importable and records every
    `my_package` import a `networks` module makes."""
    seen = []
    real_import = builtins.__import__

    def hook(name, globals=None, locals=None, fromlist=(), level=0):
        caller = (globals or {}).get("__name__", "")
        if level == 0 and name.split(".")[0] == "my_package" and caller.split(".")[0] == "networks":
            entry = {"importer": caller, "module": name, "names": sorted(fromlist or ())}
            if entry not in seen:
                seen.append(entry)
        return real_import(name, globals, locals, fromlist, level)
    for k in [k for k in sys.modules if k == "my_package" or k.startswith("my_package.")]:
        del sys.modules[k]
    builtins.__import__ = hook
    try:
        _netutil.import_reference_networks()
    finally:
        builtins.__import__ = real_import
        _netutil.purge_networks()
    return sorted(seen, key=lambda e: (e["importer"], e["module"]))


def main():
    sys.path.insert(0, os.path.join(ROOT, "memc-net_amd"))
    imports = record_imports()
    with open(os.path.join(HERE, "reference_imports.json"), "w") as f:
        json.dump({"source": "the reference's networks package, imported unmodified (make_golden_reference_class.py)",
                   "imports": imports}, f, indent=1)
        f.write("\n")
    _oracle_ops.install()
    ref = _netutil.import_reference_networks()
    for cls, make in (("star", star_vectors), ("base", base_vectors)):
        torch.manual_seed(0)
        out = make(ref)
        out["torch_version"] = np.array(torch.__version__)
        path = os.path.join(HERE, "reference_%s_64.npz" % cls)
        np.savez_compressed(path, **out)
        print("%s: %d arrays, %d bytes" % (os.path.basename(path), len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
