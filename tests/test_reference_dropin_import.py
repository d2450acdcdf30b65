"""The drop-in claim, at the import surface: what the reference's own, UNMODIFIED `networks` modules import from
`my_package` (recorded in tests/golden/reference_imports.json by make_golden_reference_class.py while the reference
package was imported) resolves, with the REAL `memc-net_amd/my_package` (the ctypes loader over libmemc_hip.so -- not
the oracle-backed stand-in the other network tests install) on `sys.path`, to this repository's classes; the network
built on them constructs, and the first operator call on CPU tensors fails with the loader's "no CPU path" error --
i.e. the reference's import lines reach the real HIP binding and nothing falls back.

CPU only.  On a GPU the same network running on the HIP operators is covered by tests/test_gpu_network.py."""
import importlib
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _netutil      # noqa: E402


def _fresh_real_my_package():
    for k in [k for k in sys.modules if k == "my_package" or k.startswith("my_package.")]:
        del sys.modules[k]
    import my_package._ext.my_lib as my_lib
    assert "memc-net_amd" in my_lib.__file__ and os.path.exists(my_lib.LIB_PATH)
    return my_lib


def test_unmodified_reference_network_reaches_the_real_loader():
    my_lib = _fresh_real_my_package()
    with open(os.path.join(HERE, "golden", "reference_imports.json")) as f:
        imports = json.load(f)["imports"]
    importers = {e["importer"] for e in imports}
    assert {"networks.MEMC_Net", "networks.MEMC_Net_star"} <= importers
    try:
        # every name the reference's network modules import (MEMC_Net_star.py:6-7 and the others) resolves to a class
        # of this repository's my_package
        for e in imports:
            mod = importlib.import_module(e["module"])
            assert "memc-net_amd" in mod.__file__, e
            for name in e["names"]:
                cls = getattr(mod, name)
                assert isinstance(cls, type) and issubclass(cls, torch.nn.Module), e
        assert sys.modules["my_package._ext.my_lib"] is my_lib
        from my_package.modules.FilterInterpolationModule import FilterInterpolationModule
        from my_package.modules.FlowProjectionModule import FlowProjectionModule
        _netutil.purge_networks()
        import networks
        assert "memc-net_amd" in networks.__file__
        net = networks.MEMC_Net_star(channel=3, filter_size=4, training=False).eval()
        assert sum(p.numel() for p in net.parameters()) == 70312501
        base = sys.modules["networks._base"]         # where the network binds the operator classes it calls
        assert base.FilterInterpolationModule is FilterInterpolationModule
        assert base.FlowProjectionModule is FlowProjectionModule
        x = _netutil.frames(3, 1, 128, 128)
        with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
            net(x)                                   # first custom operator on the path: FlowProjectionModule
    finally:
        _netutil.purge_networks()


def test_unmodified_reference_operator_call_sites():
    """The call shapes of MEMC_Net_star.py:264-285 against the real modules: constructor arguments, argument
    counts, and the error type on CPU tensors (the reference's own CPU branches die with NameError instead)."""
    _fresh_real_my_package()
    from my_package.modules.FilterInterpolationModule import FilterInterpolationModule
    from my_package.modules.FlowProjectionModule import FlowProjectionModule
    from my_package.modules.InterpolationModule import InterpolationModule
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU path"):
        FlowProjectionModule(z(1, 2, 8, 8).requires_grad)(z(1, 2, 8, 8))        # :266
    with pytest.raises(RuntimeError, match="no CPU path"):
        FilterInterpolationModule()(z(1, 3, 8, 8), z(1, 2, 8, 8), z(1, 16, 8, 8))   # :274-275
    with pytest.raises(RuntimeError, match="no CPU path"):
        InterpolationModule()(z(1, 3, 8, 8), z(1, 2, 8, 8))                      # MEMC_Net_VE.py:454
