"""What the four plane bindings (my_lib_video, my_lib_video_lp, my_lib_still, my_lib_ssim) refuse of tensors that do live on
a device, word for word against the `gpu` cases of tests/golden/frame_binding_messages.json: per tensor argument of one call
of 2 frames of 6x10 another dtype, bytes that are not contiguous, another element count or shape, a w-stride of 2, a tensor
on another device (needs two) and a `sums` that is too short.  Each is refused by the binding before the library is called:
nothing is launched.

The fixture was recorded from the bindings of the commit before they moved onto one loader and one set of checks
(my_package/_ext/_satellite.py), on one MI355X: its cases on real device tensors, those with a tensor on another device on
stand-ins that name two (that machine had one; test_frame_bindings_host.py runs them the same way everywhere).
tests/_frame_binding_cases.py holds the cases and says how to record.  The cases that need no device are
test_frame_bindings_host.py's."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _frame_binding_cases as C      # noqa: E402

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "memc-net_amd")
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "frame_binding_messages.json")))
GPU = C.cases("gpu")


def test_the_fixture_holds_every_gpu_case_and_no_other():
    for binding in C.BINDINGS:
        assert sorted(FIXTURE[binding]["gpu"]) == sorted(c for b, _f, c, _k in GPU if b == binding)


@pytest.mark.parametrize("binding,fn,case", [c[:3] for c in GPU], ids=["%s-%s" % (c[0], c[2]) for c in GPU])
def test_a_bad_tensor_is_refused_in_the_recorded_words(binding, fn, case):
    if not C.runnable(case):
        pytest.skip("a tensor on another device needs two")
    build = next(c[3] for c in GPU if c[0] == binding and c[2] == case)
    assert C.refusal(C.load(PKG, binding), fn, build(torch.device("cuda", 0))) == FIXTURE[binding]["gpu"][case]
