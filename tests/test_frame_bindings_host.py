"""What the four plane bindings (my_lib_video, my_lib_video_lp, my_lib_still, my_lib_ssim) refuse without a device, word for
word against tests/golden/frame_binding_messages.json: a non-tensor and a CPU tensor in the place of every tensor argument
(the other arguments stand-ins that say they live on a device, so that each argument's own check is reached), a tensor that
names another device than the others, and a loader whose library file does not exist.  Importing the four loads no library.
CPU only; nothing reaches a library.

The fixture was recorded from the bindings of the commit before they moved onto one loader and one set of checks
(my_package/_ext/_satellite.py), when each module carried its own; tests/_frame_binding_cases.py holds the cases and says
how to record.  The rest of the fixture (its `gpu` cases) needs tensors on a device: test_gpu_frame_bindings.py."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _frame_binding_cases as C      # noqa: E402

PKG = os.path.join(ROOT, "memc-net_amd")
FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "frame_binding_messages.json")))
HOST = C.cases("host")
OTHER_DEVICE = [c for c in C.cases("gpu") if C.on_another_device(c[2])]


def test_the_fixture_holds_every_host_case_and_no_other():
    for binding in C.BINDINGS:
        assert sorted(FIXTURE[binding]["host"]) == sorted(c for b, _f, c, _k in HOST if b == binding)
    assert len(HOST) == 66                         # a non-tensor and a CPU tensor for each of the 33 tensor arguments


@pytest.mark.parametrize("binding,fn,case", [c[:3] for c in HOST], ids=["%s-%s" % (c[0], c[2]) for c in HOST])
def test_a_bad_argument_is_refused_in_the_recorded_words(binding, fn, case):
    build = next(c[3] for c in HOST if c[0] == binding and c[2] == case)
    assert C.refusal(C.load(PKG, binding), fn, build()) == FIXTURE[binding]["host"][case]


@pytest.mark.parametrize("binding,fn,case", [c[:3] for c in OTHER_DEVICE], ids=["%s-%s" % (c[0], c[2]) for c in OTHER_DEVICE])
def test_a_tensor_on_another_device_is_refused_in_the_recorded_words(binding, fn, case):
    """the fixture's `gpu` cases that need two devices, here on stand-ins that name two: a machine with one skips them"""
    build = next(c[3] for c in OTHER_DEVICE if c[0] == binding and c[2] == case)
    assert C.refusal(C.load(PKG, binding), fn, build()) == FIXTURE[binding]["gpu"][case]


@pytest.mark.parametrize("binding", C.BINDINGS)
def test_a_missing_library_names_the_file_the_build_and_its_own_sentence(binding, tmp_path):
    module = C.load(PKG, binding)
    missing = str(tmp_path / os.path.basename(module.LIB_PATH))
    text = C.missing_library_message(module, missing)
    assert text == FIXTURE[binding]["missing_library"]
    assert text.startswith(os.path.basename(module.LIB_PATH) + " not found at {path} -- build it with `make -C {csrc}`")
    sentence = {"my_lib_video": "the GPU frame I/O has no fallback", "my_lib_video_lp": "the fp16 / bf16 frame I/O has no fallback",
                "my_lib_still": "the still-image GPU frame I/O has no fallback", "my_lib_ssim": "the GPU SSIM has no fallback"}
    assert text.endswith("; " + sentence[binding])
    assert module.LIB_PATH == os.path.join(PKG, "lib", os.path.basename(module.LIB_PATH))      # and the module is as it was


def test_importing_the_four_loads_no_library():
    """in a fresh interpreter: after the imports no libmemc_hip*.so is mapped"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import my_package._ext.my_lib_video, my_package._ext.my_lib_video_lp\n"
            "import my_package._ext.my_lib_still, my_package._ext.my_lib_ssim\n"
            "print([l.split()[-1] for l in open('/proc/self/maps') if 'libmemc_hip' in l])" % PKG)
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert out.strip() == "[]", out
