"""The bad calls of tests/golden/frame_binding_messages.json: for each of the four plane bindings (my_lib_video, my_lib_video_lp,
my_lib_still, my_lib_ssim) and each of its functions, one good call of 2 frames of 6x10 and, per tensor argument, the
mutations that the binding must refuse with an exception of its own before it reaches the library.  Shared by
test_frame_bindings_host.py (the `host` cases, on stand-ins that say they live on a device) and
test_gpu_frame_bindings.py (the `gpu` cases, on real device tensors); not a test module.

The fixture is recorded from the bindings of the commit BEFORE a change, never from the tree under test:
    python tests/_frame_binding_cases.py --record <that checkout>/memc-net_amd tests/golden/frame_binding_messages.json
It keeps what the file already holds and replaces the cases that the machine can run: without a GPU the host cases and the
missing-library messages, with one the gpu cases too.  A case with a tensor on another device needs two; a machine with
fewer records it on stand-ins that name two devices (the bindings compare `.device`, no more).  The paths in a
missing-library message are stored as {path} and {csrc}."""
import importlib
import json
import os
import sys

import torch

BINDINGS = ["my_lib_video", "my_lib_video_lp", "my_lib_still", "my_lib_ssim"]
F, H, W = 2, 6, 10
PADS = (2, 1, 1, 0)                                # left, right, top, bottom
HP, WP = H + PADS[2] + PADS[3], W + PADS[0] + PADS[1]
RGB = ("b", "uint8", (F, H, W, 3))
I420 = ("b", "uint8", (F * H * W * 3 // 2,))
WORK = ("w", "uint8", (1 << 16,))
SUMS = ("s", "int64", (F, 2))
SSIM = ("s", "float64", (F,))
PLANE = ("v", "uint8", (F, H, W))


def planes(dtype, padded):
    return ("p", dtype, (F, 3, HP, WP) if padded else (F, 3, H, W))


# binding -> function -> its keyword arguments in order: a tensor as (role, dtype, shape), anything else as it is.
# role: b contiguous bytes, p planes of the network's storage (w-stride 1), v a strided byte view, s per-frame results, w workspace.
CALLS = {
    "my_lib_video": {
        "i420_decode": dict(i420=I420, frames=F, h=H, w=W, rgb=RGB, planes=planes("float32", True), pads=PADS),
        "rgb_quantise": dict(planes=planes("float32", False), rgb=RGB),
        "i420_encode": dict(rgb=RGB, frames=F, h=H, w=W, i420=I420),
        "luma_score": dict(rgb_a=RGB, rgb_b=RGB, frames=F, h=H, w=W, sums=SUMS, workspace=WORK),
    },
    "my_lib_video_lp": {
        "i420_decode": dict(i420=I420, frames=F, h=H, w=W, rgb=RGB, planes=planes("bfloat16", True), pads=PADS),
        "rgb_quantise": dict(planes=planes("float16", False), rgb=RGB),
    },
    "my_lib_still": {
        "rgb8_decode": dict(rgb=RGB, planes=planes("float16", True), pads=PADS),
        "rgb8_quantise": dict(planes=planes("float32", False), rgb=RGB),
        "rgb8_score": dict(a=RGB, b=RGB, sums=SUMS, work=WORK, diff=RGB),
    },
    "my_lib_ssim": {
        "ssim_u8": dict(a=PLANE, b=PLANE, ssim=SSIM, workspace=WORK),
        "ssim_luma_rgb": dict(rgb_a=RGB, rgb_b=RGB, frames=F, h=H, w=W, ssim=SSIM, workspace=WORK),
    },
}
# what each role is put through on a device: another dtype; the same shape on every second element of rows twice as long
# (as `noncontig` where the binding asks for a contiguous tensor, as `wstride` where it asks for a w-stride of 1); one more
# along the first axis (for s: a `sums` that is too short for what the other arguments say is none -- one too long is
# refused by the same check); a tensor on another device.  A workspace has no stated size.
GPU_MUTATIONS = {"b": ("dtype", "noncontig", "count", "device"), "p": ("dtype", "count", "wstride", "device"),
                 "v": ("dtype", "count", "wstride", "device"), "s": ("dtype", "noncontig", "short", "device"),
                 "w": ("dtype", "noncontig", "device")}
HOST_MUTATIONS = ("non_tensor", "cpu")


class OnDevice(torch.Tensor):
    """a CPU tensor that says it lives on a device: passes a binding's device checks and nothing else of a device"""
    is_cuda = True
    device = torch.device("cuda", 0)


class OnOtherDevice(OnDevice):
    device = torch.device("cuda", 1)


def tensor(spec, dev, how=None):
    """the tensor of `spec` on `dev`, or with dev None a stand-in, put through the mutation `how`"""
    _role, dtype, shape = spec
    dtype, shape = getattr(torch, dtype), list(shape)
    if how == "dtype":
        dtype = torch.float32 if dtype == torch.float64 else torch.float64
    if how in ("count", "short"):
        shape[0] += 1 if how == "count" else -1
    if how in ("noncontig", "wstride"):
        shape[-1] *= 2
    other = how == "device"
    if other and dev is not None:
        dev = torch.device("cuda", (dev.index + 1) % torch.cuda.device_count())
    t = torch.zeros(shape, dtype=dtype, device=dev or "cpu")
    if how in ("noncontig", "wstride"):
        t = t[..., ::2]
    return t if dev is not None else t.as_subclass(OnOtherDevice if other else OnDevice)


def cases(kind):
    """[(binding, function, case name, build)]: build(dev) -> the keyword arguments of the bad call, on tensors of dev or
    (dev None) on stand-ins.  kind `host`: the argument in turn a non-tensor or a plain CPU tensor; kind `gpu`: GPU_MUTATIONS."""
    out = []
    for binding in BINDINGS:
        for fn, args in CALLS[binding].items():
            for arg, spec in args.items():
                if not (isinstance(spec, tuple) and isinstance(spec[0], str)):
                    continue
                for how in (HOST_MUTATIONS if kind == "host" else GPU_MUTATIONS[spec[0]]):
                    out.append((binding, fn, "%s/%s:%s" % (fn, how, arg), _builder(args, arg, how)))
    return out


def _builder(args, bad, how):
    def build(dev=None):
        kw = {}
        for arg, spec in args.items():
            if not (isinstance(spec, tuple) and isinstance(spec[0], str)):
                kw[arg] = spec
            elif arg != bad:
                kw[arg] = tensor(spec, dev)
            else:
                kw[arg] = 7 if how == "non_tensor" else tensor(spec, torch.device("cpu")) if how == "cpu" else tensor(spec, dev, how)
        return kw
    return build


def load(package_dir, binding):
    if package_dir not in sys.path:
        sys.path.insert(0, package_dir)
    return importlib.import_module("my_package._ext." + binding)


def refusal(module, fn, kwargs):
    """[exception type, text] of a call that must not reach the library"""
    try:
        getattr(module, fn)(**kwargs)
    except (TypeError, ValueError, RuntimeError) as e:
        return [type(e).__name__, str(e)]
    raise AssertionError("%s.%s was not refused" % (module.__name__, fn))


def on_another_device(name):
    return "/device:" in name


def runnable(name):
    """can this machine run the gpu case on real tensors?"""
    n = torch.cuda.device_count() if torch.cuda.is_available() else 0
    return n > (1 if on_another_device(name) else 0)


def missing_library_message(module, missing):
    """the text of lib() with the binding's library path pointed at `missing`, the paths replaced by {path} and {csrc};
    the module is left as it was"""
    loader = getattr(module, "_LIB", None)             # the shared loader; before it, each module bound itself
    holder, attr = (loader, "path") if loader is not None else (module, "LIB_PATH")
    saved = getattr(holder, attr), holder._lib
    setattr(holder, attr, missing)
    holder._lib = None
    try:
        (loader or module).lib()
    except RuntimeError as e:
        csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(module.__file__))))), "csrc")
        return str(e).replace(missing, "{path}").replace(csrc, "{csrc}")
    finally:
        setattr(holder, attr, saved[0])
        holder._lib = saved[1]
    raise AssertionError("%s.lib() found %s" % (module.__name__, missing))


def record(package_dir, path):
    fixture = json.load(open(path)) if os.path.exists(path) else {}
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else None
    for binding in BINDINGS:
        module = load(package_dir, binding)
        entry = fixture.setdefault(binding, {"missing_library": None, "host": {}, "gpu": {}})
        name = os.path.basename(module.LIB_PATH)
        entry["missing_library"] = missing_library_message(module, os.path.join(package_dir, "nowhere", name))
        for kind in ("host", "gpu"):
            for b, fn, case, build in cases(kind):
                if b != binding:
                    continue
                if kind == "host" or (on_another_device(case) and not runnable(case)):
                    entry[kind][case] = refusal(module, fn, build(None))
                elif runnable(case):
                    entry[kind][case] = refusal(module, fn, build(dev))
    with open(path, "w") as f:
        json.dump(fixture, f, indent=1, sort_keys=True)
        f.write("\n")
    print({b: {k: len(v) for k, v in e.items() if isinstance(v, dict)} for b, e in fixture.items()})


if __name__ == "__main__":
    if len(sys.argv) != 4 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    record(os.path.abspath(sys.argv[2]), sys.argv[3])
