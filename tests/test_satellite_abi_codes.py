"""The return code of every entry point of the seven satellite warp libraries (libmemc_hip_lp / lp_grad / blend_grad / mx /
mx_grad / mx_blend_grad / lp_blend_grad) for a fixed list of descriptor mutations of one 2x3x8x16 call, against tests/golden/satellite_abi_codes.json.  The order of the checks is
contract: malformed (-1), then empty (0), then not covered (1), then the launch; a call that is both malformed and not
covered returns -1.  CPU only: nothing is launched -- a case that the fixture marks as enqueued (L: the covered base call,
and what the half forwards hand to their one-lane-per-site kernels) is counted and not called.

The fixture is recorded from libraries built from the commit BEFORE a change, never from the tree under test:
    python tests/test_satellite_abi_codes.py --record <that checkout>/memc-net_amd/lib
(on a machine without a GPU: there a launch fails at once, and the recorder tells an enqueued call by its path string)."""
import ctypes
import hashlib
import json
import os
import re
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
FIXTURE = os.path.join(ROOT, "tests", "golden", "satellite_abi_codes.json")
F32, F16, BF16 = 0, 1, 2
N, C, H, W, TAPS = 2, 3, 8, 16, 16
CHAR = {-1: "E", 0: "Z", 1: "N"}               # and L: enqueued

# entry point -> (library, symbol, dtype arguments, tensors as (kind, storage), positions of outputs / gradients, optional).
# kind: i image [N, C, H, W], f flow [N, 2, H, W], t taps [N, K, H, W], o occlusion [N, 1, H, W].
# storage: P / F / G the first / second / third dtype argument, 3 always fp32.
ENTRIES = {
    "lp.fwd": ("lp", "FilterInterpolationLayer_gpu_forward_lp", 2, "iP fF tP iP", (3,), ()),
    "lp.blend": ("lp", "FilterInterpolationBlendLayer_gpu_forward_lp", 2, "iP iP fF fF tP tP oP oP iP", (8,), ()),
    "lp_grad.bwd": ("lp_grad", "FilterInterpolationLayer_gpu_backward_lp", 3, "iP fF tP iG i3 fF tP", (3, 4, 5, 6), (4,)),
    "blend_grad.bwd": ("blend_grad", "FilterInterpolationBlendLayer_gpu_backward", 0, "i3 f3 t3 o3 i3 f3 t3 o3", (4, 5, 6, 7), ()),
    "mx.fwd": ("mx", "FilterInterpolationLayer_gpu_forward_mx", 2, "i3 fF tP i3", (3,), ()),
    "mx.blend": ("mx", "FilterInterpolationBlendLayer_gpu_forward_mx", 2, "i3 i3 fF fF tP tP oP oP i3", (8,), ()),
    "mx_grad.bwd": ("mx_grad", "FilterInterpolationLayer_gpu_backward_mx", 2, "i3 fF tP i3 i3 fF tP", (3, 4, 5, 6), (4,)),
    "mx_blend_grad.bwd": ("mx_blend_grad", "FilterInterpolationBlendLayer_gpu_backward_mx", 2, "i3 fF tP oP i3 fF tP oP", (4, 5, 6, 7), ()),
    "lp_blend_grad.bwd": ("lp_blend_grad", "FilterInterpolationBlendLayer_gpu_backward_lp", 3, "iP fF tP oP iG fF tP oP", (4, 5, 6, 7), ()),
}
COMBOS = {0: [()],
          2: [(F16, F32), (F16, F16), (BF16, F32), (BF16, BF16), (F32, F32), (F16, BF16), (3, F32)],
          3: [(p, f, g) for p in (F16, BF16) for f in (F32, p) for g in (F32, p)] +
             [(F32, F32, F32), (F16, BF16, F32), (F16, F32, BF16)]}


class Tensor4(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("size", ctypes.c_int64 * 4), ("stride", ctypes.c_int64 * 4)]


def desc(shape, data=0x1000, row=None):
    """contiguous, or with rows of `row` elements"""
    t = Tensor4()
    t.data = data
    n, c, h, w = shape
    row = row or w
    t.size[:] = shape
    t.stride[:] = (c * h * row, h * row, row, 1)
    return t


def is_f32(storage, combo):
    return storage == "3" or combo["PFG".index(storage)] == F32


def build(tensors, combo, n=N, c=C, w=W, taps=TAPS, tap_off=0, f32_off=None):
    """the call's descriptors; tap_off: bytes added to every taps pointer; f32_off: the tensor whose pointer moves 2 bytes"""
    chans = {"i": c, "f": 2, "t": taps, "o": 1}
    out = []
    for i, (kind, _st) in enumerate(tensors):
        data = 0x1000 * (i + 1) + (tap_off if kind == "t" else 0) + (2 if i == f32_off else 0)
        out.append(desc((n, chans[kind], H, w), data=data if n else 0))
    return out


def cases(tensors, grads, combo):
    """[(name, build keywords, descriptor mutation or None)]: the single mutations, then every malformed x uncovered pair"""
    def null(i):
        return lambda d: d.__setitem__(i, None)

    def nodata(i):
        return lambda d: setattr(d[i], "data", 0)

    def stride(i, dim, v):
        return lambda d: d[i].stride.__setitem__(dim, v)

    def grow(i, dim):
        def f(d):
            shape = list(d[i].size)
            shape[dim] += 1
            d[i] = desc(shape, data=d[i].data)
        return f

    def rows(i):
        return lambda d: d.__setitem__(i, desc(list(d[i].size), data=d[i].data, row=d[i].size[3] + 4))

    malformed = []
    for i in range(len(tensors)):
        malformed += [("null%d" % i, null(i)), ("nodata%d" % i, nodata(i)), ("wstride%d" % i, stride(i, 3, 2)),
                      ("bigstride%d" % i, stride(i, 0, 1 << 33))]
        malformed += [("grow%d.%d" % (i, dim), grow(i, dim)) for dim in range(4)]
    malformed += [("rows%d" % i, rows(i)) for i in grads]
    uncovered = [("C=4", dict(c=4)), ("W=4", dict(w=4)), ("W=10", dict(w=10)), ("W=18", dict(w=18)),
                 ("taps=8", dict(taps=8)), ("taps=25", dict(taps=25)), ("tapptr+4", dict(tap_off=4))]
    uncovered += [("f32ptr%d+2" % i, dict(f32_off=i)) for i, (_k, st) in enumerate(tensors) if is_f32(st, combo)]
    bad_taps = [("taps=0", dict(taps=0)), ("taps=15", dict(taps=15))]

    out = [("base", {}, None), ("batch=0", dict(n=0), None)]
    out += [(name, {}, m) for name, m in malformed]
    out += [(name, kw, None) for name, kw in bad_taps + uncovered]
    out += [(a + "&" + b, kw, m) for a, m in malformed for b, kw in uncovered]
    out += [(a + "&" + b, dict(kwa, **kwb), None) for a, kwa in bad_taps for b, kwb in uncovered if "taps" not in kwb]
    return out


def load(libdir):
    libs = {}
    for name in sorted({e[0] for e in ENTRIES.values()}):
        L = ctypes.CDLL(os.path.join(libdir, "libmemc_hip_%s.so" % name))
        L.path = getattr(L, "memc_%s_last_kernel_path" % name)
        L.path.restype = ctypes.c_char_p
        libs[name] = L
    for name, symbol, lead, tensors, _g, _o in ENTRIES.values():
        f = getattr(libs[name], symbol)
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * lead + [ctypes.POINTER(Tensor4)] * len(tensors.split())
    return libs


def run(libs, entry, combo, case):
    """the code of one case, and the thread's path string after it"""
    name, symbol, _lead, tensors, _g, _o = ENTRIES[entry]
    _label, kw, mutate = case
    d = build([tuple(t) for t in tensors.split()], combo, **kw)
    if mutate:
        mutate(d)
    code = getattr(libs[name], symbol)(None, *combo, *(None if t is None else ctypes.byref(t) for t in d))
    return code, libs[name].path()


def entry_cases(entry, combo):
    _name, _symbol, _lead, tensors, grads, _o = ENTRIES[entry]
    return cases([tuple(t) for t in tensors.split()], grads, combo)


def rle(chars):
    return "".join("%s%d" % (m.group(1), len(m.group(0))) for m in re.finditer(r"(.)\1*", chars))


def unrle(text):
    return "".join(c * int(n) for c, n in re.findall(r"([A-Z])(\d+)", text))


def names_digest(cs):
    return hashlib.sha1("\n".join(c[0] for c in cs).encode()).hexdigest()[:12]


def record(libdir):
    """every case in a thread of its own: the path string is per thread, so a non-empty one means THIS call enqueued"""
    libs = load(libdir)
    fixture = {}
    for entry, (_n, _s, lead, _t, _g, _o) in ENTRIES.items():
        for combo in COMBOS[lead]:
            cs, chars = entry_cases(entry, combo), []
            for case in cs:
                got = []
                th = threading.Thread(target=lambda: got.extend(run(libs, entry, combo, case)))
                th.start()
                th.join()
                chars.append("L" if got[1] else CHAR[got[0]])
            fixture["%s %s" % (entry, ",".join(map(str, combo)))] = {"cases": names_digest(cs), "codes": rle("".join(chars))}
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d (entry point, dtypes) lists in %s" % (len(fixture), FIXTURE))


@pytest.fixture(scope="module")
def libs():
    if not os.path.exists(os.path.join(LIBDIR, "libmemc_hip_mx_grad.so")):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return load(LIBDIR)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(FIXTURE))


def test_the_fixture_covers_every_entry_point_and_dtype_combination(golden):
    assert sorted(golden) == sorted("%s %s" % (e, ",".join(map(str, c))) for e, v in ENTRIES.items() for c in COMBOS[v[2]])


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_return_codes_are_the_recorded_ones(libs, golden, entry):
    wrong, called = [], 0
    for combo in COMBOS[ENTRIES[entry][2]]:
        want = golden["%s %s" % (entry, ",".join(map(str, combo)))]
        cs = entry_cases(entry, combo)
        assert names_digest(cs) == want["cases"], "the list of cases changed: record the fixture again from the parent commit"
        codes = unrle(want["codes"])
        assert len(codes) == len(cs)
        for case, c in zip(cs, codes):
            if c == "L":                       # would enqueue: not called
                continue
            code, path = run(libs, entry, combo, case)
            called += 1
            if CHAR.get(code) != c or path != b"":
                wrong.append((combo, case[0], c, code, path))
    assert not wrong, wrong[:20]
    assert called > 400, called


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    record(sys.argv[2])
