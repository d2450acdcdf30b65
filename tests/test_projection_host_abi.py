"""What the projection's host code answers before any launch, against tests/golden/projection_host_abi.json:
memc_flow_projection_workspace_bytes over a grid of shapes, and the return codes of the six (Depth)FlowProjection
_kernel / _kernel_ws entry points for the calls that return before they touch the HIP runtime -- an empty shape (0), a NULL
workspace (-1, checked before the shape).  CPU only: no call that would enqueue is made, and none that reaches the
workspace's size and alignment checks (they sit behind the query whether the stream is capturing).

The fixture is recorded from a library built from the commit BEFORE a change, never from the tree under test:
    python tests/test_projection_host_abi.py --record <that checkout>/memc-net_amd/lib"""
import ctypes
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "memc-net_amd", "lib")
FIXTURE = os.path.join(ROOT, "tests", "golden", "projection_host_abi.json")

GRID = {"w": [0, 1, 7, 8, 63, 64, 65, 198, 1280], "h": [0, 1, 31, 32, 33, 100, 720], "batch": [0, 1, 3, 32],
        "fillhole": [0, 1], "depth": [0, 1]}
EMPTY = [(0, 8, 2), (16, 0, 2), (16, 8, 0), (-1, 8, 2), (16, -3, 2), (16, 8, -1), (0, 0, 0)]     # (w, h, batch)
FULL = (16, 8, 2)

# entry point -> (has fillhole, has the depth's strides, number of tensors, takes a workspace)
ENTRIES = {
    "FlowProjection_gpu_forward_kernel": (True, False, 3, False),
    "FlowProjection_gpu_backward_kernel": (False, False, 4, False),
    "DepthFlowProjection_gpu_forward_kernel": (True, True, 4, False),
    "DepthFlowProjection_gpu_backward_kernel": (False, True, 7, False),
    "FlowProjection_gpu_forward_kernel_ws": (True, False, 3, True),
    "DepthFlowProjection_gpu_forward_kernel_ws": (True, True, 4, True),
}


def load(libdir):
    lib = ctypes.CDLL(os.path.join(libdir, "libmemc_hip.so"))
    lib.memc_flow_projection_workspace_bytes.restype = ctypes.c_size_t
    lib.memc_flow_projection_workspace_bytes.argtypes = [ctypes.c_int] * 5
    for name, (fill, depth, tensors, ws) in ENTRIES.items():
        f = getattr(lib, name)
        f.restype = ctypes.c_int
        f.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * (5 + fill + 4 * (2 + depth)) + [ctypes.c_void_p] * tensors +
                      ([ctypes.c_void_p, ctypes.c_size_t] if ws else []))
    return lib


def call(lib, name, shape, workspace=None):
    """contiguous tensors that are never read: every call made here returns before its first launch"""
    fill, depth, tensors, ws = ENTRIES[name]
    w, h, batch = shape
    strides = lambda c: [c * h * w, h * w, w, 1]
    args = [None, batch * 2 * h * w, w, h, 2, batch] + [1] * fill + strides(2) + (strides(1) if depth else []) + strides(1)
    args += [0x1000 * (i + 1) for i in range(tensors)]
    if ws:
        args += [workspace, 1 << 30]
    return getattr(lib, name)(*args)


def code_cases():
    """[(label, entry point, shape, workspace)]"""
    out = []
    for name, (_f, _d, _t, ws) in ENTRIES.items():
        out += [("%s %s" % (name, shape), name, shape, 0x100000 if ws else None) for shape in EMPTY]
        if ws:
            out += [("%s %s NULL" % (name, shape), name, shape, None) for shape in EMPTY + [FULL]]
    return out


def workspace_cases():
    return list(itertools.product(*(GRID[k] for k in ("w", "h", "batch", "fillhole", "depth"))))


def record(libdir):
    lib = load(libdir)
    fixture = {"grid": GRID,
               "workspace_bytes": [lib.memc_flow_projection_workspace_bytes(*c) for c in workspace_cases()],
               "codes": {label: call(lib, name, shape, ws) for label, name, shape, ws in code_cases()}}
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d sizes and %d codes in %s" % (len(fixture["workspace_bytes"]), len(fixture["codes"]), FIXTURE))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(LIBDIR, "libmemc_hip.so")):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return load(LIBDIR)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(FIXTURE))


def test_workspace_bytes_are_the_recorded_ones(lib, golden):
    assert golden["grid"] == GRID, "the grid changed: record the fixture again from the parent commit"
    cases = workspace_cases()
    assert len(golden["workspace_bytes"]) == len(cases) == 1008
    got = [lib.memc_flow_projection_workspace_bytes(*c) for c in cases]
    wrong = [(c, want, g) for c, want, g in zip(cases, golden["workspace_bytes"], got) if want != g]
    assert not wrong, wrong[:20]
    # (what the numbers must at least say: nothing for an empty shape, a multiple of 256 bytes, no less with hole filling)
    assert all((g == 0) == (0 in c[:3]) and g % 256 == 0 for c, g in zip(cases, got))
    size = dict(zip(cases, got))
    assert all(size[c[:3] + (1,) + c[4:]] >= size[c[:3] + (0,) + c[4:]] for c in cases if 0 not in c[:3])


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_return_codes_before_any_launch_are_the_recorded_ones(lib, golden, name):
    mine = [c for c in code_cases() if c[1] == name]
    assert sorted(golden["codes"]) == sorted(c[0] for c in code_cases()), "the cases changed: record the fixture again"
    assert len(mine) == (15 if ENTRIES[name][3] else 7)
    wrong = [(label, golden["codes"][label], got) for label, _n, shape, ws in mine
             for got in [call(lib, name, shape, ws)] if got != golden["codes"][label]]
    assert not wrong, wrong
    # the contract the recorded codes spell: an empty shape is served (0); a NULL workspace is refused (-1) before that
    assert all(golden["codes"][label] == (-1 if label.endswith("NULL") else 0) for label, _n, _s, _w in mine)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    record(sys.argv[2])
