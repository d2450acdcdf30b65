"""tests/_far_views.py -- views at the limits of 32-bit addressing: the guard rules restated in integers, the strides just
inside and just outside them, one arena out of which such views are cut, and the table of guarded (entry point, tensor
group) pairs of DESIGN.md's "Addressing audit".  A helper: tests/test_far_views_host.py (arithmetic only),
tests/test_far_views_abi.py (return codes, nothing launched) and tests/test_gpu_far_views.py (the device) import it.

The rules (independent of the C++: plain Python integers never wrap):
    fits_u32      ((h - 1) * row_stride + w) * 4 < 2^32         memc_tile.hpp plane_fits_u32: 32-bit BYTE offsets
    fits_int      (h - 1) * row_stride + w <= INT32_MAX         fi_stack.hip plane_fits_int, spynet_level*.hip, layer_api.cpp
    owner_4plane  4 * (3 * chan_stride + (h - 1) * row_stride + w) < 2^32      fi_bwd_cn.hip bwd_cn_owner_ok
A group is the set of tensors that the host checks force to share strides (same_layout); at a limit its tensors share one
stride tuple and INTERLEAVE: row r of every plane of every tensor of the group lies inside the same row-stride gap, so a
call whose planes span 4 or 8 GiB of addresses touches a few hundred KiB."""
import collections

INT32_MAX = (1 << 31) - 1
F32, F16, BF16 = 0, 1, 2                        # memc_dtype
CANARY_BITS = 0x7FC0BEEF                        # a quiet NaN with a payload: what an arena holds outside its windows


def fits_u32(h, w, row_stride):
    return (max(h - 1, 0) * row_stride + w) * 4 < (1 << 32)


def fits_int(h, w, row_stride):
    return max(h - 1, 0) * row_stride + w <= INT32_MAX


def owner_4plane(h, w, row_stride, chan_stride):
    return 4 * (3 * chan_stride + max(h - 1, 0) * row_stride + w) < (1 << 32)


def near_far(rule, h, w, quantum):
    """(near, far): the largest row stride that is a multiple of `quantum` and that rule(h, w, stride) admits, and that
    stride plus `quantum`.  rule: monotone in the stride (admits 0 .. some limit), e.g. fits_u32 or
    lambda h, w, s: owner_4plane(h, w, s, chan_stride).  Bisection on the multiple; needs h >= 2 (a one-row plane has no limit)."""
    assert h >= 2 and quantum >= 1 and rule(h, w, 0)
    lo, hi = 0, (1 << 33) // quantum            # rule(lo * quantum) holds, rule(hi * quantum) does not
    assert not rule(h, w, hi * quantum)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if rule(h, w, mid * quantum):
            lo = mid
        else:
            hi = mid
    return lo * quantum, hi * quantum


RULES = {"u32": fits_u32, "int": fits_int}


def rule_of(key, group):
    """the rule that guards `group` of entry point `key`: ENTRIES[key].rule, or its entry for the group where it is a dict"""
    r = ENTRIES[key].rule
    return RULES[r[group] if isinstance(r, dict) else r]

# ------------------------------------------------------------------------------------------------------------------
# Windows and layouts: integers only (the host tests run these on the CPU; Arena below puts one on a device)
# ------------------------------------------------------------------------------------------------------------------
Window = collections.namedtuple("Window", "name shape strides base itemsize")


def window_rows(w):
    """the [lo, hi) BYTE intervals of a window's rows (its contiguous runs)"""
    (B, C, H, W), (sb, sc, sh, sw) = w.shape, w.strides
    assert sw == 1
    return [((w.base + b * sb + c * sc + y * sh) * w.itemsize, (w.base + b * sb + c * sc + y * sh + W) * w.itemsize)
            for b in range(B) for c in range(C) for y in range(H)]


class Layout(object):
    """Windows inside [0, nbytes).  view() records one and checks what every library asks of a tensor: strides that fit
    `int`, a base aligned to `align` bytes; check() that no two windows share a byte."""

    def __init__(self):
        self.windows = []

    def view(self, name, shape, strides, base, itemsize=4, align=4):
        assert len(shape) == 4 and len(strides) == 4 and strides[3] == 1
        assert all(0 <= s <= INT32_MAX for s in strides), "a stride of %s does not fit int: %s" % (name, (strides,))
        assert base >= 0 and (base * itemsize) % align == 0, "%s: base %d x %d B is not %d-byte aligned" % (name, base, itemsize, align)
        w = Window(name, tuple(shape), tuple(strides), base, itemsize)
        self.windows.append(w)
        return w

    @property
    def nbytes(self):
        return max(hi for w in self.windows for _lo, hi in window_rows(w))

    def check(self):
        rows = sorted((lo, hi, w.name) for w in self.windows for lo, hi in window_rows(w))
        for (alo, ahi, an), (blo, bhi, bn) in zip(rows, rows[1:]):
            assert ahi <= blo, "windows overlap: %s [%d, %d) and %s [%d, %d)" % (an, alo, ahi, bn, blo, bhi)
        return self


def pad4(w):
    return (w + 3) & ~3


def interleave(layout, tensors, row_stride, base=0, itemsize=4, align=16):
    """Place `tensors` [(name, shape)] with the row stride `row_stride` so that they interleave: channel stride the padded
    width, batch stride C * that, tensor after tensor inside the first row gap.  Tensors of the same shape get the same
    stride tuple (a same_layout group).  Returns {name: Window} and the first free element behind them in the row gap."""
    out, at = {}, base
    for name, (B, C, H, W) in tensors:
        wp = pad4(W)
        out[name] = layout.view(name, (B, C, H, W), (C * wp, wp, row_stride, 1), at, itemsize, align)
        at += B * C * wp
    assert at - base <= row_stride, "the row gap of %d elements cannot hold %d" % (row_stride, at - base)
    return out, at


def far_outer(layout, tensors, dim, itemsize=4, align=16):
    """Ordinary rows, and per tensor a batch (dim 0) or channel (dim 1) stride such that (size - 1) * stride exceeds 2^31
    elements (2^32 bytes even of halves) while the stride itself fits int.  tensors: (name, shape) or (name, shape,
    itemsize).  The tensors, and the planes of the other outer dimension, interleave inside the first gap (16-byte
    aligned slots of the fp32 size whatever the storage).  Returns {name: Window}."""
    assert dim in (0, 1)
    out, at = {}, 0                              # at: bytes
    for t in tensors:
        name, (B, C, H, W) = t[0], t[1]
        size = t[2] if len(t) > 2 else itemsize
        n = (B, C)[dim]
        assert n >= 3, "%s: (n - 1) * stride beyond 2^31 needs a stride beyond int with n = %d" % (name, n)
        stride = pad4(((1 << 31) + (n - 1)) // (n - 1) + 64)   # (n - 1) * stride > 2^31
        wp = pad4(W)
        strides = (stride, H * wp, wp, 1) if dim == 0 else (H * wp, stride, wp, 1)
        out[name] = layout.view(name, (B, C, H, W), strides, at // size, size, align)
        at += (C if dim == 0 else B) * H * wp * 4
    assert at <= (1 << 26)                       # far inside the smallest stride (2^31 / 63)
    return out


# ------------------------------------------------------------------------------------------------------------------
# The arena: one device allocation filled with a canary
# ------------------------------------------------------------------------------------------------------------------
class Arena(object):
    """`numel` fp32 elements on `device`, every one the canary (a NaN with a payload: a kernel that READS outside its
    windows poisons its result, one that WRITES outside them is found by untouched_outside).  tensor(window) cuts the
    as_strided view of a Layout's window (fp32, or two halves per element for itemsize 2)."""

    def __init__(self, numel, device):
        import torch
        self.torch = torch
        self.bits = torch.empty(numel, dtype=torch.int32, device=device)
        self.numel = numel
        self.cut = []
        self.fill()

    def fill(self):
        self.bits.fill_(CANARY_BITS)                           # (below 2^31: the same number as an int32)
        self.cut = []

    def tensor(self, window, dtype=None):
        torch = self.torch
        dtype = dtype or torch.float32
        assert torch.empty(0, dtype=dtype).element_size() == window.itemsize
        assert max(hi for _lo, hi in window_rows(window)) <= self.numel * 4
        t = self.bits.view(dtype).as_strided(window.shape, window.strides, window.base)
        self.cut.append(t)
        return t

    def unwritten(self, windows):
        """every element of these windows (tensors cut by tensor()) still holds the canary: a refused call wrote nothing
        into them.  To be asked BEFORE untouched_outside, which resets the windows it is given."""
        torch = self.torch
        for t in windows:
            if t.element_size() == 4:
                bad = int(torch.count_nonzero(t.view(torch.int32) != CANARY_BITS))
            else:                                              # halves: the low half of a canary word at even elements
                assert t.storage_offset() % 2 == 0 and all(st % 2 == 0 for st in t.stride()[:3])
                h16 = t.view(torch.int16)
                bad = int(torch.count_nonzero(h16[..., 0::2] != (CANARY_BITS & 0xFFFF) - (1 << 16))) + \
                    int(torch.count_nonzero(h16[..., 1::2] != CANARY_BITS >> 16))
            assert bad == 0, "%d elements of a window that a refused call should have left alone were written" % bad

    def untouched_outside(self, outputs, inputs=None):
        """Reset the output windows and the input windows to the canary, then the whole arena must be the canary: nothing
        was written outside a window.  outputs / inputs: tensors cut by tensor(); inputs default to every other one cut
        since fill()."""
        torch = self.torch
        if inputs is None:
            inputs = [t for t in self.cut if not any(t is o for o in outputs)]
        canary = torch.tensor([CANARY_BITS], dtype=torch.int32, device=self.bits.device)
        for t in list(outputs) + list(inputs):
            if t.element_size() == 4:
                t.view(torch.int32).copy_(canary.expand(t.shape))
            else:                                              # halves: a canary word's low half at even elements, its high half at odd
                assert t.storage_offset() % 2 == 0 and all(st % 2 == 0 for st in t.stride()[:3])
                h16 = t.view(torch.int16)
                h16[..., 0::2] = (CANARY_BITS & 0xFFFF) - (1 << 16)
                h16[..., 1::2] = CANARY_BITS >> 16
        bad = 0
        step = 1 << 27                                         # (a chunk's comparison is 128 MiB of bool)
        for i in range(0, self.numel, step):
            bad += int(torch.count_nonzero(self.bits[i:i + step] != canary))
        assert bad == 0, "%d elements of the arena outside the windows were written" % bad


# ------------------------------------------------------------------------------------------------------------------
# The guarded (entry point, group) pairs: DESIGN.md "Addressing audit", the rows whose far side has a return code.
# tensors: (name, kind); kind -> channels: i image C, f flow 2, t taps 16, o occlusion / count / depth 1, x the stack's
# out (64), s SPyNet's out / gradoutput (8), q SPyNet's coarse flow (2 channels, half size).  groups: name -> positions.
# lead: the dtype arguments in front of the tensors; tail: the int arguments behind them.
# ------------------------------------------------------------------------------------------------------------------
Entry = collections.namedtuple("Entry", "lib symbol lead tensors tail groups rule quantum code half tail_types")


def _e(lib, symbol, lead, tensors, groups, rule="u32", quantum=4, code=1, tail=(), half=(), tail_types=None):
    """tail_types: one letter per trailing argument -- i int (the default), f float, p pointer, z size_t"""
    return Entry(lib, symbol, tuple(lead), tuple(tuple(t.split(":")) for t in tensors.split()), tuple(tail),
                 collections.OrderedDict(groups), rule, quantum, code, tuple(half), tail_types or "i" * len(tail))


_FI_BWD = (("image", (0, 3, 4)), ("flow", (1, 5)), ("taps", (2, 6)))
_BLEND_BWD = (("image", (0, 4)), ("flow", (1, 5)), ("taps", (2, 6)), ("occlusion", (3, 7)))
_BLEND_FWD = (("image", (0, 1, 8)), ("flow", (2, 3)), ("taps", (4, 5)), ("occlusion", (6, 7)))
_STACK = (("input1", (0,)), ("flow", (1,)), ("taps", (2,)), ("out", (3,)))
_STACK_TAIL = (6, 0, 3, -1, -1)                 # n_neighbours, c_base, skip, flow_base, tap_base: tests/test_stack_abi.py's call

# half: positions stored as the payload dtype (two bytes per element) in the call the ABI test makes (F16 payload, fp32 flow
# and gradoutput)
ENTRIES = collections.OrderedDict([
    ("lp_grad.bwd", _e("lp_grad", "FilterInterpolationLayer_gpu_backward_lp", (F16, F32, F32),
                       "input1:i input2:f input3:t gradoutput:i gradinput1:i gradinput2:f gradinput3:t", _FI_BWD, half=(0, 2, 6))),
    ("blend_grad.bwd", _e("blend_grad", "FilterInterpolationBlendLayer_gpu_backward", (),
                          "input:i flow:f filter:t occlusion:o gradoutput:i gradflow:f gradfilter:t gradocclusion:o", _BLEND_BWD)),
    ("mx.fwd", _e("mx", "FilterInterpolationLayer_gpu_forward_mx", (F16, F32), "input1:i input2:f input3:t output:i",
                  (("image", (0, 3)), ("flow", (1,)), ("taps", (2,))), half=(2,))),
    ("mx.blend", _e("mx", "FilterInterpolationBlendLayer_gpu_forward_mx", (F16, F32),
                    "input0:i input2:i flow0:f flow1:f filter0:t filter1:t occlusion0:o occlusion1:o output:i", _BLEND_FWD,
                    half=(4, 5, 6, 7))),
    ("mx_grad.bwd", _e("mx_grad", "FilterInterpolationLayer_gpu_backward_mx", (F16, F32),
                       "input1:i input2:f input3:t gradoutput:i gradinput1:i gradinput2:f gradinput3:t", _FI_BWD, half=(2, 6))),
    ("mx_blend_grad.bwd", _e("mx_blend_grad", "FilterInterpolationBlendLayer_gpu_backward_mx", (F16, F32),
                             "input:i flow:f filter:t occlusion:o gradoutput:i gradflow:f gradfilter:t gradocclusion:o",
                             _BLEND_BWD, half=(2, 3, 6, 7))),
    ("lp_blend_grad.bwd", _e("lp_blend_grad", "FilterInterpolationBlendLayer_gpu_backward_lp", (F16, F32, F32),
                             "input:i flow:f filter:t occlusion:o gradoutput:i gradflow:f gradfilter:t gradocclusion:o",
                             _BLEND_BWD, half=(0, 2, 3, 6, 7))),
    ("lp_bl.fwd", _e("lp_bl", "InterpolationLayer_gpu_forward_lp", (F16, F32), "input1:i input2:f output:i",
                     (("image", (0, 2)),), rule="int", half=(0, 2))),
    ("lp_bl.fwd_ch", _e("lp_bl", "InterpolationChLayer_gpu_forward_lp", (F16, F32), "input1:i input2:f output:i",
                        (("image", (0, 2)),), rule="int", half=(0, 2))),
    ("lp_bl.bwd", _e("lp_bl", "InterpolationLayer_gpu_backward_lp", (F16, F32),
                     "input1:i input2:f gradoutput:i gradinput1:i gradinput2:f", (("image", (0, 2, 3)),), half=(0, 2))),
    ("lp_bl.bwd_ch", _e("lp_bl", "InterpolationChLayer_gpu_backward_lp", (F16, F32),
                        "input1:i input2:f gradoutput:i gradinput1:i gradinput2:f", (("image", (0, 2, 3)),), half=(0, 2))),
    ("lp_proj_grad.bwd", _e("lp_proj_grad", "FlowProjectionLayer_gpu_backward_lp", (F16,),
                            "input1:f count:o gradoutput:f gradinput1:f", (("flow", (0, 2, 3)), ("count", (1,))),
                            half=(0, 2, 3))),
    ("lp_dproj_grad.bwd", _e("lp_dproj_grad", "DepthFlowProjectionLayer_gpu_backward_lp", (F16,),
                             "input1:f input2:o count:o output:f gradoutput:f gradinput1:f gradinput2:o",
                             (("flow", (0, 3, 4, 5)), ("depth", (1, 6)), ("count", (2,))), half=(0, 1, 4, 5, 6))),
    ("stack.fwd", _e("stack", "FilterInterpolationStackLayer_gpu_forward", (), "input1:I flow:F taps:T out:x", _STACK,
                     rule="int", tail=_STACK_TAIL)),
    ("lp_stack.fwd", _e("lp_stack", "FilterInterpolationStackLayer_gpu_forward_lp", (F16, F32),
                        "input1:I flow:F taps:T out:x", _STACK, rule="int", tail=_STACK_TAIL, half=(0, 2, 3))),
    ("spynet.fwd", _e("spynet", "SpyNetLevelLayer_gpu_forward", (), "first:i second:i coarse:q out:s",
                      (("first", (0,)), ("second", (1,)), ("coarse", (2,)), ("out", (3,))), rule="int", quantum=1,
                      tail=(0, 0))),
    ("spynet_grad.bwd", _e("spynet_grad", "SpyNetLevelLayer_gpu_backward", (), "second:i coarse:q gradoutput:s gradcoarse:q",
                           (("second", (0,)), ("coarse", (1,)), ("gradoutput", (2,)), ("gradcoarse", (3,))), rule="int",
                           quantum=1, tail=(0, 0))),
] + [
    # libmemc_hip.so (include/memc_warp.h, "Limits"): every tensor of every layer entry point under the int rule; a view
    # beyond it is malformed (-1).  Groups: the tensors that same_layout ties together.
    ("memc.bl_fwd", _e("", "InterpolationLayer_gpu_forward", (), "input1:i input2:f output:i",
                       (("image", (0, 2)), ("flow", (1,))), rule="int", quantum=1, code=-1)),
    ("memc.bl_fwd_ch", _e("", "InterpolationChLayer_gpu_forward", (), "input1:i input2:f output:i",
                          (("image", (0, 2)), ("flow", (1,))), rule="int", quantum=1, code=-1)),
    ("memc.bl_bwd", _e("", "InterpolationLayer_gpu_backward", (), "input1:i input2:f gradoutput:i gradinput1:i gradinput2:f",
                       (("image", (0, 2, 3)), ("flow", (1, 4))), rule="int", quantum=1, code=-1)),
    ("memc.bl_bwd_ch", _e("", "InterpolationChLayer_gpu_backward", (),
                          "input1:i input2:f gradoutput:i gradinput1:i gradinput2:f",
                          (("image", (0, 2, 3)), ("flow", (1, 4))), rule="int", quantum=1, code=-1)),
    ("memc.fi_fwd", _e("", "FilterInterpolationLayer_gpu_forward", (), "input1:i input2:f input3:t output:i",
                       (("image", (0, 3)), ("flow", (1,)), ("taps", (2,))), rule="int", quantum=1, code=-1)),
    ("memc.fi_bwd", _e("", "FilterInterpolationLayer_gpu_backward", (),
                       "input1:i input2:f input3:t gradoutput:i gradinput1:i gradinput2:f gradinput3:t", _FI_BWD, rule="int",
                       quantum=1, code=-1)),
    ("memc.fi_blend", _e("", "FilterInterpolationBlendLayer_gpu_forward", (),
                         "input0:i input2:i flow0:f flow1:f filter0:t filter1:t occlusion0:o occlusion1:o output:i",
                         _BLEND_FWD, rule="u32", quantum=1, code=-1)),     # filter_interpolation.hip:1197: -1, no 64-bit family
    ("memc.proj_fwd", _e("", "FlowProjectionLayer_gpu_forward", (), "input1:f count:o output:f",
                         (("flow", (0, 2)), ("count", (1,))), rule="int", quantum=1, code=-1, tail=(1,))),
    ("memc.fi_ctx", _e("", "FilterInterpolationCtxLayer_gpu_forward", (),
                       "image:i context:c flow:f filter:t prev:i occlusion_prev:o occlusion_this:o image_out:i context_out:c",
                       (("image", (0, 4, 7)), ("context", (1, 8)), ("flow", (2,)), ("taps", (3,)), ("occlusion", (5, 6))),
                       rule={"image": "u32", "occlusion": "u32", "context": "int", "flow": "int", "taps": "int"},  # :1229
                       quantum=1, code=-1)),
    ("memc.upsample4", _e("", "FlowUpsample4Layer_gpu_forward", (), "input:f output:u",
                          (("input", (0,)), ("output", (1,))), rule="int", quantum=1, code=-1, tail=(1.0, 1.0, 0),
                          tail_types="ffi")),
    ("memc.proj_fwd_ws", _e("", "FlowProjectionLayer_gpu_forward_ws", (), "input1:f count:o output:f",
                            (("flow", (0, 2)), ("count", (1,))), rule="int", quantum=1, code=-1, tail=(1, 0x20000, 1 << 20),
                            tail_types="ipz")),
    ("memc.dproj_fwd_ws", _e("", "DepthFlowProjectionLayer_gpu_forward_ws", (), "input1:f input2:o count:o output:f",
                             (("flow", (0, 3)), ("depth", (1,)), ("count", (2,))), rule="int", quantum=1, code=-1,
                             tail=(1, 0x20000, 1 << 20), tail_types="ipz")),
    ("memc.proj_bwd", _e("", "FlowProjectionLayer_gpu_backward", (), "input1:f count:o gradoutput:f gradinput1:f",
                         (("flow", (0, 2, 3)), ("count", (1,))), rule="int", quantum=1, code=-1)),
    ("memc.dproj_fwd", _e("", "DepthFlowProjectionLayer_gpu_forward", (), "input1:f input2:o count:o output:f",
                          (("flow", (0, 3)), ("depth", (1,)), ("count", (2,))), rule="int", quantum=1, code=-1, tail=(1,))),
    ("memc.dproj_bwd", _e("", "DepthFlowProjectionLayer_gpu_backward", (),
                          "input1:f input2:o count:o output:f gradoutput:f gradinput1:f gradinput2:o",
                          (("flow", (0, 3, 4, 5)), ("depth", (1, 6)), ("count", (2,))), rule="int", quantum=1, code=-1)),
])

GUARDED = [(key, group) for key, e in ENTRIES.items() for group in e.groups]

ABI_B, ABI_C, ABI_H, ABI_W = 2, 3, 33, 72
ARENA_NUMEL = (1 << 31) + (1 << 21)             # the GPU module's arena: the int rule's far side and a little, fp32 elements


def kind_shape(kind, B=ABI_B, C=ABI_C, H=ABI_H, W=ABI_W):
    """the shape of a tensor of `kind` in a call of B x C x H x W (the stack: six neighbours per batch element)"""
    return {"i": (B, C, H, W), "f": (B, 2, H, W), "t": (B, 16, H, W), "o": (B, 1, H, W),
            "I": (6 * B, 3, H, W), "F": (6 * B, 2, H, W), "T": (6 * B, 16, H, W), "x": (B, 64, H, W),
            "s": (B, 8, H, W), "q": (B, 2, H // 2, W // 2), "c": (B, 8, H, W), "u": (B, 2, 4 * H, 4 * W)}[kind]


def abi_layout(key, group, side="far"):
    """The descriptors of entry point `key` with the tensors of `group` (None: no tensor) at the near / far row stride of
    the entry's rule and every other tensor dense: [(shape, strides, byte address)] per tensor, made-up addresses that no
    refused call dereferences.  The group's tensors interleave from one 16-byte-aligned address; the others are dense,
    16-byte aligned and far below it (SPyNet's span check must not see an overlap)."""
    e = ENTRIES[key]
    at_limit = e.groups[group] if group is not None else ()
    lay = Layout()
    out, dense_at = [None] * len(e.tensors), 0x10000
    far_base = 1 << 36                                         # bytes; the dense tensors lie below 2^35
    shapes = [kind_shape(kind) for _name, kind in e.tensors]
    if at_limit:
        H, W = shapes[at_limit[0]][2], shapes[at_limit[0]][3]
        near, far = near_far(rule_of(key, group), H, W, e.quantum)
        stride = far if side == "far" else near
        at = 0
        for i in at_limit:
            B, C, _h, _w = shapes[i]
            wp = pad4(W)
            itemsize = 2 if i in e.half else 4
            out[i] = (shapes[i], (C * wp, wp, stride, 1), far_base + at * 4)
            lay.view(e.tensors[i][0], shapes[i], (C * wp, wp, stride, 1), (far_base + at * 4) // itemsize, itemsize, 16)
            at += B * C * wp                                   # (a slot of fp32 size whatever the storage)
        assert at <= stride
    for i, shape in enumerate(shapes):
        if out[i] is None:
            B, C, H, W = shape
            itemsize = 2 if i in e.half else 4
            out[i] = (shape, (C * H * W, H * W, W, 1), dense_at)
            lay.view(e.tensors[i][0], shape, (C * H * W, H * W, W, 1), dense_at // itemsize, itemsize, 16)
            dense_at += (B * C * H * W * 4 + 0xFFFF) & ~0xFFFF
    assert dense_at < (1 << 35)
    lay.check()
    return out


def group_layout(key, group, stride, nb=ABI_B):
    """The windows of tests/test_gpu_far_views.py for entry point `key` with `group` at row stride `stride`: the group's
    tensors (shapes kind_shape(kind, nb, 3, 33, 72), two-byte elements at the positions in Entry.half) interleave from
    the arena's start in 16-byte aligned slots of the fp32 size.  Returns (Layout, {position: Window})."""
    e = ENTRIES[key]
    lay, wins, at = Layout(), {}, 0
    for i in e.groups[group]:
        b, c, h, w = kind_shape(e.tensors[i][1], nb, 3, ABI_H, ABI_W)
        size = 2 if i in e.half else 4
        wins[i] = lay.view(e.tensors[i][0], (b, c, h, w), (c * pad4(w), pad4(w), stride, 1), at // size, size, 16)
        at += b * c * pad4(w) * 4
    lay.check()
    assert at <= stride * 2 and lay.nbytes <= ARENA_NUMEL * 4
    return lay, wins


def outer_layout(key, group, dim, nb):
    """the same for a far batch (dim 0) or channel (dim 1) stride: far_outer"""
    e = ENTRIES[key]
    lay = Layout()
    wins = far_outer(lay, [(i, kind_shape(e.tensors[i][1], nb, 3, ABI_H, ABI_W), 2 if i in e.half else 4)
                           for i in e.groups[group]], dim)
    lay.check()
    assert lay.nbytes <= ARENA_NUMEL * 4
    return lay, wins
