"""tests/_far_views.py checked on the CPU, with integers only: the near / far strides against brute-force evaluation of the
guard rules, the disjointness and alignment of every layout the GPU module and the ABI module use, that the far-batch and
far-channel layouts really pass 2^31 elements and 2^32 bytes, and that the helper's table of guarded (entry point, group)
pairs is DESIGN.md's audit table.  No device, no multi-GiB allocation."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _far_views as V                      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_worked_example():
    assert V.near_far(V.fits_u32, 33, 72, 4) == (33554428, 33554432)
    assert 32 * 33554428 + 72 == 1073741768 < 1 << 30 <= 32 * 33554432 + 72
    assert V.near_far(V.fits_int, 33, 72, 4) == (67108860, 67108864)
    # the far strides select the shifted tile grid of the RGB forward and the stack (multiples of 256), the near ones do not
    assert 33554432 % 256 == 0 and 67108864 % 256 == 0 and 33554428 % 256 != 0 and 67108860 % 256 != 0


@pytest.mark.parametrize("rule", [V.fits_u32, V.fits_int, lambda h, w, s: V.owner_4plane(h, w, s, 80),
                                  lambda h, w, s: V.owner_4plane(h, w, s, 1 << 20)],
                         ids=["u32", "int", "4plane-c80", "4plane-c2^20"])
def test_near_far_against_brute_force(rule):
    for h in (2, 3, 17, 33, 600, 4321):
        for w in (1, 5, 70, 72, 1280):
            for q in (1, 4, 256):
                near, far = V.near_far(rule, h, w, q)
                assert far == near + q and near % q == 0
                # every multiple in a window around the pair, evaluated directly
                for s in range(max(near - 64 * q, 0), near + 64 * q + 1, q):
                    assert rule(h, w, s) == (s <= near), (h, w, q, s)
                # and the rule is a statement about the last element of the plane
                assert rule(h, w, near) and not rule(h, w, far)


def test_the_rules_are_the_documented_inequalities():
    for h, w, s in ((33, 72, 33554428), (33, 72, 33554432), (600, 64, 1 << 21), (600, 64, 1 << 22), (1, 9, 1 << 31)):
        last = (h - 1) * s + w
        assert V.fits_u32(h, w, s) == (last * 4 < 2 ** 32)
        assert V.fits_int(h, w, s) == (last <= 2 ** 31 - 1)
        assert V.owner_4plane(h, w, s, 5000) == (4 * (3 * 5000 + last) < 2 ** 32)
    # the view of the issue: 600 rows that lie 2^22 floats apart pass "every stride fits int" and wrap a 32-bit row offset
    assert (1 << 22) <= V.INT32_MAX and not V.fits_int(600, 64, 1 << 22) and V.fits_int(600, 64, 1 << 21)


def test_a_layout_finds_overlap_misalignment_and_wide_strides():
    lay = V.Layout()
    lay.view("a", (1, 1, 2, 8), (0, 0, 100, 1), 0)
    lay.view("b", (1, 1, 2, 8), (0, 0, 100, 1), 8)
    lay.check()
    lay.view("c", (1, 1, 1, 8), (0, 0, 100, 1), 104)             # row 1 of "a" is [100, 108)
    with pytest.raises(AssertionError):
        lay.check()
    with pytest.raises(AssertionError):
        V.Layout().view("d", (1, 1, 2, 8), (0, 0, 1 << 31, 1), 0)
    with pytest.raises(AssertionError):
        V.Layout().view("e", (1, 1, 2, 8), (0, 0, 100, 1), 2, align=16)
    with pytest.raises(AssertionError):
        V.Layout().view("f", (1, 1, 2, 8), (0, 0, 100, 1), 1, itemsize=2, align=8)


B, H, W = 2, 33, 72
GPU_ARENA = V.ARENA_NUMEL


def gpu_specs():
    """every (tensors, stride) the GPU module places: forward and backward of the adaptive warp for 3 and 8 channels, the
    bilinear warp's, at every stride it uses, one group at a time and all together"""
    for C in (1, 3, 8):
        for Wd in (72, 70, 6):
            groups = {"image": [("x", (B, C, H, Wd)), ("gout", (B, C, H, Wd)), ("g1", (B, C, H, Wd))],
                      "flow": [("flow", (B, 2, H, Wd)), ("g2", (B, 2, H, Wd))],
                      "taps": [("filt", (B, 16, H, Wd)), ("g3", (B, 16, H, Wd))]}
            strides = set(V.near_far(V.fits_u32, H, Wd, 4)) | set(V.near_far(V.fits_int, H, Wd, 4)) | \
                set(V.near_far(V.fits_int, H, Wd, 1)) | {V.near_far(V.fits_int, H, Wd, 1)[0] // 256 * 256}
            for stride in sorted(strides):
                for pick in (["image"], ["flow"], ["taps"], ["image", "flow", "taps"]):
                    yield [t for g in pick for t in groups[g]], stride


def test_gpu_layouts_are_disjoint_aligned_and_inside_the_arena():
    n = 0
    for tensors, stride in gpu_specs():
        lay = V.Layout()
        wins, end = V.interleave(lay, tensors, stride)
        lay.check()
        assert lay.nbytes <= GPU_ARENA * 4 <= 10 << 30, (stride, lay.nbytes)
        for w in wins.values():
            assert (w.base * 4) % 16 == 0 and w.strides[2] == stride and all(s <= V.INT32_MAX for s in w.strides)
        # the tensors interleave: row r of every plane lies inside the same row-stride gap
        assert end <= stride
        n += 1
    assert n > 100


@pytest.mark.parametrize("dim,C,nb", [(0, 3, 3), (0, 8, 3), (1, 3, 2), (1, 8, 2), (1, 16, 2)])
def test_far_batch_and_channel_layouts_pass_2G_elements(dim, C, nb):
    lay = V.Layout()
    tensors = [("a", (nb, C, H, W)), ("b", (nb, C, H, W)), ("c", (nb, C, H, W))]
    if dim == 0:
        tensors += [("flow", (nb, 2, H, W)), ("taps", (nb, 16, H, W))]
    wins = V.far_outer(lay, tensors, dim)
    lay.check()
    assert lay.nbytes <= GPU_ARENA * 4 and lay.nbytes <= int(8.8 * 2 ** 30)
    far = 0
    for w in wins.values():
        assert all(s <= V.INT32_MAX for s in w.strides) and (w.base * 4) % 16 == 0
        span = (w.shape[dim] - 1) * w.strides[dim]
        if w.shape[dim] == (nb if dim == 0 else C):
            assert span > 1 << 31 and span * 4 > 1 << 32 and span * 2 > 1 << 32     # elements; bytes of fp32 and of halves
            far += 1
    assert far >= 3


def test_abi_layouts_are_disjoint_and_aligned_for_every_library():
    """the descriptors of tests/test_far_views_abi.py: no two tensors of a call share a byte, every base is 16-byte aligned
    (the stack's rule; 8 for half quads), every stride of a group at its limit is a multiple of the entry's quantum and
    fits int -- so the plane guard is the one thing a far call fails"""
    for key, group in V.GUARDED:
        e = V.ENTRIES[key]
        for side in ("near", "far"):
            layout = V.abi_layout(key, group, side)             # (checks disjointness itself)
            for i, (shape, strides, address) in enumerate(layout):
                assert address % 16 == 0 and all(0 <= s <= V.INT32_MAX for s in strides)
                if i in e.groups[group]:
                    assert all(s % e.quantum == 0 for s in strides[:3])
                    assert V.rule_of(key, group)(shape[2], shape[3], strides[2]) == (side == "near")
                else:
                    assert V.fits_u32(shape[2], shape[3], strides[2])


def test_every_entry_point_s_gpu_layouts():
    """the layouts tests/test_gpu_far_views.py builds for every guarded (entry point, group): group_layout at the near, the
    far and the 256-multiple stride, outer_layout for far batches and channels -- both check disjointness, alignment and
    the arena's size themselves; here also that a far-outer window really passes 2^31 elements and 2^32 bytes"""
    n = 0
    for key, group in V.GUARDED:
        e = V.ENTRIES[key]
        shape = V.kind_shape(e.tensors[e.groups[group][0]][1])
        near, far = V.near_far(V.rule_of(key, group), shape[2], shape[3], e.quantum)
        for stride in (near, far, near // 256 * 256):
            _lay, wins = V.group_layout(key, group, stride)
            for i, w in wins.items():
                assert (w.base * w.itemsize) % 16 == 0 and (w.itemsize == 2) == (i in e.half)
            n += 1
        for dim, nb in ((0, 3), (1, 2)):
            if all(V.kind_shape(e.tensors[i][1], nb)[dim] >= 3 for i in e.groups[group]):
                _lay, wins = V.outer_layout(key, group, dim, nb)
                for w in wins.values():
                    span = (w.shape[dim] - 1) * w.strides[dim]
                    assert span > 1 << 31 and span * w.itemsize > 1 << 32 and all(s <= V.INT32_MAX for s in w.strides)
                n += 1
    assert n > 350


def audit_rows():
    """(entry point, group, guarded?) of DESIGN.md's audit table: the rows between its two markers"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    body = text.split("<!-- addressing-audit:begin -->")[1].split("<!-- addressing-audit:end -->")[0]
    rows = []
    for line in body.splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        if len(cells) >= 6 and re.match(r"^`[\w.]+`$", cells[0]):
            rows.append((cells[0].strip("`"), cells[1].strip("`"), cells[-1]))
    return rows


def test_the_table_is_the_audit_s_guarded_rows():
    rows = audit_rows()
    guarded = sorted((k, g) for k, g, code in rows if code in ("1", "-1"))
    assert guarded == sorted(V.GUARDED), (set(guarded) ^ set(V.GUARDED))
    for k, g, code in rows:
        if code in ("1", "-1"):
            assert int(code) == V.ENTRIES[k].code, (k, g)
        else:
            assert code.startswith("none"), (k, g, code)       # an unguarded row says why it needs no guard
    assert len(rows) > len(guarded)                             # the 64-bit entry points are listed too
