#!/usr/bin/env python
"""tools/isa_diff.py -- does a source change leave the device code as it was?  Compiles every translation unit of
memc-net_amd/csrc/Makefile device-only to assembly (hipcc --cuda-device-only -S, the Makefile's flags; cross-compiles
without a GPU) in two trees, the product build and the -DMEMC_MEASURE build, and compares each pair of files with the
`__hip_cuid_` lines dropped (that symbol is a hash of the source text).

    python tools/isa_diff.py                      # HEAD against the working tree
    python tools/isa_diff.py BASE [NEW]           # each a directory holding the repository, or a git revision
    python tools/isa_diff.py --only lp_ HEAD      # only the units whose name contains `lp_`

One line per unit: `identical`; `same functions in another order` where the two files hold the same functions -- body,
resource block and metadata entry compared by name, the labels' function numbers dropped -- and the same data around
them (the order of kernels in a code object is the order in which the source first uses each template); or the number
of differing lines followed by the kernels whose resource block (VGPRs, SGPRs, LDS bytes, scratch bytes, occupancy)
changed, old -> new.  Exit status 1 if any unit differs in more than the order."""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("memc-net_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
JOBS = 16

_RES = (("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("lds", r"; LDSByteSize: (\d+)"),
        ("scratch", r"; ScratchSize: (\d+)"), ("occ", r"; Occupancy: (\d+)"))


def make_vars(tree):
    """ARCH, CXXFLAGS and the source lists, read from the tree's own Makefile: a new satellite library needs no edit here"""
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    find = lambda name: re.search(r"^%s\s*[?:]?=\s*(.*)$" % name, text, re.M)
    get = lambda name: find(name).group(1).split() if find(name) else []       # (a list an older Makefile lacks: empty)
    v = {n: get(n) for n in ("ARCH", "CXXFLAGS", "SRCS", "ARMS")}
    # the satellite libraries: SRCS_<NAME> for every NAME of SATELLITES (an older Makefile without that list: every SRCS_*)
    names = get("SATELLITES") or re.findall(r"^SRCS_(\w+)\s*:?=", text, re.M)
    v["SATELLITES"] = [s for n in names for s in get("SRCS_" + n)]
    return v


def units(tree):
    """(label, source, defines): what the libraries are built from, host-only files left out"""
    v = make_vars(tree)
    hip = [s for s in v["SRCS"] if s.endswith(".hip")]
    return ([("product/" + s, s, []) for s in hip + v["SATELLITES"]] +
            [("measure/" + s, s, ["-DMEMC_MEASURE"]) for s in hip + v["ARMS"]])


def materialise(spec, tmp):
    """a directory as it is; a git revision exported (csrc and include only)"""
    if os.path.isdir(os.path.join(spec, CSRC)):
        return os.path.abspath(spec)
    dst = tempfile.mkdtemp(prefix="tree_", dir=tmp)
    ar = subprocess.run(["git", "-C", ROOT, "archive", spec, CSRC, "include"], stdout=subprocess.PIPE, check=True)
    subprocess.run(["tar", "-x", "-C", dst], input=ar.stdout, check=True)
    return dst


def assemble(tree, src, defs, out):
    v = make_vars(tree)
    cmd = [HIPCC, "--offload-arch=" + v["ARCH"][0]] + v["CXXFLAGS"] + ["-I../../include", "-I."] + defs + \
          ["--cuda-device-only", "-S", "-o", out, src]
    r = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on %s in %s:\n%s" % (src, tree, r.stdout[-2000:]))
    return [l for l in open(out).read().split("\n") if "__hip_cuid_" not in l]


def resources(lines):
    """kernel -> {vgpr, sgpr, lds, scratch, occ}, from the comment block the compiler writes behind each kernel"""
    res, cur = {}, None
    for l in lines:
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", l)
        if m:
            cur = res.setdefault(m.group(1), {})
        elif l.startswith("; Function info:"):         # a device function that is not a kernel
            cur = None
        elif cur is not None and l.startswith(";"):
            for key, pat in _RES:
                m = re.match(pat, l)
                if m:
                    cur[key] = int(m.group(1))
    return res


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), text=True, stdout=subprocess.PIPE, check=True).stdout
        return [re.sub(r"^void ", "", re.sub(r"\(.*$", "", o)) for o in out.split("\n")[:len(names)]]
    except Exception:
        return names


_LABEL = re.compile(r"(?<![A-Za-z0-9_])((?:\.L)?(?:BB|JTI|CPI|func_begin|func_end|tmp))\d+")     # .LBB<function number>_<block>, .Lfunc_end<n>


def by_function(lines):
    """({function: its lines, labels without the function number}, {kernel: its metadata entry}, every other line)"""
    funcs, meta, rest, cur, state = {}, {}, [], None, "text"
    for l in lines:
        m = re.search(r"; -- Begin function (\S+)", l)
        if m:
            cur, state = funcs.setdefault(m.group(1), []), "func"
            if rest and rest[-1].startswith("\t.section\t.text." + m.group(1) + ","):       # a template's own section
                cur.append(rest.pop())
        elif state == "csdata" and not l.startswith(";"):          # behind the resource comment block: the function is over
            cur, state = None, "text"
        elif l.startswith("amdhsa.kernels:"):
            cur, state = None, "meta"
        elif state == "meta" and l.startswith("  - "):
            cur = []
            meta[len(meta)] = cur
        elif state == "meta" and not l.startswith("  "):
            cur, state = None, "text"
        if cur is None:
            rest.append(l)
        else:
            cur.append(re.sub(r"\s+;", " ;", _LABEL.sub(r"\1#", l)))      # (a comment's column follows the label's width)
            if state == "func" and ".AMDGPU.csdata" in l:
                state = "csdata"
    name = lambda entry: next(l.split()[-1] for l in entry if l.lstrip().startswith(".name:"))
    return funcs, {name(e): e for e in meta.values()}, rest


def compare(a, b):
    if a == b:
        return "identical", []
    fa, fb = by_function(a), by_function(b)
    if fa == fb:
        return "same functions in another order (%d functions, %d kernels: bodies, resource blocks, metadata equal by name)" % (
            len(fb[0]), len(fb[1])), []
    n = sum(1 for l in difflib.unified_diff(a, b, lineterm="", n=0)
            if l[:1] in "+-" and not l.startswith(("+++", "---")))
    ra, rb = resources(a), resources(b)
    changed = [k for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)]
    fmt = lambda r: "absent" if r is None else "vgpr %(vgpr)s sgpr %(sgpr)s lds %(lds)s scratch %(scratch)s occ %(occ)s" % r
    notes = ["    %s: %s -> %s" % (d, fmt(ra.get(k)), fmt(rb.get(k))) for k, d in zip(changed, demangle(changed))]
    return "%d differing lines, %d of %d kernels with other resources" % (n, len(changed), len(rb)), notes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("base", nargs="?", default="HEAD")
    ap.add_argument("new", nargs="?", default=ROOT)
    ap.add_argument("--only", default="", help="only the units whose label contains this")
    a = ap.parse_args()
    differ = False
    with tempfile.TemporaryDirectory() as tmp:
        base, new = materialise(a.base, tmp), materialise(a.new, tmp)
        todo = [u for u in units(new) if a.only in u[0]]
        with concurrent.futures.ThreadPoolExecutor(max_workers=JOBS) as ex:
            jobs = {}
            for i, (label, src, defs) in enumerate(todo):
                for side, tree in (("a", base), ("b", new)):
                    have = os.path.exists(os.path.join(tree, CSRC, src))
                    jobs[label, side] = ex.submit(assemble, tree, src, defs, os.path.join(tmp, "%d%s.s" % (i, side))) \
                        if have else None
            print("%s -> %s" % (a.base, "working tree" if a.new == ROOT else a.new))
            for label, _, _ in todo:
                if jobs[label, "a"] is None:
                    print("%-44s new unit" % label)
                    continue
                verdict, notes = compare(jobs[label, "a"].result(), jobs[label, "b"].result())
                differ |= not verdict.startswith(("identical", "same functions in another order"))
                print("%-44s %s" % (label, verdict))
                for n in notes:
                    print(n)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
