#!/usr/bin/env python3
"""Are a tree's kernels the code another tree's were?  Compiles the named .hip files of two checkouts to gfx950 assembly and compares
them function by function (a standalone tool; needs hipcc, no GPU).

    python tools/disasm_compare.py <old tree> <new tree> [file.hip ...] [--arch gfx950] [--tmp DIR] [--diff NAME]

<old tree> and <new tree> are repository roots (for the old one: `git worktree add` or `git archive <commit> | tar -x -C DIR`).
Default files: zwz_kernels.hip zwz_lazy.hip zwz_dstream.hip.  Each is compiled with
`hipcc -O3 -std=c++17 --offload-arch=<arch> -S --cuda-device-only`.  Of every function the instruction lines are kept: comments,
directives and blank lines are dropped, the function number in local labels (.LBB<n>_<k>, .Ltmp<n>) and the per-build
__hip_cuid_ symbol are normalised.  Functions are matched by mangled name; a kernel template that gained a trailing `bool`
argument, or a trailing parameter pack, whose old form is the `false` or the empty one is matched to it (the name without `Lb0E` /
`JE` and without the parameter list).  Prints, per
file, how many functions are identical, which differ (instruction counts old -> new; with --diff NAME a unified diff of the functions
whose name contains NAME) and which are new; exit status 1 if any old function differs or is gone.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG = "parallel-data-compression-and-decompression_amd"


def functions(path):
    out, name = {}, None
    for line in open(path):
        line = line.split(";")[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L") and not line.startswith("\t"):
            name = m.group(1)
            out[name] = []
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            name = None
            continue
        if name is None or (s.startswith(".") and not s.startswith(".L")):
            continue
        s = re.sub(r"\.LBB\d+_", ".LBB_", s)
        s = re.sub(r"\.Ltmp\d+", ".Ltmp", s)
        out[name].append(re.sub(r"__hip_cuid_\w+", "__hip_cuid", s))
    return {k: v for k, v in out.items() if k != "amdhsa.kernels" and not k.startswith("__hip_cuid")}


def key(name, olds):
    """a new function's name as the old tree knew it: itself, or its form without a trailing template argument `false`"""
    if name in olds:
        return name
    short = re.sub(r"(Lb0E|JE)EEv.*", "EEv", name)
    for o in olds:
        if short != name and re.sub(r"EEv.*", "EEv", o) == short:
            return o
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("files", nargs="*", default=["zwz_kernels.hip", "zwz_lazy.hip", "zwz_dstream.hip"])
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--diff", default="")
    a = ap.parse_args()
    tmp = a.tmp or tempfile.mkdtemp(prefix="zwz_disasm_")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

    def build(job):
        tag, root, f = job
        out = os.path.join(tmp, "%s_%s.s" % (tag, f))
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=" + a.arch, "-S", "--cuda-device-only", "-o", out,
                               os.path.join(root, PKG, "csrc", f)], stderr=subprocess.DEVNULL)
        return out

    jobs = [(t, r, f) for t, r in (("old", a.old), ("new", a.new)) for f in a.files]
    with ThreadPoolExecutor(len(jobs)) as ex:
        list(ex.map(build, jobs))
    bad = 0
    for f in a.files:
        old = functions(os.path.join(tmp, "old_%s.s" % f))
        new = {}
        for k, v in functions(os.path.join(tmp, "new_%s.s" % f)).items():
            new[key(k, old)] = v
        same = [n for n in old if new.get(n) == old[n]]
        diff = [n for n in old if n in new and new[n] != old[n]]
        gone = [n for n in old if n not in new]
        fresh = [n for n in new if n not in old]
        bad += len(diff) + len(gone)
        print("%s: %d functions in the old tree, %d identical, %d differ, %d gone; %d new" % (f, len(old), len(same), len(diff), len(gone), len(fresh)))
        for n in diff:
            print("  differs  %s  %d -> %d instructions" % (n, len(old[n]), len(new[n])))
            if a.diff and a.diff in n:
                for line in difflib.unified_diff(old[n], new[n], lineterm="", n=1):
                    print("      " + line)
        for n in gone:
            print("  gone     %s" % n)
        for n in fresh:
            print("  new      %s  %d instructions" % (n, len(new[n])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
